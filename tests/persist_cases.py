"""Cases, inputs and the NumPy model for the producer kernels of the persistent hand-shake (csrc/mgx_aux.hip: persistent_post_kernel,
persistent_wait_kernel, persistent_feed_kernel<4|2|1|0>), shared by tests/test_persist_producers_gpu.py (the kernels against the
model) and tests/test_persist_branch_census.py (which paths each case reaches, derived on the CPU from the launchers' own header).

The model is written from the words of include/mgx.h ("Persistent stepping"): granule q of env b holds, in bits [31:0], the action
bytes of agents 4q .. 4q+3 (i8, little-endian) and, in bits [63:32], the tag.  The bytes of agents >= A are ignored by the consumer,
so comparisons mask them out (`granule_mask`): what the kernels happen to write there is not pinned."""
import collections
import zlib

import numpy as np


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ===================================================================================================================== the model
def gpe_of(A):
    """granules per env"""
    return (A + 3) // 4


def granules_reference(actions, tag):
    """actions i8[B,A], tag -> u64[B, ceil(A/4)]; the bytes of agents >= A are zero here and masked by `granule_mask`"""
    B, A = actions.shape
    gpe = gpe_of(A)
    out = np.zeros((B, gpe), np.uint64)
    for ai in range(A):
        q, j = divmod(ai, 4)
        out[:, q] |= actions[:, ai].astype(np.uint8).astype(np.uint64) << np.uint64(8 * j)
    return out | (np.uint64(tag) << np.uint64(32))


def granule_mask(A):
    """u64[ceil(A/4)]: the tag and the bytes of agents < A"""
    m = np.full(gpe_of(A), 0xFFFFFFFF00000000, np.uint64)
    for ai in range(A):
        q, j = divmod(ai, 4)
        m[q] |= np.uint64(0xFF) << np.uint64(8 * j)
    return m


def decode(granules, A):
    """The consumer's extraction restated (csrc/mgx_fused_body.inc, the persistent branch): u64[B, ceil(A/4)] -> (actions i8[B,A],
    tags u32[B, ceil(A/4)])"""
    B = granules.shape[0]
    acts = np.zeros((B, A), np.int8)
    for q in range(granules.shape[1]):
        for j in range(4):
            if 4 * q + j < A:
                acts[:, 4 * q + j] = ((granules[:, q] >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.uint8).view(np.int8)
    return acts, (granules >> np.uint64(32)).astype(np.uint32)


def random_actions(r, shape):
    """the whole int8 range, about a quarter -1 ("absent")"""
    a = r.integers(-128, 128, size=shape).astype(np.int8)
    a[r.random(shape) < 0.25] = -1
    return a


# ===================================================================================================================== post
#: labels: see tests/test_persist_branch_census.py: post_reached
POST_LABELS = ("gpe == 1", "gpe > 1", "dword read", "byte gather", "last block ragged", "last block full")
PostShape = collections.namedtuple("PostShape", "A B labels")
_ONE, _MANY, _DW, _BY, _RAG, _FULL = POST_LABELS
#: every A at two B at least; B from {1, 255, 256, 257, 1003}; gpe 1, 2, 3, 4, 5, 7, 8 (5 and 7: the reciprocals that are not exact everywhere)
POST_SHAPES = [
    PostShape(1, 255, (_ONE, _BY, _RAG)), PostShape(1, 256, (_ONE, _BY, _FULL)), PostShape(1, 257, (_ONE, _BY, _RAG)),
    PostShape(2, 1, (_ONE, _BY, _RAG)), PostShape(2, 257, (_ONE, _BY, _RAG)),
    PostShape(3, 256, (_ONE, _BY, _FULL)), PostShape(3, 1003, (_ONE, _BY, _RAG)),
    PostShape(4, 1, (_ONE, _DW, _RAG)), PostShape(4, 256, (_ONE, _DW, _FULL)), PostShape(4, 1003, (_ONE, _DW, _RAG)),
    PostShape(5, 255, (_MANY, _BY, _RAG)), PostShape(5, 257, (_MANY, _BY, _RAG)),
    PostShape(7, 1, (_MANY, _BY, _RAG)), PostShape(7, 1003, (_MANY, _BY, _RAG)),
    PostShape(8, 256, (_MANY, _DW, _FULL)), PostShape(8, 257, (_MANY, _DW, _RAG)),
    PostShape(12, 255, (_MANY, _DW, _RAG)), PostShape(12, 1003, (_MANY, _DW, _RAG)),
    PostShape(16, 1, (_MANY, _DW, _RAG)), PostShape(16, 256, (_MANY, _DW, _FULL)),
    PostShape(17, 257, (_MANY, _BY, _RAG)), PostShape(17, 1003, (_MANY, _BY, _RAG)),
    PostShape(25, 255, (_MANY, _BY, _RAG)), PostShape(25, 1003, (_MANY, _BY, _RAG)),
    PostShape(32, 1, (_MANY, _DW, _RAG)), PostShape(32, 257, (_MANY, _DW, _RAG)),
]
POST_TAGS = (1, 2 ** 31 - 1, 2 ** 32 - 1)
POST_GRANULE_OFFSETS = (0, 8)
PostCase = collections.namedtuple("PostCase", "A B act_off gr_off tag labels")


def post_action_offsets(A):
    """byte offsets of the action tensor the launcher accepts at this A"""
    return (0, 4) if A % 4 == 0 else (0, 1, 2, 3)


def _post_cases():
    out = []
    for s in POST_SHAPES:
        for off in post_action_offsets(s.A):
            k = len(out)                        # (the granule offset and the tag go round)
            out.append(PostCase(s.A, s.B, off, POST_GRANULE_OFFSETS[k % 2], POST_TAGS[k % 3], s.labels))
    return out


POST = _post_cases()
POST_IDS = [f"a{c.A}_B{c.B}_act+{c.act_off}_gr+{c.gr_off}_tag{c.tag:x}" for c in POST]


def post_inputs(case):
    """(actions i8[B,A], the actions of the second post)"""
    r = _rng("post", case.A, case.B, case.act_off)
    return random_actions(r, (case.B, case.A)), random_actions(r, (case.B, case.A))


# ===================================================================================================================== feed
#: labels: see tests/test_persist_branch_census.py: feed_reached
FEED_LABELS = ("GB 4", "GB 2", "GB 1", "GB 0", "one workgroup", "several workgroups", "the cap of 32", "short last workgroup",
               "per_wg rounded up", "register chunk only", "second chunk full", "second chunk partial", "third chunk",
               "by-index tail at g_lo == 0", "by-index tail at g_lo > 0")
FeedCase = collections.namedtuple("FeedCase", "A B T act_off waves trace nwg per_wg labels")
#: (A, B, T): the recorded sequence is i8[T,B,A]; act_off: byte offset of the action tensor, a multiple of GB; waves: the length of
#: done[]; trace: with the trace buffer; nwg, per_wg: the launch the case was written for (asserted by the census)
FEED = [
    FeedCase(3, 200, 2, 1, 7, True, 1, 200, ("GB 0", "one workgroup", "by-index tail at g_lo == 0")),
    FeedCase(4, 2049, 3, 4, 2049, False, 2, 1026,
             ("GB 4", "several workgroups", "short last workgroup", "per_wg rounded up", "register chunk only")),
    FeedCase(2, 2049, 3, 2, 7, True, 2, 1026,
             ("GB 2", "several workgroups", "short last workgroup", "per_wg rounded up", "register chunk only")),
    FeedCase(1, 2049, 3, 3, 2049, False, 2, 1026,
             ("GB 1", "several workgroups", "short last workgroup", "per_wg rounded up", "register chunk only")),
    FeedCase(1, 4097, 2, 1, 7, True, 3, 1366, ("GB 1", "several workgroups", "short last workgroup", "register chunk only")),
    FeedCase(5, 1003, 2, 3, 2049, False, 1, 2006, ("GB 0", "one workgroup", "by-index tail at g_lo == 0")),
    FeedCase(7, 30001, 2, 2, 7, True, 30, 2002,
             ("GB 0", "several workgroups", "short last workgroup", "per_wg rounded up", "by-index tail at g_lo > 0")),
    FeedCase(4, 65536, 2, 0, 2049, False, 32, 2048, ("GB 4", "the cap of 32", "register chunk only")),
    FeedCase(4, 67621, 3, 4, 7, True, 32, 2114, ("GB 4", "the cap of 32", "short last workgroup", "second chunk partial")),
    FeedCase(2, 67621, 3, 2, 2049, False, 32, 2114, ("GB 2", "the cap of 32", "short last workgroup", "second chunk partial")),
    FeedCase(1, 67621, 3, 1, 7, True, 32, 2114, ("GB 1", "the cap of 32", "short last workgroup", "second chunk partial")),
    FeedCase(16, 16500, 2, 0, 2049, False, 32, 2064,
             ("GB 4", "the cap of 32", "short last workgroup", "per_wg rounded up", "second chunk partial")),
    FeedCase(1, 140001, 2, 0, 7, True, 32, 4376,
             ("GB 1", "the cap of 32", "short last workgroup", "second chunk full", "third chunk")),
]
FEED_IDS = [f"a{c.A}_B{c.B}_T{c.T}_act+{c.act_off}" for c in FEED]


def feed_gb(A):
    """action bytes a granule takes from the tensor in one load (csrc/mgx_aux.hip: the kernel's template argument)"""
    return 4 if A % 4 == 0 else 2 if A == 2 else 1 if A == 1 else 0


def feed_inputs(case):
    """the recorded sequence, i8[T,B,A]"""
    return random_actions(_rng("feed", case.A, case.B, case.T), (case.T, case.B, case.A))


#: the producer that outlives its consumer: (A, B), T, the value every done[] word holds, the length of done[]
OUTLIVE = dict(A=4, B=2049, T=5, done=2, waves=7)

# ===================================================================================================================== wait
#: labels: see tests/test_persist_branch_census.py: wait_reached
WAIT_LABELS = ("under one wavefront", "ragged 256 boundary", "exactly one pass", "second pass", "ragged second pass")
WAIT_WAVES = (1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4097)
WAIT_TAIL = 64                                  # zero words behind done[0:waves], before the guard
WAIT_LATE_AT = (255, 256, 2047, 2048)           # where, besides 0 and waves - 1, the one late flag sits (those that exist)


def wait_late_positions(waves):
    return sorted({0, waves - 1} | {p for p in WAIT_LATE_AT if p < waves})


# ===================================================================================================================== consumer
#: the two-part post inside a real session: EnvSpec arguments, batch; 6 steps each
TWO_PART = [
    ("16x16_a4_v7_B1003", dict(width=16, height=16, num_agents=4, view_size=7, max_steps=40), 1003),
    ("20x12_a5_v9_B257", dict(width=20, height=12, num_agents=5, view_size=9, max_steps=64), 257),
]
TWO_PART_STEPS = 6
