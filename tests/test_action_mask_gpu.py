"""Effective-action masks on the GPU: action_mask_kernel (csrc/mgx_action_mask.hip) against the NumPy statement of the rule in
tests/test_action_mask.py, bit for bit -- first through the backend on synthetic state sets of valid random states (every member a
view one row into a larger allocation, the output between guard bytes of 0xAA), at the smallest shapes that reach every cell format,
every lane-group size of the launch geometry (csrc/mgx_aux_geom.h: action_mask_geom; `geometry` restates it and
tests/test_action_mask.py holds the restatement to the header) and a wavefront that is full, one env short and one env over; then
through BatchedMultiGridEnv.action_mask and EnvSnapshot.action_mask on small real envs, against the model of an oracle-backed twin.
No index the kernel dereferences is out of range: agents on a border facing out read no cell (include/mgx.h)."""
import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, layouts
from tests import util
from tests.test_action_mask import (EXPAND, MaskOracle, expanded, geometry, hook_examples, model_action_mask, random_rows, spec_for)
from tests.test_env_snapshot import make_env
from tests.test_episode_stats import actions_for
from tests.test_state_key import cell_bytes_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MAX = 2 ** 31 - 1
FILL = 0xAA
ROWS = 70

#: (W, H, cell_bytes): 64x64 in compact cells only
FORMAT = {1: "compact", 2: "16bit", 3: "bytes"}
SHAPES = {f"{W}x{H}_{FORMAT[cb]}": (W, H, cb) for W, H in ((3, 3), (7, 6), (16, 16)) for cb in (2, 1, 3)}
SHAPES["64x64_compact"] = (64, 64, 1)
KIND_OF = ("empty", "redbluedoors", "rules")


def backend(spec):
    from multigrid_amd.ops import HipBackend
    return HipBackend(spec, torch.device(DEV))


class MaskSet:
    """`rows` valid random states (tests/test_action_mask.py: random_rows) in the three members a mask reads.  guard=True: each
    member is a view one row into an allocation with a row of other bytes on either side; guard=False: the members ARE their
    allocations -- row 0 starts one, the last row ends it."""

    def __init__(self, spec, rows, seed, guard=True, states=None):
        r = np.random.default_rng(seed)
        self.spec, self.rows, self.cb = spec, rows, cell_bytes_of(spec)
        self.host = states if states is not None else random_rows(r, rows, spec.width, spec.height, spec.num_agents, self.cb, spec.env_kind)
        self.dev, self.keep = {}, []
        for m, arr in self.host.items():
            arr = arr.view(np.int16) if arr.dtype == np.uint16 else arr      # (the 16-bit cells: torch's int16)
            if guard:
                pad = r.integers(0, 256, size=(1,) + arr.shape[1:]).astype(arr.dtype)
                full = torch.from_numpy(np.concatenate([pad, arr, pad])).to(DEV)
                self.keep.append(full)
                self.dev[m] = full[1:rows + 1]
            else:
                self.dev[m] = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)
        self._model = {}

    def model(self, aux=True):
        if aux not in self._model:
            h = self.host
            self._model[aux] = model_action_mask(self.cb, h["cells"], h["agents"], h["aux"] if aux else None, self.spec)
        return self._model[aux]


def mask_both(be, st, n, idx, flags, ctx, aux=True, bad=True, lead=1, stream=None):
    """one mgx_action_mask and the model's masks: the output bytes (they start `lead` bytes into a buffer of 0xAA: an odd address at
    lead = 1), the guard bytes around them and the bad words"""
    A = st.spec.num_agents
    per = A * (7 if flags & EXPAND else 1)
    idx = None if idx is None else np.asarray(idx, dtype=np.int64)
    full = torch.full((lead + n * per + 16,), FILL, dtype=torch.uint8, device=DEV)
    out = full[lead:lead + n * per]
    assert out.data_ptr() % 2 == lead % 2
    out = out.view(n, A, 7) if flags & EXPAND else out.view(n, A)
    bad_d = torch.tensor([0, INT32_MAX], dtype=torch.int32, device=DEV) if bad else None
    rows = dict(st.dev) if aux else {m: t for m, t in st.dev.items() if m != "aux"}
    idx_d = None if idx is None else torch.from_numpy(idx).to(DEV)
    if stream is None:
        be.action_mask(n, rows, st.rows, idx_d, flags, out, bad_d)
    else:
        stream.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
        with torch.cuda.stream(stream):
            be.action_mask(n, rows, st.rows, idx_d, flags, out, bad_d)
        stream.synchronize()
    per_row = st.model(aux)
    per_row = expanded(per_row).reshape(st.rows, per) if flags & EXPAND else per_row
    src = np.arange(n) if idx is None else idx
    ok = (src >= 0) & (src < st.rows)
    want = np.full(lead + n * per + 16, FILL, np.uint8)
    body = want[lead:lead + n * per].reshape(n, per)
    body[ok] = per_row[src[ok]]
    got = full.cpu().numpy()
    assert (got[:lead] == FILL).all() and (got[lead + n * per:] == FILL).all(), ctx + ": a guard byte was written"
    assert got.tolist() == want.tolist(), ctx
    if bad:
        first = int(np.flatnonzero(~ok)[0]) if (~ok).any() else INT32_MAX
        assert bad_d.cpu().tolist() == [int((~ok).sum()), first], ctx + ": bad"


@pytest.mark.parametrize("A", [1, 2, 3, 5, 32])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_model(shape, A):
    W, H, cb = SHAPES[shape]
    case = list(SHAPES).index(shape) + A
    kind = KIND_OF[case % 3]
    spec = spec_for(W, H, A, cb, kind, overlap=bool(case % 2))
    be = backend(spec)
    r = np.random.default_rng(A * 100 + W * H + cb)
    st = MaskSet(spec, ROWS, 7 + case)
    assert geometry(A, ROWS)[0] == {1: 1, 2: 2, 3: 4, 5: 8, 32: 32}[A]
    for k, n in enumerate((1, 63, 64, 65)):
        flags = EXPAND if k % 2 else 0
        ctx = f"{shape} A={A} {kind} n={n} flags={flags}"
        mask_both(be, st, n, None, flags, ctx + " identity", aux=k != 2, lead=k % 2)
        mask_both(be, st, n, r.permutation(ROWS)[:n], EXPAND - flags, ctx + " permutation", lead=1 - k % 2)
        mask_both(be, st, n, r.integers(0, ROWS, size=n), flags, ctx + " repeats", bad=k % 2 == 0, aux=kind != "empty" or k == 1)
    ids = r.integers(0, ROWS, size=65)
    ids[0], ids[5], ids[64] = -1, ROWS, -1                                    # == rows, and negative: counted, their bytes left alone
    mask_both(be, st, 65, ids, 0, f"{shape} A={A} out of range")
    mask_both(be, st, 65, ids, EXPAND, f"{shape} A={A} out of range, expanded", lead=3)
    ids[5], ids[64] = 2 ** 40, -2 ** 40
    mask_both(be, st, 65, ids, EXPAND, f"{shape} A={A} far out of range, nobody counts", bad=False, aux=False)


@pytest.mark.parametrize("cb", [2, 1, 3])
def test_border_agents_facing_out_in_the_first_and_the_last_row_of_the_allocation(cb):
    """four agents on the four borders facing out (and a fifth in a corner, facing out too): their front position is outside the
    grid, so no cell is read for them -- in env row 0 the cell 'before' their tile would lie before the allocation, in the last row
    behind it.  Their masks are the turns alone."""
    W, H, A = 7, 6, 5
    spec = spec_for(W, H, A, cb, "rules", overlap=False)
    states = random_rows(np.random.default_rng(40 + cb), ROWS, W, H, A, cb, "rules")
    out = np.array([(2, 0, 3), (3, 4, 0), (0, W - 1, 2), (1, 2, H - 1), (1, W - 1, H - 1)], np.uint8)      # (dir, x, y)
    for row in (0, ROWS - 1):
        states["agents"][row, :, 1:4] = out
        states["agents"][row, :, 4] = 0
        states["aux"][row, 0], states["aux"][row, 1:4] = 1, (2, W, 2)         # (a rule that names agent 2's front position, beside
                                                                              #  the grid: no bit)
    st = MaskSet(spec, ROWS, 0, guard=False, states=states)
    assert st.model()[0].tolist() == [3] * A and st.model()[ROWS - 1].tolist() == [3] * A
    be = backend(spec)
    mask_both(be, st, ROWS, None, 0, f"borders cb={cb}")
    mask_both(be, st, 4, [0, ROWS - 1, ROWS - 1, 0], EXPAND, f"borders cb={cb} expanded")


def test_a_stale_door_and_a_rule_with_and_without_aux():
    for spec, rows, want in hook_examples():
        for cb in (3, 2, 1):
            cells = rows["cells"] if cb == 3 else (layouts.pack_cells8(rows["cells"]) if cb == 1 else layouts.pack_cells(rows["cells"]))
            sp = spec_for(spec.width, spec.height, spec.num_agents, cb, spec.env_kind)
            aux = rows["aux"] is not None
            states = {"cells": np.ascontiguousarray(cells), "agents": rows["agents"]}
            if aux:
                states["aux"] = rows["aux"]
            st = MaskSet(sp, 1, 1, states=states)
            assert st.model(aux).tolist() == want
            mask_both(backend(sp), st, 1, None, 0, f"{spec.env_kind} cb={cb} aux={aux}", aux=aux)
            mask_both(backend(sp), st, 3, [0, 0, 0], EXPAND, f"{spec.env_kind} cb={cb} aux={aux} expanded", aux=aux)


def test_a_launch_on_another_stream():
    spec = spec_for(16, 16, 3, 2, "redbluedoors", overlap=False)
    st = MaskSet(spec, ROWS, 5)
    side = torch.cuda.Stream(torch.device(DEV))
    mask_both(backend(spec), st, 65, None, 0, "side stream", stream=side)
    mask_both(backend(spec), st, 65, np.arange(65)[::-1].copy(), EXPAND, "side stream, expanded", stream=side)


# ---- real envs ---------------------------------------------------------------------------------------------------------------------

EMPTY8 = EnvSpec(8, 8, 2, 7, max_steps=8, allow_agent_overlap=False)
BUP = EnvSpec(16, 16, 4, 7, max_steps=1024, joint_reward=True, allow_agent_overlap=False, env_kind="blockedunlockpickup")


def test_blockedunlockpickup_envs_and_their_snapshot_have_the_models_masks():
    B = 64
    st = util.random_state(BUP, B, seed=5, box_contents_p=0.6)
    env = BatchedMultiGridEnv(BUP, B, DEV)
    env.load_state(st["grid"], st["agents"], st["rng"], st["target"], st["step_count"])
    want = model_action_mask(3, st["grid"], st["agents"], st["target"], BUP)
    assert all((((want >> b) & 1) == 1).any() and ((((want >> b) & 1) == 0) & (want != 0)).any() for b in range(2, 6))
    mask = env.action_mask()
    assert mask.dtype is torch.uint8 and mask.cpu().numpy().tolist() == want.tolist()
    wide = env.action_mask(expand=True)
    assert wide.dtype is torch.bool and wide.cpu().numpy().tolist() == expanded(want).astype(bool).tolist()
    snap = env.snapshot()
    for t in range(3):
        env.step(torch.from_numpy(util.random_actions(B, BUP.num_agents, seed=t, p_missing=0.0)).to(DEV))
    assert (env.action_mask() != mask).any()
    rows = torch.tensor([3, 3, B - 1, B, 0], device=DEV)                       # (one row out of range: left alone, and counted)
    out = torch.full((5, BUP.num_agents), FILL, dtype=torch.uint8, device=DEV)
    assert snap.action_mask(rows, out=out) is out
    assert out.cpu().tolist() == want[[3, 3, B - 1]].tolist() + [[FILL] * BUP.num_agents, want[0].tolist()]
    with pytest.raises(ValueError, match=r"1 pair\(s\) named an env id or a snapshot row out of range.*first at pair 3"):
        env.check_errors()
    env.restore(snap)
    assert torch.equal(env.action_mask(), mask)
    env.check_errors()


def test_a_step_and_its_masks_in_one_graph():
    B, A = 130, 2
    env = make_env("pool", B=B, spec=EMPTY8, dev=DEV)
    twin = make_env("pool", B=B, spec=EMPTY8, backend=MaskOracle(EMPTY8))
    acts = actions_for(B, A, 5, 1)
    buf = acts[0].to(DEV).clone()
    mask = torch.zeros((B, A), dtype=torch.uint8, device=DEV)
    cur = torch.cuda.current_stream(torch.device(DEV))
    side, graph = torch.cuda.Stream(torch.device(DEV)), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        env.step(buf, auto_reset=True); env.action_mask(out=mask)             # (everything bound and allocated before the capture)
        with torch.cuda.graph(graph, stream=side):
            env.step(buf, auto_reset=True)
            env.action_mask(out=mask)
    cur.wait_stream(side)
    twin.step(acts[0], auto_reset=True)
    assert mask.cpu().tolist() == twin.action_mask().tolist()
    seen = set()
    for t in range(1, 4):                                                     # three replays, each another step
        buf.copy_(acts[t].to(DEV))
        mask.fill_(FILL)
        graph.replay()
        twin.step(acts[t], auto_reset=True)
        assert mask.cpu().tolist() == twin.action_mask().tolist(), t
        assert env.agents.cpu().tolist() == twin.agents.tolist(), t
        seen |= set(mask.cpu().reshape(-1).tolist())
    assert {3, 3 | 4} <= seen
    env.check_errors()


def test_the_example_forks_only_the_children_that_can_differ():
    """examples/masked_expand.py on 2048 envs of C3 (BlockedUnlockPickup): 8 roots, three levels; every level is also expanded 7 ways
    inside the example, and the two expansions must reach the same states"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "masked_expand.py")
    mod_spec = importlib.util.spec_from_file_location("masked_expand", path)
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c3", roots=8, depth=3, batch=2048, device=DEV)
    levels = out["frontier_per_level"]
    assert out["batch"] == 2048 and out["verified"] and len(levels) == 4 and levels[0] == 8 < levels[1] < levels[2] <= 2048 // 7
    assert 0 < out["forks"] < out["forks_7way"] == 6 * sum(levels[:3]) and out["forks_saved"] > 0.2
