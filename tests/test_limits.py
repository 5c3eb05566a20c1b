"""The edges of the envelope: the largest shapes every entry point accepts and the first ones it must refuse.

Those are the shapes where the kernels take other code: one env's LDS tile passes 64 KiB (and, with the rollout's staging, most of a
CU's 160 KiB), tile offsets (y * W + x) * cell bytes pass 16 bits, view windows reach coordinates past 128 up to 254, and
`envs_per_wavefront` drops to 1.

CPU (no GPU): every spec check of the C ABI is asked -- the plain step's and the rollouts' launch geometry (`mgx_launch_info`,
`mgx_rollout_info`), and the entry points whose spec check comes before their pointer checks (gen_obs and its one-hot form, the step
with one-hot output and its rollout, `mgx_full_obs`) -- over sides around every limit, agent counts, view sizes, both hook kinds, the
three cell formats and two batches.  The answers are OK or UNSUPPORTED, acceptance shrinks with the grid, an accepted launch fits a CU
and holds its tiles, and the largest accepted square side of each entry point is LIMITS below, the table DESIGN.md section 7 states.

GPU: the largest accepted shapes of every kernel family against the CPU oracle, every output of every step and the state after
it, with agents on the far edges (`util.random_state(edge_agents=True)`); the same cases on the bounds-checked build."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrid_amd import BatchedMultiGridEnv, EnvSpec, _lib, layouts
from multigrid_amd.spec import MgxSpecC
from oracle import binding as ob
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
LDS_PER_CU = 160 * 1024

SIDES = (3, 64, 113, 114, 115, 127, 128, 129, 180, 181, 182, 229, 230, 231, 253, 254, 255)
AGENTS = (1, 2, 3, 5, 16, 32)
VIEWS = (3, 7, 9, 15)
KINDS = ("empty", "blockedunlockpickup")
CELL_BYTES = (1, 2, 3)
BATCHES = (1, 5000)
ENTRIES = ("step", "rollout", "persistent", "gen_obs", "gen_obs_one_hot", "step_one_hot", "rollout_one_hot", "full_obs")

#: The largest accepted square side per entry point and cell format (2 = 16-bit cells, 1 = compact cells, 3 = byte grids), the same
#: for every A <= 32, v <= 15 and env kind unless a kind is named; None = the entry point does not serve that format.  The limit of
#: the fused kernel's entry points is the uint8 position format (one env's tile of a 255 x 255 grid fits a CU's LDS with room to
#: spare); mgx_full_obs stages an env's cells and its output in 64 KiB: (cb + 3) * W * H + 96 bytes.  Device generation (254) is
#: checked after the pointers: the GPU test below measures it.
LIMITS = {
    "step": {2: 255, 1: 255, 3: 255},
    "gen_obs": {2: 255, 1: 255, 3: 255},
    "rollout": {2: 255, 1: ("empty", 255), 3: None},
    "persistent": {2: 255, 1: ("empty", 255), 3: None},
    "step_one_hot": {2: 255, 1: ("empty", 255), 3: None},
    "gen_obs_one_hot": {2: 255, 1: None, 3: None},
    "rollout_one_hot": {2: 255, 1: None, 3: None},
    "full_obs": {2: 114, 1: 127, 3: 104},
}
GENERATION_LIMIT = 254


def _c_spec(W, H, A, V, kind="empty", cb=2) -> MgxSpecC:
    return EnvSpec(W, H, A, V, max_steps=10, env_kind=kind, cell_bytes=cb).to_c()


def _rollout_info_fn():
    L = _lib.lib()
    L.mgx_rollout_info.restype = C.c_int
    L.mgx_rollout_info.argtypes = [C.POINTER(MgxSpecC), C.c_int64, C.c_int32, C.POINTER(_lib.MgxRolloutInfo)]
    return L.mgx_rollout_info


def info_entry(e):
    """the entry points that report a launch geometry (the others are asked at batch 0: see `query`)"""
    return e in ("step", "rollout", "persistent")


def query(entry, sc, batch):
    """(return code, launch geometry or None) of `entry`'s spec check for `sc`.  The entry points that take tensors are asked with
    NULL pointers: at batch 0 the spec check is all they do (OK / UNSUPPORTED); at batch > 0 an accepted spec must then be refused
    for its pointers (INVALID_ARGUMENT) -- which `test_spec_checks_come_before_pointer_checks` holds them to."""
    L = _lib.lib()
    s = C.byref(sc)
    if entry == "step":
        info = _lib.MgxLaunchInfo()
        return L.mgx_launch_info(s, batch, C.byref(info)), info
    if entry in ("rollout", "persistent"):
        info = _lib.MgxRolloutInfo()
        return _rollout_info_fn()(s, batch, int(entry == "persistent"), C.byref(info)), info
    if entry == "gen_obs":
        return L.mgx_gen_obs(s, batch, None, None, None, None, None), None
    if entry == "gen_obs_one_hot":
        return L.mgx_gen_obs_one_hot(s, batch, None, None, None, None, None), None
    if entry == "step_one_hot":
        return L.mgx_step_one_hot(s, batch, None, *([None] * 13)), None
    if entry == "rollout_one_hot":
        args = _lib.MgxStepArgs()
        args.steps, args.one_hot = 2, 1
        return L.mgx_step_ex(s, batch, C.byref(args), None), None
    if entry == "full_obs":
        return L.mgx_full_obs(s, batch, None, None, None, None), None
    raise KeyError(entry)


def _tile_lower_bound(entry, info, W, H, cb):
    """Bytes the tiles of one workgroup need at the least: envs per workgroup x W x H x LDS bytes per cell (compact cells stay one
    byte in LDS; 16-bit cells and byte grids are held as 16-bit cells).  (The resident rollout shapes share the tiles' wall ring,
    kShapes 9: those start above 16384 envs, beyond the batches asked here.)"""
    per_cell = 1 if cb == 1 else 2
    if entry == "step":
        envs = info.envs_per_workgroup
    else:
        envs = info.envs_per_slice * info.slices * (info.threads_per_workgroup // 64)
    return envs * W * H * per_cell


def _sweep(A, V, kind, cb):
    """accepted[entry][batch] = bool[len(SIDES), len(SIDES)] over (W, H), with every answer and geometry checked on the way."""
    acc = {e: {b: np.zeros((len(SIDES), len(SIDES)), bool) for b in BATCHES} for e in ENTRIES}
    for i, W in enumerate(SIDES):
        for j, H in enumerate(SIDES):
            sc = _c_spec(W, H, A, V, kind, cb)
            for e in ENTRIES:
                for b in BATCHES:
                    rc, info = query(e, sc, b if info_entry(e) else 0)
                    ctx = f"{e} {W}x{H} A={A} v={V} {kind} cell_bytes={cb} batch={b}: rc {rc}"
                    assert rc in (OK, UNSUPPORTED), ctx
                    acc[e][b][i, j] = rc == OK
                    if rc == OK and info is not None:
                        assert 0 < info.lds_bytes <= LDS_PER_CU, f"{ctx}: {info.lds_bytes} B of LDS per workgroup"
                        need = _tile_lower_bound(e, info, W, H, cb)
                        assert info.lds_bytes >= need, f"{ctx}: {info.lds_bytes} B of LDS per workgroup < {need} B of tiles"
                        assert info.workgroups >= 1 and info.threads_per_workgroup % 64 == 0, ctx
    return acc


# ---------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("cb", CELL_BYTES)
@pytest.mark.parametrize("kind", KINDS)
def test_spec_checks_answer_ok_or_unsupported_and_acceptance_is_monotone(kind, cb):
    for A in AGENTS:
        for V in VIEWS:
            acc = _sweep(A, V, kind, cb)
            for e in ENTRIES:
                for b in BATCHES:
                    a = acc[e][b]
                    ctx = f"{e} A={A} v={V} {kind} cell_bytes={cb} batch={b}"
                    # down-closed: (W, H) accepted => (W', H') accepted for W' <= W, H' <= H (SIDES ascend)
                    bad = np.argwhere((a[1:, :] & ~a[:-1, :]))
                    assert not len(bad), f"{ctx}: {SIDES[bad[0][0] + 1]}x{SIDES[bad[0][1]]} accepted, a narrower grid refused"
                    bad = np.argwhere((a[:, 1:] & ~a[:, :-1]))
                    assert not len(bad), f"{ctx}: {SIDES[bad[0][0]]}x{SIDES[bad[0][1] + 1]} accepted, a shorter grid refused"
                    assert np.array_equal(a, acc[e][BATCHES[0]]), f"{ctx}: acceptance depends on the batch"


def test_spec_checks_come_before_pointer_checks():
    """With NULL tensors and a batch > 0 the tensor-taking entry points refuse an accepted spec for its pointers and a refused one as
    UNSUPPORTED: what the batch-0 answers of the sweep stand for is the spec check itself."""
    for (W, H) in ((255, 255), (255, 3), (115, 115), (128, 128), (105, 105)):
        for A, V in ((1, 3), (32, 15), (3, 9)):
            for kind in KINDS:
                for cb in CELL_BYTES:
                    sc = _c_spec(W, H, A, V, kind, cb)
                    for e in ENTRIES:
                        if info_entry(e):
                            continue
                        at0, _ = query(e, sc, 0)
                        at_b, _ = query(e, sc, 5000)
                        assert at_b == (INVALID if at0 == OK else at0), f"{e} {W}x{H} A={A} v={V} {kind} cb={cb}: {at0} / {at_b}"


def _largest_square(entry, A, V, kind, cb):
    best = None
    for side in range(3, 256):
        rc, _ = query(entry, _c_spec(side, side, A, V, kind, cb), 5000 if info_entry(entry) else 0)
        assert rc in (OK, UNSUPPORTED)
        if rc == OK:
            assert best == side - 1 or (best is None and side == 3), f"{entry}: acceptance not contiguous at {side}"
            best = side
    return best


@pytest.mark.parametrize("entry", ENTRIES)
def test_largest_accepted_square_side_is_the_documented_table(entry):
    for cb in CELL_BYTES:
        want = LIMITS[entry][cb]
        for kind in KINDS:
            w = want[1] if isinstance(want, tuple) and want[0] == kind else (None if isinstance(want, tuple) else want)
            for A in AGENTS:
                for V in VIEWS:
                    got = _largest_square(entry, A, V, kind, cb)
                    assert got == w, f"{entry} cell_bytes={cb} {kind} A={A} v={V}: largest accepted side {got}, table says {w}"


@pytest.mark.parametrize("cb", CELL_BYTES)
def test_full_obs_refuses_exactly_beyond_its_lds_staging(cb):
    """mgx_full_obs: (cb + 3) * W * H + 96 <= 64 KiB, for every width -- not only squares -- and whatever A and v."""
    for W in range(3, 256):
        Hmax = min(255, (64 * 1024 - 96) // ((cb + 3) * W))
        for H in sorted({3, Hmax, Hmax + 1, 255}):
            if H < 3 or H > 255:
                continue
            rc, _ = query("full_obs", _c_spec(W, H, 2, 7, "empty", cb), 0)
            assert rc == (OK if H <= Hmax else UNSUPPORTED), f"full_obs cell_bytes={cb} {W}x{H}: {rc}"


def test_side_256_is_refused_by_the_spec_and_by_the_c_abi():
    for W, H in ((256, 256), (256, 3), (3, 256), (256, 255)):
        with pytest.raises(ValueError):
            EnvSpec(W, H, 2, 7)
        for kind in KINDS:
            for cb in CELL_BYTES:
                sc = _c_spec(255, 255, 2, 7, kind, cb)
                sc.width, sc.height = W, H
                for e in ENTRIES:
                    for b in (0, 5000):
                        rc, _ = query(e, sc, b)
                        assert rc == UNSUPPORTED, f"{e} {W}x{H} {kind} cell_bytes={cb}: {rc}"
    EnvSpec(255, 255, 32, 15)                                       # (the largest spec is one)
    for bad in (dict(num_agents=33), dict(view_size=17)):
        with pytest.raises(ValueError):
            EnvSpec(**{**dict(width=255, height=255, num_agents=32, view_size=15), **bad})


def _design_table():
    """The limits table of DESIGN.md section 7: {entry: {cell_bytes: text}}."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 7."):text.index("## 8.")]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"^\| `([a-z_]+)`[^|]*\|([^|]*)\|([^|]*)\|([^|]*)\|", line)
        if m:
            rows[m.group(1)] = {2: m.group(2).strip(), 1: m.group(3).strip(), 3: m.group(4).strip()}
    return rows


def test_design_section_7_states_the_table():
    rows = _design_table()
    names = {"step": "mgx_step", "gen_obs": "mgx_gen_obs", "rollout": "mgx_rollout", "persistent": "mgx_step_persistent",
             "step_one_hot": "mgx_step_one_hot", "gen_obs_one_hot": "mgx_gen_obs_one_hot", "rollout_one_hot": "mgx_step_ex",
             "full_obs": "mgx_full_obs"}
    for entry, name in names.items():
        assert name in rows, f"DESIGN.md section 7 has no row for {name}"
        for cb, want in LIMITS[entry].items():
            if want is None:
                text = "—"
            elif isinstance(want, tuple):
                text = f"{want[1]} (hook-free)"
            else:
                text = str(want)
            assert rows[name][cb] == text, f"DESIGN.md section 7, {name}, cell_bytes={cb}: {rows[name][cb]!r}, the library: {text!r}"
    assert rows["mgx_step_generate"] == {2: str(GENERATION_LIMIT), 1: "—", 3: "—"}
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "230×230" not in text and "sides ≤ 254" not in text


def test_full_obs_beyond_the_kernel_limit_is_composed_like_the_reference():
    """BatchedMultiGridEnv.full_obs where mgx_full_obs answers UNSUPPORTED: the tensor is built from the unpacked grid (CPU here: the
    oracle backend stands in for the device and refuses like the library)."""
    class Refusing(util.OracleBackend):
        def full_obs(self, B, grid, agents, out):
            raise _lib.MgxError(UNSUPPORTED, "mgx_full_obs")
    for cb in CELL_BYTES:
        spec = EnvSpec(128, 115, 5, 7, max_steps=20, cell_bytes=cb)
        st = util.random_state(spec, 3, seed=40 + cb, edge_agents=True, box_contents_p=0.0 if cb == 1 else 0.5)
        st["agents"][1, 3, 2:4] = st["agents"][1, 1, 2:4]           # two agents on one cell: the later one is drawn
        env = BatchedMultiGridEnv(spec, 3, "cpu", backend=Refusing(spec))
        env.load_state(st["grid"], st["agents"], validate=False)
        full = env.full_obs().numpy()
        assert full.shape == (3, 128, 115, 3)
        for b in range(3):
            want = ob.full_obs(layouts.grid_from_product(st["grid"][b]), layouts.unpack_agents(st["agents"][b]))
            np.testing.assert_array_equal(full[b], want, err_msg=f"cell_bytes={cb} env {b}")


# ---------------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
NT = ob.max_threads()


def _states(spec, B, seed, distinct=None, **kw):
    """Edge states for B envs; a batch beyond `distinct` repeats a block of that many envs (compared on slices anyway)."""
    n = B if distinct is None else min(B, distinct)
    st = util.random_state(dataclasses.replace(spec, cell_bytes=2), n, seed, edge_agents=True, **kw)
    if n < B:
        st = {k: np.concatenate([v] * (-(-B // n)))[:B] for k, v in st.items()}
    return st


def _pair(spec, B, seed, auto_reset=False, sample=None, distinct=None):
    """(HIP env over B edge states, oracle-backend envs over `sample` slices (all of them by default), the sampled env indices)."""
    hooks = spec.env_kind != "empty"
    st = _states(spec, B, seed, distinct, terminated_p=0.1)
    if auto_reset:
        st["step_count"][::2] = spec.max_steps - 1
    hip = BatchedMultiGridEnv(spec, B, DEV, first_env=5)
    hip.load_state(st["grid"], st["agents"], st["rng"], st["target"] if hooks else None, st["step_count"], validate=False)
    sample = sample or [(0, B)]
    rspec = dataclasses.replace(spec, cell_bytes=2)
    ref = []
    for lo, hi in sample:
        r = BatchedMultiGridEnv(rspec, hi - lo, "cpu", first_env=5 + lo, backend=util.OracleBackend(rspec, nthreads=NT))
        r.load_state(st["grid"][lo:hi], st["agents"][lo:hi], st["rng"][lo:hi], st["target"][lo:hi] if hooks else None,
                     st["step_count"][lo:hi], validate=False)
        ref.append(r)
    if auto_reset:
        pool = util.random_state(rspec, 3, seed + 1, density=0.3, terminated_p=0.0, edge_agents=True)
        for e in [hip] + ref:
            e.set_layout_pool(pool["grid"], pool["agents"], pool["target"] if hooks else None)
    return hip, ref, sample, np.concatenate([np.arange(lo, hi) for lo, hi in sample])


def _ref_step(ref, sample, acts, auto_reset, one_hot):
    outs = []
    for r, (lo, hi) in zip(ref, sample):
        if auto_reset:
            r.reset_done()
        o = r.step(torch.from_numpy(acts[lo:hi]), one_hot=one_hot)
        outs.append([x.numpy().copy() for x in o] + ([r.was_reset.numpy().copy()] if auto_reset else []))
    return [np.concatenate([o[k] for o in outs]) for k in range(len(outs[0]))]


def _check_state(hip, ref, idx, ctx):
    for name in ("grid", "agents", "step_count", "rng") + (("aux",) if hip.spec.env_kind != "empty" else ()):
        want = np.concatenate([getattr(r, name).numpy() for r in ref])
        assert np.array_equal(getattr(hip, name).cpu().numpy()[idx], want), f"{ctx}: {name}"


def _lds(spec, B, roll=False):
    return _lib.launch_info(spec, B, roll=roll)["lds_bytes"]


def run_steps(spec, B, T, auto_reset=False, one_hot=False, sample=None, distinct=None, seed=1):
    hip, ref, sample, idx = _pair(spec, B, seed, auto_reset, sample, distinct)
    ctx = f"{spec.width}x{spec.height} A={spec.num_agents} v={spec.view_size} {spec.env_kind} cell_bytes={spec.cell_bytes} B={B}"
    resets = 0
    for t in range(T):
        acts = util.random_actions(B, spec.num_agents, seed=70 + t)
        got = hip.step(torch.from_numpy(acts).to(DEV), auto_reset=auto_reset, one_hot=one_hot)
        want = _ref_step(ref, sample, acts, auto_reset, one_hot)
        got = [g.cpu().numpy()[idx] for g in got] + ([hip.was_reset.cpu().numpy()[idx]] if auto_reset else [])
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.tobytes() == w.tobytes(), f"{ctx} one_hot={one_hot} auto_reset={auto_reset} step {t}: output {k}"
        _check_state(hip, ref, idx, f"{ctx} step {t}")
        resets += int(got[-1].sum()) if auto_reset else 0
    if auto_reset:
        assert resets >= len(idx) // 2, resets
    hip.check_errors()


def run_gen_obs(spec, B, one_hot=False, seed=2):
    hip, ref, sample, idx = _pair(spec, B, seed)
    got, gd = hip.gen_obs(one_hot=one_hot)
    o, d = ob.gen_obs_batch(dataclasses.replace(spec, cell_bytes=2).as_dict(), ref[0].grid.numpy(), ref[0].agents.numpy(), NT)
    want = ob.one_hot(o) if one_hot else o
    assert got.cpu().numpy().tobytes() == want.tobytes(), f"gen_obs one_hot={one_hot} {spec}"
    np.testing.assert_array_equal(gd.cpu().numpy(), d)


def run_rollout(spec, B, T, auto_reset=False, one_hot=False, seed=3):
    """mgx_rollout* (the T steps in one launch, state in LDS) == T steps == the oracle, every output and the state after."""
    e1, ref, sample, idx = _pair(spec, B, seed, auto_reset)
    e2, _, _, _ = _pair(spec, B, seed, auto_reset)
    acts = np.stack([util.random_actions(B, spec.num_agents, seed=90 + t) for t in range(T)])
    out = e2.rollout(torch.from_numpy(acts).to(DEV), auto_reset=auto_reset, one_hot=one_hot)
    for t in range(T):
        got = e1.step(torch.from_numpy(acts[t]).to(DEV), auto_reset=auto_reset, one_hot=one_hot)
        want = _ref_step(ref, sample, acts[t], auto_reset, one_hot)
        ctx = f"rollout {spec} step {t}"
        for k, key in enumerate(("obs", "dir", "reward", "terminated", "truncated")):
            assert torch.equal(out[key][t], got[k]), f"{ctx}: {key} rollout != step"
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), f"{ctx}: {key} step != oracle"
        if auto_reset:
            assert torch.equal(out["was_reset"][t], e1.was_reset), f"{ctx}: was_reset"
            assert np.array_equal(e1.was_reset.cpu().numpy(), want[5]), f"{ctx}: was_reset vs oracle"
    for n in ("grid", "agents", "rng", "step_count", "aux") + (("episode",) if auto_reset else ()):
        assert torch.equal(getattr(e1, n), getattr(e2, n)), f"rollout {spec}: {n}"
    _check_state(e1, ref, idx, f"rollout {spec}")
    e1.check_errors(); e2.check_errors()


def _full_obs_want(st, b):
    return ob.full_obs(layouts.grid_from_product(st["grid"][b]), layouts.unpack_agents(st["agents"][b])).astype(np.uint8)


def run_full_obs(W, H, cb, B, kernel, sample=None, seed=4):
    spec = EnvSpec(W, H, 4, 7, max_steps=20, cell_bytes=cb)
    rc, _ = query("full_obs", spec.to_c(), 0)
    assert rc == (OK if kernel else UNSUPPORTED), (W, H, cb, rc)
    st = _states(spec, B, seed, distinct=64, box_contents_p=0.0 if cb == 1 else 0.5)
    env = BatchedMultiGridEnv(spec, B, DEV)
    env.load_state(st["grid"], st["agents"], validate=False)
    full = env.full_obs().cpu().numpy()
    for lo, hi in sample or [(0, B)]:
        for b in range(lo, hi):
            assert np.array_equal(full[b], _full_obs_want(st, b)), f"full_obs {W}x{H} cell_bytes={cb} env {b}"


def run_generation(side, B=4, T=6):
    """mgx_step_generate (Empty-Random episode starts generated in the step's launch) at the largest side it takes."""
    from tests.test_layout_gen import _make
    spec = EnvSpec(side, side, 3, 15, max_steps=3)
    gen = dict(kind="empty_random")
    hip, ref = _make(spec, gen, B, DEV), _make(spec, gen, B, "cpu", backend=util.OracleBackend(spec, nthreads=NT))
    for t in range(T):
        act = torch.from_numpy(util.random_actions(B, 3, seed=t, p_missing=0.0))
        got = hip.step(act.to(DEV), auto_reset=True)
        want = [x.clone() for x in ref.step(act)]
        ref.reset_done()
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.cpu().numpy().tobytes() == w.numpy().tobytes(), f"generate {side} step {t}: output {k}"
        assert torch.equal(hip.was_reset.cpu(), ref.was_reset), f"generate {side} step {t}: was_reset"
    for f in ("grid", "agents", "rng", "step_count", "episode"):
        assert torch.equal(getattr(hip, f).cpu(), getattr(ref, f)), f
    assert int(hip.episode.sum()) >= B
    hip.check_errors()


def _wide(W, H, A, V, kind="empty", cb=2, max_steps=40):
    return EnvSpec(W, H, A, V, max_steps=max_steps, joint_reward=kind != "empty", env_kind=kind, cell_bytes=cb)


STREAM_B = 2100


def _stream_case():
    spec = _wide(250, 250, 2, 15)
    assert STREAM_B * 250 * 250 * 2 > 128 << 20 and _lds(spec, STREAM_B) > 64 * 1024
    run_steps(spec, STREAM_B, 2, sample=[(0, 16), (1040, 1056), (STREAM_B - 16, STREAM_B)], distinct=32)


#: name -> the case; each one is a pytest test below and runs again on the bounds-checked build
CASES = {
    # the plain step on every cell format; A = 32 with v = 15 (the most view slots) on a grid of 255 x 253
    "step_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15), 3, 6),
    "step_255x253_a32_v15": lambda: run_steps(_wide(255, 253, 32, 15), 2, 4),
    "step_253x255_a5_v9": lambda: run_steps(_wide(253, 255, 5, 9), 3, 5),
    "step_compact_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15, cb=1), 3, 6),
    "step_bytegrid_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15, cb=3), 3, 6),
    # the fused auto-reset: a layout of the pool copied into the tile
    "autoreset_255_a5_v15": lambda: run_steps(_wide(255, 255, 5, 15, max_steps=3), 4, 6, auto_reset=True),
    "autoreset_compact_255_a2_v15": lambda: run_steps(_wide(255, 255, 2, 15, cb=1, max_steps=3), 4, 6, auto_reset=True),
    "autoreset_bytegrid_255_a2_v7": lambda: run_steps(_wide(255, 255, 2, 7, cb=3, max_steps=3), 4, 6, auto_reset=True),
    # one-hot output: 4 bytes per staged cell
    "one_hot_255_a32_v15": lambda: run_steps(_wide(255, 255, 32, 15), 2, 4, one_hot=True),
    "one_hot_compact_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15, cb=1), 3, 5, one_hot=True),
    "one_hot_autoreset_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15, max_steps=3), 3, 6, auto_reset=True, one_hot=True),
    # a hook env (BlockedUnlockPickup kind, random target box in aux): the aux carve
    "hook_255_a3_v15": lambda: run_steps(_wide(255, 255, 3, 15, "blockedunlockpickup"), 3, 6),
    "hook_autoreset_one_hot_255_a32_v15": lambda: run_steps(_wide(255, 255, 32, 15, "blockedunlockpickup", max_steps=3), 2, 5,
                                                            auto_reset=True, one_hot=True),
    # gen_obs
    "gen_obs_255_a32_v15": lambda: run_gen_obs(_wide(255, 255, 32, 15), 3),
    "gen_obs_one_hot_255_a32_v15": lambda: run_gen_obs(_wide(255, 255, 32, 15), 3, one_hot=True),
    "gen_obs_compact_255_a3_v15": lambda: run_gen_obs(_wide(255, 255, 3, 15, cb=1), 3),
    "gen_obs_bytegrid_255_a3_v15": lambda: run_gen_obs(_wide(255, 255, 3, 15, cb=3), 3),
    # the rollout: its carve keeps the tile beside the staging
    "rollout_255_a32_v15": lambda: run_rollout(_wide(255, 255, 32, 15), 2, 5),
    "rollout_hook_autoreset_255_a3_v15": lambda: run_rollout(_wide(255, 255, 3, 15, "blockedunlockpickup", max_steps=3), 3, 6,
                                                             auto_reset=True),
    "rollout_compact_255_a3_v15": lambda: run_rollout(_wide(255, 255, 3, 15, cb=1), 3, 5),
    "rollout_one_hot_255_a2_v15": lambda: run_rollout(_wide(255, 255, 2, 15), 3, 4, one_hot=True),
    # mgx_full_obs at its exact boundary (square and W = 255), one env per wavefront; the first refused sizes through the fallback
    "full_obs_114_cb2": lambda: run_full_obs(114, 114, 2, 5, True),
    "full_obs_255x51_cb2": lambda: run_full_obs(255, 51, 2, 5, True),
    "full_obs_127_cb1": lambda: run_full_obs(127, 127, 1, 5, True),
    "full_obs_104_cb3": lambda: run_full_obs(104, 104, 3, 5, True),
    "full_obs_115_cb2_fallback": lambda: run_full_obs(115, 115, 2, 3, False),
    "full_obs_128_cb1_fallback": lambda: run_full_obs(128, 128, 1, 3, False),
    "full_obs_255_cb3_fallback": lambda: run_full_obs(255, 255, 3, 3, False),
    # several envs per wavefront (G = 4) over a ragged batch.  (mgx_full_obs' clamp of G * W * H to 65535 cannot bind: G starts at
    # 2048 / (W * H) and only halves, so this is the G > 1 path there is)
    "full_obs_16_many": lambda: run_full_obs(16, 15, 2, 20001, True, sample=[(0, 64), (10000, 10064), (19937, 20001)]),
    # device generation at 254
    "generate_254": lambda: run_generation(GENERATION_LIMIT),
    # streamed tile loads: a grid tensor beyond 128 MiB of 250 x 250 grids
    "streamed_250_a2_v15": _stream_case,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_edge_shapes_vs_oracle(name):
    CASES[name]()


def test_the_edge_cases_take_more_than_64_kib_of_lds():
    """What the GPU cases below are for: one env's tile beyond 64 KiB in every mode (one env per wavefront)."""
    for spec, roll in ((_wide(255, 255, 3, 15), False), (_wide(255, 255, 3, 15, cb=1), False),
                       (_wide(255, 255, 32, 15, "blockedunlockpickup"), True), (_wide(255, 255, 3, 15, cb=1), True)):
        li = _lib.launch_info(spec, 3, roll=roll)
        assert li["envs_per_wavefront"] == 1 and li["lds_bytes"] > 64 * 1024, (spec, li)


@pytest.mark.gpu
def test_device_generation_refuses_255():
    from tests.test_layout_gen import _make
    with pytest.raises(_lib.MgxError) as e:
        env = _make(EnvSpec(255, 255, 3, 15, max_steps=3), dict(kind="empty_random"), 2, DEV)
        env.step(torch.zeros((2, 3), dtype=torch.int8, device=DEV), auto_reset=True)
        env.reset_done()
    assert e.value.code == UNSUPPORTED


@pytest.mark.gpu
def test_fully_obs_wrapper_on_a_128x128_env_vs_oracle():
    """A grid of a size the reference wraps and mgx_full_obs refuses: FullyObsWrapper gives the reference's image."""
    import multigrid_amd as mg
    env = mg.make("MultiGrid-Empty-8x8-v0", size=128, agents=3, agent_view_size=7, device=DEV)
    wrapped = mg.FullyObsWrapper(env)
    assert query("full_obs", env._benv.spec.to_c(), 0)[0] == UNSUPPORTED
    obs, _ = wrapped.reset(seed=3)
    st = util.random_state(env._benv.spec, 1, seed=8, edge_agents=True)
    env._benv.load_state(st["grid"][0], st["agents"][0], validate=False)
    for t in range(4):
        obs = wrapped.observation(env.gen_obs()) if t == 0 else wrapped.step({0: 2, 1: 1, 2: 2})[0]
        g = layouts.grid_from_product(env._benv.grid[0].cpu().numpy())
        a = layouts.unpack_agents(env._benv.agents[0].cpu().numpy())
        want = ob.full_obs(g, a)
        for i in range(3):
            assert obs[i]["image"].shape == (128, 128, 3)
            np.testing.assert_array_equal(obs[i]["image"], want, err_msg=f"step {t} agent {i}")


@pytest.mark.gpu
def test_edge_shapes_on_the_bounds_checked_build():
    """Every case above on lib/libmgx_chk.so (-DMGX_BOUNDS_CHECK=1: each LDS address of the fused kernel asserted inside its
    wavefront's slice), in a process of its own: still bit-exact, and no access out of its slice."""
    from multigrid_amd import build
    assert os.path.exists(build.LIB_CHK), "libmgx_chk.so is missing: __graft_entry__.build() makes it"
    code = ("import ctypes\n"
            "from multigrid_amd import _lib\n"
            "from tests import test_limits as t\n"
            "assert _lib.LIB_PATH.endswith('libmgx_chk.so')\n"
            "for name, case in t.CASES.items():\n"
            "    case()\n"
            "    print('case ok', name, flush=True)\n"
            "v = (ctypes.c_int32 * 2)()\n"
            "assert _lib.lib().mgx_debug_bounds_violations(v) == 0\n"
            "print(f'bounds violations: {v[0]} (last site {v[1]})')\n")
    env = dict(os.environ, MGX_LIBMGX=build.LIB_CHK, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.count("case ok") == len(CASES), out.stdout[-2000:]
    assert "bounds violations: 0 " in out.stdout, out.stdout[-500:]
