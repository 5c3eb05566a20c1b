"""The selection kernels (csrc/mgx_select.hip) against the NumPy model of tests/test_select.py, on the device, byte for byte: `index`
and `count` sit between guard words, and every input is a view one element into a larger allocation.

Which of these tests fail under which mutant of the kernels -- each mutant was built as a library of its own (every one of them in
bounds: a place is stored only below k) and the 74 cases of this file run against it on an MI355X:
  the quota ignored (every item of the        19 cases: test_a_tie_group_over_several_tiles_is_taken_partly, test_sizes_scores_and_k
  threshold's tie group is chosen, placed     [n-narrow] from n = 63 on and three other cases whose threshold is tied,
  by lt_before + eq_before)                   test_keep_variants[narrow], all of test_the_large_sizes, test_determinism_and_n_zero,
                                              test_a_captured_select_replays_on_new_data, test_the_example_runs_a_level_as_one_graph.
                                              (NOT where every score is equal: nothing is smaller than the threshold there, and the
                                              first k of the tie group are what the rule takes too.)
  the sign bit not flipped                    22 cases: test_sizes_scores_and_k[n-full] and [n-high_digit] from n = 63 on (both signs
                                              present), test_keep_variants[full], test_the_work_buffer_is_the_callers, all of
                                              test_the_large_sizes, test_a_captured_select_replays_on_new_data
  the last pass skipped (T = the digits of    63 cases: every case with scores but [1-full] -- all of test_sizes_scores_and_k beside
  the first two passes, then zeros)           it, the tie group, test_keep_variants[full] and [narrow], the work buffer, the large
                                              sizes, determinism, the captured select, the example; the cases without scores pass
  the pads not written                        70 cases: every one that holds a call with k > |C|; the tie group, determinism and the
                                              two smaller large sizes, which cut, pass
  the sum over chunks off by one chunk (a     all 74 cases: a workgroup that counts its own chunk among those before it misplaces
  workgroup counts its own among them)        every item it writes, from n = 1 on"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from multigrid_amd import Selection, Selector, _lib
from tests.test_select import I32_MAX, I32_MIN, MAX_CHUNKS, SCORE_KINDS, TILE, model, scores_of, threshold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = TILE                                                  # the tile of a workgroup: 256 items
GUARD64, GUARD32 = -0x0123456789ABCDEF, -0x01234567
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 5 * T - 7)


def on_device(arr):
    """an input as a view one element into a larger allocation (None stays None)"""
    if arr is None:
        return None
    arr = np.ascontiguousarray(arr)
    full = torch.from_numpy(np.concatenate([arr[:1] * 0 + 1, arr, arr[:1] * 0 + 1]) if arr.size else np.zeros(2, arr.dtype)).to(DEV)
    return full[1:arr.size + 1]


def outputs(k):
    """((index between guards, its view), (count between guards, its view))"""
    index = torch.full((k + 2,), GUARD64, dtype=torch.int64, device=DEV)
    count = torch.full((4,), GUARD32, dtype=torch.int32, device=DEV)
    return (index, index[1:k + 1]), (count, count[1:3])


def check(sel, n, score, keep, values, k, fill, what=None):
    """one call against the model, byte for byte, guards included; returns (index, count) as NumPy arrays"""
    (index_full, index), (count_full, count) = outputs(k)
    res = sel.select(on_device(score), on_device(keep), k=k, values=on_device(values), fill=fill, out=Selection(index, count))
    want_index, want_count = model(n, score, keep, values, k, fill)
    got_index, got_count = index_full.cpu().numpy(), count_full.cpu().numpy()
    assert res.index is index and res.count is count
    assert got_count.tolist() == [GUARD32, *want_count.tolist(), GUARD32], (what, n, k, got_count.tolist(), want_count.tolist())
    assert got_index[0] == GUARD64 and got_index[-1] == GUARD64, (what, n, k)
    assert got_index[1:-1].tobytes() == want_index.tobytes(), (what, n, k, np.flatnonzero(got_index[1:-1] != want_index)[:8].tolist())
    return got_index[1:-1], got_count[1:3]


def ks_of(n, cands):
    return sorted({1, max(1, cands - 1), max(1, cands), cands + 1, n + 9})


@pytest.fixture(scope="module")
def sel():
    return Selector(1 << 20, DEV)


@pytest.mark.parametrize("kind", SCORE_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_scores_and_k(sel, n, kind):
    """n around a wavefront and around one, two and five tiles; every kind of score (each of the three passes the deciding one, the
    sign, ties); k = 1, |C| - 1, |C|, |C| + 1 and beyond n; keep NULL and at a half; values and fill alternate"""
    r = np.random.default_rng(1000 * n + len(kind))
    score = scores_of(kind, n, r)
    values = r.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    for keep in (None, (r.random(n) < 0.5).astype(np.uint8)):
        cands = n if keep is None else int(np.count_nonzero(keep))
        for j, k in enumerate(ks_of(n, cands)):
            check(sel, n, score, keep, values if j % 2 else None, k, 12345 if j % 2 else -1, kind)
    if kind == "full" and n >= 4:
        assert {I32_MIN, -1, 0, I32_MAX} <= set(score.tolist())


def test_a_tie_group_over_several_tiles_is_taken_partly(sel):
    """scores in 0..7 over five tiles: the tie group at the threshold spans every tile and is taken PARTLY (0 < r < #eq), then WHOLLY
    and nothing more (r = #eq), then one item of it (r = 1)"""
    n = 5 * T - 7
    r = np.random.default_rng(77)
    score, values = scores_of("narrow", n, r), r.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    for keep in (None, (r.random(n) < 0.5).astype(np.uint8) * 0x80):
        cand = score if keep is None else score[keep != 0]
        below, upto = int((cand < 3).sum()), int((cand <= 3).sum())
        for k, quota in ((below + (upto - below) // 2, None), (upto, upto - below), (below + 1, 1)):
            thr, q, eq, where = threshold(score, keep, k)
            assert thr == 3 and eq == upto - below and (0 < q < eq if quota is None else q == quota)       # else the case is hollow
            assert len(set((where // T).tolist())) >= 3
            index, count = check(sel, n, score, keep, None, k, -1)
            assert count.tolist() == [k, cand.size]
            check(sel, n, score, keep, values, k, 12345)
            # the part of the tie group that is taken is its FIRST q items
            assert sorted(set(index.tolist()) & set(where.tolist())) == where[:q].tolist()


@pytest.mark.parametrize("kind", ["full", "narrow", None])
def test_keep_variants(sel, kind):
    """keep NULL, all zero (m = 0: every entry `fill`), all set, a half, only the last item, only items of the last tile, and the
    bytes 2 and 0x80, which count as set -- with scores and without"""
    n = 5 * T - 7
    r = np.random.default_rng(31)
    score = None if kind is None else scores_of(kind, n, r)
    last_tile = np.zeros(n, np.uint8)
    last_tile[(n - 1) // T * T:] = r.random(n - (n - 1) // T * T) < 0.7
    odd_bytes = r.choice(np.array([0, 2, 0x80, 0xFF], np.uint8), size=n)
    only_last = np.zeros(n, np.uint8)
    only_last[-1] = 1
    keeps = {"null": None, "none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "half": (r.random(n) < 0.5).astype(np.uint8),
             "last": only_last, "last_tile": last_tile, "bytes": odd_bytes}
    for name, keep in keeps.items():
        if keep is None and score is None:
            continue
        cands = n if keep is None else int(np.count_nonzero(keep))
        for k in ks_of(n, cands)[:4] + [7]:
            index, count = check(sel, n, score, keep, None, k, -1, name)
            if name == "none":
                assert count.tolist() == [0, 0] and (index == -1).all()
            if name == "last":
                assert count.tolist() == [1, 1] and index[0] == n - 1
    assert int(last_tile[:(n - 1) // T * T].sum()) == 0 < int(last_tile.sum())


@pytest.mark.parametrize("n", SIZES)
def test_without_scores_the_call_is_a_nonzero(sel, n):
    r = np.random.default_rng(n)
    for p in (0.01, 0.5, 1.0):
        keep = (r.random(n) < p).astype(np.uint8) * r.choice(np.array([1, 2, 0x80], np.uint8), size=n)
        index, count = check(sel, n, None, keep, None, n, -1)
        want = torch.nonzero(torch.from_numpy(keep)).view(-1).tolist()
        assert index[:count[0]].tolist() == want and count.tolist() == [len(want)] * 2 and (index[count[0]:] == -1).all()
        check(sel, n, None, keep, r.integers(0, 1 << 40, size=n, dtype=np.int64), max(1, len(want) - 1), 12345)
    as_bool = torch.from_numpy(keep != 0).to(DEV)                              # a torch bool tensor is a u8 tensor here
    assert sel.select(keep=as_bool, k=n).index.tolist() == index.tolist()


def test_the_work_buffer_is_the_callers():
    """arbitrary on entry (0xFF everywhere), reused by a second, SMALLER call on other data; and a Selector made for n takes n"""
    r = np.random.default_rng(9)
    own = Selector(2 * T + 3, DEV)
    assert own.work.numel() * 8 >= _lib.lib().mgx_select_work_bytes(2 * T + 3)
    own.work.fill_(-1)
    n = 2 * T + 3
    score, keep = scores_of("full", n, r), (r.random(n) < 0.5).astype(np.uint8)
    check(own, n, score, keep, None, 100, -1)
    check(own, n, None, keep, None, n, -1)
    for m in (T + 1, 65, 1):                                                   # smaller and smaller, the buffer as the last call left it
        check(own, m, scores_of("low_digit", m, r), None, None, max(1, m // 2), 12345)
        check(own, m, scores_of("narrow", m, r), (r.random(m) < 0.5).astype(np.uint8), None, m, -1)
    own.work.fill_(0x5A5A5A5A5A5A5A5A)
    check(own, n, score, keep, r.integers(0, 99, size=n, dtype=np.int64), 7, -1)


@pytest.mark.parametrize("n", [MAX_CHUNKS * T, MAX_CHUNKS * T + 1, 1 << 20])
def test_the_large_sizes(sel, n):
    """the edge of one tile per workgroup (1024 chunks of one tile, then 513 of two) and 2^20 (four tiles a workgroup), once each, the
    beam cut at k = 4096; the threshold's tie group is taken partly"""
    r = np.random.default_rng(n % 1000)
    score = r.integers(-500, 500, size=n).astype(np.int32)
    keep = (r.random(n) < 0.9).astype(np.uint8)
    thr, q, eq, _ = threshold(score, keep, 4096)
    assert 0 < q < eq
    check(sel, n, score, keep, None, 4096, -1)
    if n == 1 << 20:
        check(sel, n, None, keep, None, n, -1)                                 # the compaction at full length


def test_determinism_and_n_zero(sel):
    """two runs give equal bytes; n == 0 answers {0, 0} and all `fill` in one launch and needs no work buffer"""
    n = 5 * T - 7
    r = np.random.default_rng(3)
    score, keep = scores_of("narrow", n, r), (r.random(n) < 0.5).astype(np.uint8)
    a = check(sel, n, score, keep, None, 300, -1)
    sel.work.fill_(-1)
    b = check(sel, n, score, keep, None, 300, -1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in (1, 5, T + 1):
        index, count = check(sel, 0, np.zeros(0, np.int32), None, None, k, 12345)
        assert count.tolist() == [0, 0] and (index == 12345).all()
    (index_full, index), (count_full, count) = outputs(3)
    L, some = _lib.lib(), torch.zeros(4, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    assert L.mgx_select(0, some.data_ptr(), None, None, 3, -9, index.data_ptr(), count.data_ptr(), None, 0, stream) == _lib.OK
    torch.cuda.synchronize()
    assert index_full.tolist() == [GUARD64, -9, -9, -9, GUARD64] and count_full.tolist() == [GUARD32, 0, 0, GUARD32]
    # ... where n > 0 without one is refused, before the launch
    assert L.mgx_select(4, some.data_ptr(), None, None, 3, -9, index.data_ptr(), count.data_ptr(), None, 0, stream) == _lib.ERR_INVALID_ARGUMENT


def test_a_captured_select_replays_on_new_data():
    """one select with scores, keep and values and one without scores in a graph, replayed three times with the inputs rewritten in
    place between the replays: every replay equals the model (the call initialises its work buffer itself)"""
    n, k = 5 * T - 7, 200
    r = np.random.default_rng(12)
    dev = torch.device(DEV)
    own = Selector(n, DEV)
    score, keep = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    values = torch.zeros(n, dtype=torch.int64, device=DEV)
    cur, side, graph = torch.cuda.current_stream(dev), torch.cuda.Stream(dev), torch.cuda.CUDAGraph()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        cut = own.select(score, keep, k=k, values=values, fill=12345)
        flat = Selector(n, DEV)
        nz = flat.select(keep=keep, k=n)
        with torch.cuda.graph(graph, stream=side):
            own.select(score, keep, k=k, values=values, fill=12345, out=cut)
            flat.select(keep=keep, k=n, out=nz)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    for replay, kind in enumerate(("narrow", "full", "equal")):
        s, kp = scores_of(kind, n, r), (r.random(n) < (0.5, 0.9, 0.2)[replay]).astype(np.uint8)
        v = r.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
        score.copy_(torch.from_numpy(s))
        keep.copy_(torch.from_numpy(kp))
        values.copy_(torch.from_numpy(v))
        for o in (*cut, *nz):
            o.fill_(-77)
        own.work.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((cut, model(n, s, kp, v, k, 12345)), (nz, model(n, None, kp, None, n, -1))):
            assert got.index.cpu().numpy().tobytes() == want[0].tobytes() and got.count.cpu().numpy().tobytes() == want[1].tobytes(), replay
        assert int(cut.count[1]) > k == int(cut.count[0]) or kind == "equal"


def test_the_example_runs_a_level_as_one_graph():
    """examples/graph_search.py at C2's batch: eager with --check (both selections of every level against torch), then with --graph
    (the level captured once and replayed): the two status histories are equal, the goal is found, nothing was dropped or skipped
    (run() ends with env.check_errors() and table.check_errors())"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "graph_search.py")
    mod_spec = importlib.util.spec_from_file_location("graph_search", path)
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    eager = mod.run("c2", roots=1, beam=8, depth=40, device=DEV, check=True)
    graph = mod.run("c2", roots=1, beam=8, depth=40, device=DEV, graph=True)
    assert eager["batch"] == 4096 and eager["checked"] and eager["selections_checked"] == 2 * eager["depth"] and graph["graph"]
    assert eager["found"] and graph["found"] and eager["drops"] == graph["drops"] == 0
    assert eager["history"] == graph["history"] and len(eager["history"]) == eager["depth"] > 10
    assert eager["table_entries"] == graph["table_entries"] == 1 + sum(eager["new_per_level"])
