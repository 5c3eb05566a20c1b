"""The device selection (include/mgx.h "SELECTION") without a GPU.

THE RULE is held to ONE reference: `model`, in NumPy -- `lexsort` over the candidates by (score, index), cut at k, the indices sorted,
padded with `fill` (the reference project has no such notion).  csrc/mgx_select.h -- the statement the kernels are compiled from: the
biased key, the digit split, the threshold and quota arithmetic, and the serial select over host arrays by the same radix passes -- is
built by g++ into a program of its own with its own main(), plain and under ASan / UBSan, and run on case files written here; every
output byte is compared with the model.  Nothing of it is loaded into Python.  The Python layer (`Selector`,
`BatchedMultiGridEnv.selector`) runs through `SelectModel`, a launcher backed by the model, and examples/graph_search.py through an
oracle launcher plus that class and the key tables' model launcher.  tests/test_select_gpu.py holds the kernels to the same model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multigrid_amd
from multigrid_amd import EnvSpec, Selection, Selector, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
TILE, MAX_CHUNKS = 256, 1024                              # csrc/mgx_select.h: SELECT_TILE, SELECT_MAX_CHUNKS


# ---- the rule in NumPy -------------------------------------------------------------------------------------------------------------

def model(n, score, keep, values, k, fill):
    """(index int64 [k], count int32 [2]): THE RULE"""
    cand = np.arange(n, dtype=np.int64) if keep is None else np.flatnonzero(np.asarray(keep).reshape(-1)[:n]).astype(np.int64)
    order = cand if score is None else cand[np.lexsort((cand, np.asarray(score).reshape(-1)[cand]))]
    m = min(k, cand.size)
    chosen = np.sort(order[:m])
    index = np.full(k, fill, dtype=np.int64)
    index[:m] = chosen if values is None else np.asarray(values).reshape(-1)[chosen]
    return index, np.array([m, cand.size], dtype=np.int32)


def threshold(score, keep, k):
    """(T, r, eq, where): the m-th smallest score of the candidates, the quota of its tie group, the group's size and its indices"""
    n = len(score)
    cand = np.arange(n) if keep is None else np.flatnonzero(keep)
    m = min(k, cand.size)
    assert m > 0
    s = np.sort(score[cand].astype(np.int64))
    T = int(s[m - 1])
    where = cand[score[cand] == T]
    return T, m - int((s < T).sum()), int(where.size), where


SCORE_KINDS = ("equal", "full", "low_digit", "mid_digit", "high_digit", "narrow")


def scores_of(kind, n, r):
    """int32 [n].  Together the kinds make each of the three radix passes (bits 31..21, 20..10, 9..0) the deciding one."""
    if kind == "equal":
        return np.full(n, 7, np.int32)
    if kind == "full":                                     # the whole int32 range, with the values that catch the sign
        s = r.integers(I32_MIN, I32_MAX, size=n, endpoint=True).astype(np.int32)
        special = np.array([I32_MIN, -1, 0, I32_MAX], np.int32)
        at = r.permutation(n)[:min(n, 4)]
        s[at] = special[:at.size]
        return s
    if kind == "low_digit":                                # differ only in the lowest digit
        return (np.int64(-123456 << 10) + r.integers(0, 1024, size=n)).astype(np.int32)
    if kind == "mid_digit":                                # differ only in the middle digit
        return ((np.int64(37) << 21) + (r.integers(0, 2048, size=n) << 10) + 515).astype(np.int32)
    if kind == "high_digit":                               # differ only in the highest digit, both signs
        return ((r.integers(-1024, 1024, size=n) << 21) + 77777).astype(np.int32)
    assert kind == "narrow"                                # a level's spread: long tie groups
    return r.integers(0, 8, size=n).astype(np.int32)


def random_case(r, n_max=700):
    """one random call: (n, score | None, keep | None, values | None, k, fill)"""
    n = int(r.integers(0, n_max + 1))
    score = scores_of(SCORE_KINDS[int(r.integers(len(SCORE_KINDS)))], n, r) if r.random() < 0.8 else None
    keep = None
    if score is None or r.random() < 0.7:
        keep = (r.random(n) < r.choice([0.0, 0.01, 0.5, 1.0])).astype(np.uint8) * r.choice([1, 2, 0x80]).astype(np.uint8)
    values = r.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64) if r.random() < 0.5 else None
    cands = n if keep is None else int(np.count_nonzero(keep))
    k = int(r.choice([1, max(1, cands - 1), max(1, cands), cands + 1, n + 5, int(r.integers(1, max(2, n)))]))
    return n, score, keep, values, k, int(r.choice([-1, 12345]))


# ---- csrc/mgx_select.h, built by g++ into a program of its own -----------------------------------------------------------------------

HOST_MAIN = r"""
// reads i64 words: cases; per case: n, k, fill, have (bit 0 score, 1 keep, 2 values), then score[n], keep[n], values[n] as given.
// Every array is allocated at its exact size, so that a sanitized build sees an access past it.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mgx_select.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> w;
    int64_t x;
    while (std::fread(&x, 8, 1, f) == 1) w.push_back(x);
    std::fclose(f);
    size_t at = 0;
    const int64_t cases = w[at++];
    for (int64_t c = 0; c < cases; ++c) {
        const int64_t n = w[at++], k = w[at++], fill = w[at++], have = w[at++];
        std::vector<int32_t> score;
        std::vector<uint8_t> keep;
        std::vector<int64_t> values;
        if (have & 1) for (int64_t i = 0; i < n; ++i) score.push_back((int32_t)w[at++]);
        if (have & 2) for (int64_t i = 0; i < n; ++i) keep.push_back((uint8_t)w[at++]);
        if (have & 4) for (int64_t i = 0; i < n; ++i) values.push_back(w[at++]);
        std::vector<int64_t> index(k, -7);
        std::vector<int32_t> count(2, -7);
        std::vector<uint32_t> hist(mgx::SELECT_MAX_BINS, 0xFFFFFFFFu);
        mgx::select_serial(n, (have & 1) ? score.data() : nullptr, (have & 2) ? keep.data() : nullptr, (have & 4) ? values.data() : nullptr,
                           k, fill, index.data(), count.data(), hist.data());
        std::printf("count %d %d index", count[0], count[1]);
        for (int64_t j = 0; j < k; ++j) std::printf(" %lld", (long long)index[j]);
        std::printf("\n");
    }
    // the key, the digits and the geometry
    const int32_t probes[] = {INT32_MIN, -1, 0, 1, INT32_MAX, 0x12345678};
    for (int32_t s : probes) {
        const uint32_t u = mgx::select_key(s);
        std::printf("key %u digits %u %u %u prefixes %u %u %u\n", u, mgx::select_digit(u, 0), mgx::select_digit(u, 1), mgx::select_digit(u, 2),
                    mgx::select_prefix(u, 0), mgx::select_prefix(u, 1), mgx::select_prefix(u, 2));
        const uint32_t p1 = mgx::select_extend(0, 0, mgx::select_digit(u, 0)), p2 = mgx::select_extend(p1, 1, mgx::select_digit(u, 1));
        if (mgx::select_extend(p2, 2, mgx::select_digit(u, 2)) != u) return 3;
    }
    const int64_t sizes[] = {0, 1, 256, 257, 262144, 262145, 1 << 20, 2147483647LL};
    for (int64_t n : sizes)
        std::printf("n %lld tiles %lld per %lld chunks %lld bytes %zu\n", (long long)n, (long long)mgx::select_tiles(n),
                    (long long)mgx::select_tiles_per_chunk(n), (long long)mgx::select_chunks(n), mgx::select_work_bytes(n));
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("select_host")
    src = d / "select_host.cpp"
    src.write_text(HOST_MAIN)
    inc = ["-I", os.path.join(ROOT, "multigrid_amd", "csrc")]
    exes = {"plain": str(d / "plain"), "sanitized": str(d / "sanitized")}
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-Werror", *inc, str(src), "-o", exes["plain"]])
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           *inc, str(src), "-o", exes["sanitized"]])

    def run(which, payload: bytes):
        path = d / f"input_{which}.bin"
        path.write_bytes(payload)
        p = subprocess.run([exes[which], str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return [ln for ln in p.stdout.split("\n") if ln]
    return run


def payload_of(cases) -> bytes:
    words = [len(cases)]
    for n, score, keep, values, k, fill in cases:
        words += [n, k, fill, (score is not None) | (keep is not None) << 1 | (values is not None) << 2]
        for arr in (score, keep, values):
            if arr is not None:
                words += np.asarray(arr).astype(np.int64).tolist()
    return np.array(words, dtype=np.int64).tobytes()


def lines_of(cases):
    out = []
    for case in cases:
        index, count = model(*case)
        out.append(f"count {count[0]} {count[1]} index" + "".join(f" {int(v)}" for v in index))
    return out


def edge_cases():
    """the hand-made ones: empty input, nobody kept, one item, the sign, ties taken partly, k beyond n"""
    r = np.random.default_rng(5)
    sign = np.array([0, -1, I32_MAX, I32_MIN, 1, -1, I32_MIN, 0], np.int32)
    ties = np.array([3, 1, 3, 3, 0, 3, 3, 9, 3], np.int32)
    cases = [(0, np.zeros(0, np.int32), None, None, 3, 12345), (0, None, np.zeros(0, np.uint8), None, 1, -1),
             (5, scores_of("full", 5, r), np.zeros(5, np.uint8), None, 4, -1), (1, np.array([I32_MIN], np.int32), None, None, 1, -1),
             (1, None, np.array([0x80], np.uint8), np.array([99], np.int64), 2, -1)]
    cases += [(8, sign, None, None, k, -1) for k in range(1, 10)]
    cases += [(9, ties, None, np.arange(100, 109, dtype=np.int64), k, 12345) for k in range(1, 11)]
    cases += [(9, ties, (np.arange(9) % 2 == 0).astype(np.uint8) * 2, None, k, -1) for k in (1, 2, 3, 4, 5, 6)]
    cases += [(9, None, (ties == 3).astype(np.uint8), None, k, -1) for k in (1, 5, 6, 7, 20)]
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_header_program_equals_the_model(host_programs, which):
    r = np.random.default_rng(2024)
    cases = edge_cases() + [random_case(r) for _ in range(400)]
    got = host_programs(which, payload_of(cases))
    want = lines_of(cases)
    assert len(got) >= len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, cases[i][0], cases[i][4])
    # not hollow: cuts, ties taken partly, every kind of argument
    cut = part = 0
    for n, score, keep, values, k, fill in cases:
        _, count = model(n, score, keep, values, k, fill)
        cut += count[1] > count[0]
        if score is not None and count[0] > 0:
            T, q, eq, _ = threshold(score, keep, k)
            part += 0 < q < eq
    assert cut > 50 and part > 30
    assert sum(c[1] is None for c in cases) > 20 and sum(c[2] is None for c in cases) > 20 and sum(c[3] is not None for c in cases) > 50


def test_the_header_program_splits_keys_and_sizes_launches_as_documented(host_programs):
    got = host_programs("plain", payload_of([]))
    keys = [ln for ln in got if ln.startswith("key ")]
    for s, ln in zip((I32_MIN, -1, 0, 1, I32_MAX, 0x12345678), keys):
        u = (s & 0xFFFFFFFF) ^ 0x80000000
        assert ln == f"key {u} digits {u >> 21} {(u >> 10) & 2047} {u & 1023} prefixes 0 {u >> 21} {u >> 10}"
    assert [int(ln.split()[1]) for ln in keys[:5]] == [0, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF]      # signed order, unsigned keys
    sizes = [ln.split() for ln in got if ln.startswith("n ")]
    L = _lib.lib()
    for f in sizes:
        n, tiles, per, chunks, nbytes = (int(f[i]) for i in (1, 3, 5, 7, 9))
        assert tiles == -(-n // TILE) and per == -(-tiles // MAX_CHUNKS) and chunks == (-(-tiles // per) if per else 0) <= MAX_CHUNKS
        assert nbytes == (((16 + 2 * 2048 + 1024 + 2 * min(tiles, MAX_CHUNKS)) * 4 + 15) // 16) * 16 == L.mgx_select_work_bytes(n)
    assert [int(f[5]) for f in sizes] == [0, 1, 1, 1, 1, 2, 4, 8192]          # the tiles a workgroup takes: 2 from n = 2^18 + 1 on


# ---- the Python layer over a launcher backed by the model ----------------------------------------------------------------------------

class SelectModel:
    """`select` / `select_work_bytes` of a backend, on CPU tensors, backed by `model`; it refuses what the entry point refuses.  A
    mixin: it keeps no state but the calls it saw."""

    def select_work_bytes(self, n):
        return (((16 + 2 * 2048 + 1024 + 2 * min(-(-n // TILE), MAX_CHUNKS)) * 4 + 15) // 16) * 16

    def select(self, n, score, keep, values, k, fill, index, count, work):
        if n < 0 or k < 1 or (score is None and keep is None):
            raise _lib.MgxError(_lib.ERR_INVALID_ARGUMENT, "mgx_select")
        assert work.numel() * work.element_size() >= self.select_work_bytes(n)
        assert index.dtype is torch.int64 and tuple(index.shape) == (k,) and count.dtype is torch.int32 and tuple(count.shape) == (2,)
        for t, dtypes in ((score, (torch.int32,)), (keep, (torch.bool, torch.uint8)), (values, (torch.int64,))):
            assert t is None or (t.dtype in dtypes and t.numel() == n and t.is_contiguous())
        as_np = lambda t: None if t is None else (t.view(torch.uint8) if t.dtype is torch.bool else t).reshape(-1).numpy()
        got_index, got_count = model(n, as_np(score), as_np(keep), as_np(values), k, fill)
        index.copy_(torch.from_numpy(got_index))
        count.copy_(torch.from_numpy(got_count))
        self.select_calls = getattr(self, "select_calls", 0) + 1


def cpu_selector(n_max=64):
    return Selector(n_max, "cpu", backend=SelectModel())


def test_select_shapes_flattening_and_out_reuse():
    assert multigrid_amd.Selector is Selector and multigrid_amd.Selection is Selection
    assert "Selector" in multigrid_amd.__all__ and "Selection" in multigrid_amd.__all__
    sel = cpu_selector(64)
    assert sel.n_max == 64 and sel.work.numel() * sel.work.element_size() >= sel.backend.select_work_bytes(64)
    score = torch.tensor([[5, 1, 5], [0, 5, 1]], dtype=torch.int32)             # a [B, A] input goes in as it is, flattened
    res = sel.select(score, k=4)
    assert isinstance(res, Selection) and res.index.dtype is torch.int64 and res.index.shape == (4,)
    assert res.count.dtype is torch.int32 and res.count.tolist() == [4, 6] and res.index.tolist() == [0, 1, 3, 5]
    keep = torch.tensor([[True, False, True], [False, True, True]])
    res = sel.select(score, keep, k=4)
    assert res.index.tolist() == [0, 2, 4, 5] and res.count.tolist() == [4, 4]
    res = sel.select(score, keep, k=2, values=torch.arange(10, 16).view(2, 3), fill=7)
    assert res.index.tolist() == [10, 15] and res.count.tolist() == [2, 4]
    flags = keep.to(torch.uint8) * 0x80                                        # any non-zero byte; no scores: a fixed-shape nonzero
    res = sel.select(keep=flags, k=6)
    assert res.index.tolist() == torch.nonzero(flags.view(-1)).view(-1).tolist() + [-1, -1] and res.count.tolist() == [4, 4]
    again = sel.select(keep=flags, k=6, fill=12345, out=res)                   # out=: the same tensors, nothing allocated
    assert again.index is res.index and again.count is res.count and again.index.tolist()[4:] == [12345, 12345]
    empty = sel.select(torch.zeros((0, 3), dtype=torch.int32), k=2)
    assert empty.index.tolist() == [-1, -1] and empty.count.tolist() == [0, 0]
    assert sel.select(torch.zeros(64, dtype=torch.int32), k=1).count.tolist() == [1, 64]       # numel == n_max is taken


def test_arguments_are_refused_by_name():
    for n_max in (0, -1, 2 ** 31, 64.0, True, None):
        with pytest.raises(ValueError, match="Selector: n_max must be an int"):
            Selector(n_max, "cpu", backend=SelectModel())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Selector(64, "cpu")
    sel = cpu_selector(16)
    score, keep, values = torch.arange(6, dtype=torch.int32), torch.ones(6, dtype=torch.bool), torch.arange(6)
    for bad in (score.to(torch.int64), torch.arange(12, dtype=torch.int32)[::2], [1, 2], score.view(2, 3).t()):
        with pytest.raises(ValueError, match="select: score must be a contiguous int32 tensor on cpu"):
            sel.select(bad, k=2)
    for bad in (keep.to(torch.int32), torch.ones(12, dtype=torch.bool)[::2], [True]):
        with pytest.raises(ValueError, match="select: keep must be a contiguous bool or uint8 tensor on cpu"):
            sel.select(score, bad, k=2)
    for bad in (values.to(torch.int32), torch.arange(12)[::2], 5):
        with pytest.raises(ValueError, match="select: values must be a contiguous int64 tensor on cpu"):
            sel.select(score, keep, k=2, values=bad)
    with pytest.raises(ValueError, match=r"select: keep must have the shape of the other inputs, \(6,\), got \(2, 3\)"):
        sel.select(score, keep.view(2, 3), k=2)
    with pytest.raises(ValueError, match=r"select: values must have the shape of the other inputs, \(6,\), got \(5,\)"):
        sel.select(score, k=2, values=torch.arange(5))
    with pytest.raises(ValueError, match="select: at least one of score and keep is required"):
        sel.select(k=2, values=values)
    with pytest.raises(ValueError, match="select: the inputs hold 17 items, this Selector takes at most n_max = 16"):
        sel.select(torch.zeros(17, dtype=torch.int32), k=2)
    for k in (0, -1, 2 ** 31, 2.0, True, None):
        with pytest.raises(ValueError, match="select: k must be an int"):
            sel.select(score, k=k)
    with pytest.raises(TypeError):
        sel.select(score, keep, 2)                                             # k is keyword-only
    for fill in (1 << 63, 1.5, None, False):
        with pytest.raises(ValueError, match="select: fill must be an int that fits int64"):
            sel.select(score, k=2, fill=fill)
    res = sel.select(score, k=2)
    with pytest.raises(ValueError, match="select: out= must be a Selection"):
        sel.select(score, k=2, out=res.index)
    with pytest.raises(ValueError, match=r"select: out=.index must be a contiguous int64 tensor of shape \(3,\)"):
        sel.select(score, k=3, out=res)
    with pytest.raises(ValueError, match=r"select: out=.count must be a contiguous int32 tensor of shape \(2,\)"):
        sel.select(score, k=2, out=Selection(res.index, res.index))
    assert sel.backend.select_calls == 1                                              # the refused calls launched nothing
    assert sel.select(score, k=2, fill=-(1 << 63)).count.tolist() == [2, 6]


def test_an_env_makes_selectors_on_its_device_with_its_backend():
    from tests.test_env_snapshot import make_env
    from tests.test_state_key import KeyOracle

    class Oracle(KeyOracle, SelectModel):
        pass
    spec = EnvSpec(5, 5, 2, 3, max_steps=6)
    env = make_env("pool", B=7, spec=spec, backend=Oracle(spec))
    sel = env.selector()
    assert isinstance(sel, Selector) and sel.backend is env.backend and sel.device == env.agents.device and sel.n_max == 7
    assert env.selector(100).n_max == 100
    mask = (env.state_key().view(7, 1) >> torch.arange(2)) & 1 != 0              # [B, A] bools made from the env's own keys
    res = sel.select(keep=mask[:, 0].contiguous(), k=7)
    assert res.index[:int(res.count[0])].tolist() == torch.nonzero(mask[:, 0]).view(-1).tolist() and int(res.count[1]) == int(mask[:, 0].sum())
    with pytest.raises(ValueError, match="select: the inputs hold 14 items"):
        sel.select(keep=mask, k=7)
    with pytest.raises(ValueError, match="Selector: n_max"):
        env.selector(0)


def test_the_example_selects_what_the_torch_formulation_selects():
    """examples/graph_search.py with check=True on 112 envs of C2 (Empty-16x16), one root, a beam of 8, through an oracle launcher
    plus the model launchers of the key tables and the selection: at every level both selections equal `nonzero` and the sorted stable
    argsort of the same tensors, and the search finds the goal"""
    import importlib.util
    from multigrid_amd import workloads
    from tests.test_distance import DistOracle
    from tests.test_key_table import KeyTableModel
    from tests.test_state_key import KeyOracle

    class SearchOracle(DistOracle, KeyOracle, KeyTableModel, SelectModel):
        pass
    mod_spec = importlib.util.spec_from_file_location("graph_search", os.path.join(ROOT, "examples", "graph_search.py"))
    mod = importlib.util.module_from_spec(mod_spec)
    mod_spec.loader.exec_module(mod)
    out = mod.run("c2", roots=1, beam=8, depth=40, batch=112, device="cpu", backend=SearchOracle(workloads.spec_of("c2")), capacity=4096,
                  check=True)
    assert out["found"] and out["drops"] == 0 and out["checked"] and out["selections_checked"] == 2 * out["depth"]
    hist = out["history"]
    assert [h[0] for h in hist] == list(range(1, out["depth"] + 1)) and all(1 <= h[1] <= 8 for h in hist[:-1])
    assert out["table_entries"] == 1 + sum(out["new_per_level"]) and out["nodes_expanded"] <= 8 * out["depth"]
    with pytest.raises(ValueError, match="no goal cell"):
        mod.run("c3", batch=64, device="cpu", backend=SearchOracle(workloads.spec_of("c3")))
    with pytest.raises(ValueError, match="not with --graph"):
        mod.run("c2", batch=64, device="cpu", check=True, graph=True)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_c_abi_argument_validation():
    """the return codes of mgx_select in the header's order.  EVERY call here is refused before a launch (the pointers are never
    dereferenced): the answer to n == 0, which is a launch, is tests/test_select_gpu.py's."""
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    p, big, huge = 4096, 2 ** 31, 1 << 40

    def sel(n, score=p, keep=p + 1, values=p, k=4, fill=-1, index=p, count=p, work=p, work_bytes=huge):
        return L.mgx_select(n, score, keep, values, k, fill, index, count, work, work_bytes, None)
    # first: n, k, "score and keep both NULL", index, count -- before n == 0 is answered, whatever else is wrong
    for n in (0, 4, big):
        assert sel(-1) == INV and sel(n, k=0) == INV and sel(n, k=-5) == INV
        assert sel(n, score=None, keep=None) == INV and sel(n, index=None) == INV and sel(n, count=None) == INV
        assert sel(n, k=0, work=None, work_bytes=0) == INV
    # (then n == 0: a launch)
    # then the work buffer and the alignments -- before the sizes are looked at
    for n in (4, big, 1 << 40):
        need = L.mgx_select_work_bytes(n)
        assert sel(n, work=None) == INV and sel(n, work_bytes=0) == INV and sel(n, work_bytes=need - 1) == INV
        assert sel(n, score=p + 2) == INV and sel(n, values=p + 4) == INV and sel(n, index=p + 4) == INV
        assert sel(n, count=p + 2) == INV and sel(n, work=p + 8) == INV and sel(n, work=p + 4, k=big) == INV
    # then the sizes; `keep` is bytes and has no alignment; score, keep (one of them) and values are nullable
    assert sel(big) == UNS and sel(4, k=big) == UNS and sel(1 << 40, k=1 << 40) == UNS
    assert sel(big, keep=p + 3) == UNS and sel(big, score=None, values=None) == UNS and sel(big, keep=None) == UNS
    # mgx_select_work_bytes: monotone in n, and what it reports for n is accepted for n (k too large: refused only at the last step)
    sizes = [0, 1, 2, 255, 256, 257, 1000, 4096, 65536, 262144, 262145, 10 ** 6, 10 ** 7, 2 ** 31 - 1]
    needs = [L.mgx_select_work_bytes(n) for n in sizes]
    assert needs == sorted(needs) and needs[0] > 0 and all(b % 16 == 0 for b in needs) and needs[-1] < 1 << 16
    assert needs == [SelectModel().select_work_bytes(n) for n in sizes] and L.mgx_select_work_bytes(-3) == needs[0]
    for n, need in zip(sizes[1:], needs[1:]):
        assert sel(n, k=big, work_bytes=need) == UNS and sel(n, k=big, work_bytes=need - 1) == INV, n


def test_the_exports_are_the_headers_declarations():
    from tests.test_capi import declared_functions
    names = declared_functions()
    for name in ("mgx_select", "mgx_select_work_bytes"):
        assert name in names and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "SELECTION (additive to ABI 11)" in hdr and "LEFT OUT ON PURPOSE" in hdr
    assert _lib.lib().mgx_select_work_bytes.restype is C.c_size_t
    from multigrid_amd import build, ops
    assert any(u[0] == "mgx_select" for u in build.UNITS) and os.path.join(build.CSRC, "mgx_select.h") in build.DEPS
    assert issubclass(ops.HipBackend, ops.SelectOps) and issubclass(ops.HipBackend, ops.KeyTableOps)
