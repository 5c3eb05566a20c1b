"""The view frames' rule on the CPU (include/mgx.h "VIEW FRAMES"): the NumPy composer against the frames the reference's own
Grid.render drew (tests/golden/render/view_frames.npz), and the header's key rule (csrc/mgx_render.h: render_view_key, built by
g++) against the composer and, exhaustively, against a table-driven restatement in a sanitized stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from multigrid_amd import _lib
from tests import render_util as ru
from tests import view_frames_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_fixture_holds_what_the_rule_treats_specially():
    image, dirs, colours, frames = vu.fixture()
    K, v = image.shape[0], image.shape[1]
    assert 10 <= K <= 16 and v == 7 and dirs.shape == colours.shape == (K,)
    assert frames[8, 1].shape == (K, 56, 56, 3) and frames[7, 0].shape == (K, 49, 49, 3)
    assert os.path.getsize(vu.FIXTURE) < 384 * 1024
    t, s = image[..., 0].astype(int), image[..., 2].astype(int)
    own = t[:, v // 2, v - 1]
    assert {5, 6, 7} <= set(own.tolist()), "a carried key, ball and box"
    other = t == 10
    other[:, v // 2, v - 1] = False
    rel = ((s - dirs.astype(int)[:, None, None] + 3) & 3)[other]
    assert len(set(rel.tolist())) >= 3, "other agents in at least three relative directions"
    assert {0, 1, 2} <= set(s[t == 4].tolist()), "doors in all three states"
    assert (t == 0).any(), "unseen cells"


@pytest.mark.parametrize("ts,hl", ((8, 1), (7, 0)))
def test_composer_equals_the_references_frames(ts, hl):
    image, dirs, colours, frames = vu.fixture()
    got = vu.compose_views(image, dirs, colours, ru.host_atlas(ts), bool(hl))
    bad = np.nonzero((got != frames[ts, hl]).any(axis=(1, 2, 3)))[0]
    assert not len(bad), f"views {bad.tolist()} differ from the reference's frames at ts={ts}, highlight={hl}"


def test_header_rule_equals_the_composer_on_random_and_recorded_cells():
    """The g++ build of render_view_key over arbitrary bytes, and over every cell of the recorded views, against the composer's keys."""
    r = np.random.default_rng(7)
    n, v = 4096, 7
    obs = r.integers(0, 256, size=(n, v, v, 3), dtype=np.uint8)
    obs[: n // 2, ..., 0] = r.integers(0, 12, size=(n // 2, v, v))            # half of them with plausible types and colours
    obs[: n // 2, ..., 1] = r.integers(0, 8, size=(n // 2, v, v))
    dirs = r.integers(0, 256, size=n, dtype=np.uint8)
    colours = r.integers(0, 9, size=n, dtype=np.uint8)
    image, fdirs, fcolours, _ = vu.fixture()
    obs, dirs, colours = np.concatenate((obs, image)), np.concatenate((dirs, fdirs)), np.concatenate((colours, fcolours))
    own = np.zeros(obs.shape[:3], np.uint8)
    own[:, v // 2, v - 1] = 1
    per_cell = lambda a: np.broadcast_to(a[:, None, None], obs.shape[:3]).reshape(-1)      # noqa: E731
    for hl in (0, 1):
        want = vu.view_keys(obs, dirs, colours, bool(hl)).reshape(-1)
        got = vu.header_keys(obs.reshape(-1, 3), own.reshape(-1), per_cell(dirs), per_cell(colours), hl)
        assert (got == want).all(), (hl, int((got != want).sum()))
        assert want.min() >= 0 and want.max() < ru.NUM_KEYS


def test_header_rule_exhaustively_under_sanitizers(tmp_path):
    """tests/hostshim/view_shim.cpp as a program of its own, -fsanitize=address,undefined, run directly: 256^3 cells x 4 directions x
    {own, other} x highlight against the table-driven restatement, every key below 2 500."""
    cxx = shutil.which("g++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "view_rule_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-ffp-contract=off", "-Wall", "-Werror", vu.SHIM_SRC, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    m = re.fullmatch(r"checked (\d+) mismatches (\d+) out_of_range (\d+)\s*", p.stdout)
    assert m, p.stdout
    checked, mismatches, out_of_range = (int(g) for g in m.groups())
    assert checked == 256 ** 3 * 4 * 2 * 2 + 6 * 256 * 256 * 2 * 2 and mismatches == 0 and out_of_range == 0


def test_the_exports_are_the_headers_declarations():
    from tests.test_capi import declared_functions
    names = declared_functions()
    for name in ("mgx_render_views", "mgx_render_atlas_planar"):
        assert name in names and name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    assert set(names) == set(_lib.EXPORTS) and _lib.lib().mgx_abi_version() == _lib.ABI_VERSION == 11
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "VIEW FRAMES (additive to ABI 11)" in hdr and "enum { MGX_VIEWS_HIGHLIGHT = 1, MGX_VIEWS_PLANAR = 2 };" in hdr
    assert (_lib.VIEWS_HIGHLIGHT, _lib.VIEWS_PLANAR) == (1, 2)


def test_c_abi_refusals():
    """mgx_render_views / mgx_render_atlas_planar check their arguments before touching the device."""
    import ctypes as C
    from multigrid_amd import EnvSpec
    L, INV = _lib.lib(), _lib.ERR_INVALID_ARGUMENT
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def views(v=7, n=4, obs=p, d=p, col=p, period=1, atlas=p, ts=8, flags=0, frames=p, spec=True):
        sc = EnvSpec(8, 8, 1, 7, max_steps=10).to_c()
        sc.view_size = v
        return L.mgx_render_views(C.byref(sc) if spec else None, n, obs, d, col, period, atlas, ts, flags, frames, None)

    for ts in (0, -1, 65):
        assert views(ts=ts) == INV and L.mgx_render_atlas_planar(ts, p, None) == INV
    assert L.mgx_render_atlas_planar(8, None, None) == INV
    for v in (6, 8, 1, 2, 17, 0, -3):
        assert views(v=v) == INV, v
    assert views(period=0) == INV and views(period=-1) == INV and views(n=-1) == INV and views(flags=4) == INV
    assert views(spec=False) == INV
    for which in ("obs", "d", "col", "atlas", "frames"):
        assert views(**{which: None}) == INV, which
    assert views(n=0, obs=None, frames=None) == _lib.OK
