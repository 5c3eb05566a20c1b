#!/usr/bin/env python3
"""Record agents' views drawn by the reference's own Grid.render as fixtures: tests/golden/render/view_frames.npz.

TEST INFRASTRUCTURE -- not product code.  Runs only where the reference is importable, never on the GPU box:

    python tools/gen_view_golden.py

The reference has no entry point for an agent's view as pixels with several agents (get_pov_render raises), but its Grid.render
draws one when it is handed the view as a v x v Grid, the agents in it as Agents and the seen cells as the highlight mask -- the
oracle of the rule in include/mgx.h "VIEW FRAMES".  The views are the 40 of `util.random_state(EnvSpec(12, 10, 5, 7, max_steps=50),
8, seed=3)` observed through oracle.binding.gen_obs_batch; a dozen of them are kept, chosen so that they hold other agents in at
least three relative directions, a carried key, ball and box under the viewer, doors in all three states and unseen cells.  The
reference is imported as tools/gen_render_golden.py imports it, its tile cache switched off.  Every array written is data produced
by the reference (or its input):

    image  u8[K, v, v, 3]   dir u8[K]   colour u8[K]        the views, the viewers' directions and colours
    frames_ts8_hl1  u8[K, 8v, 8v, 3]                        Grid.render(8, agents, highlight_mask = seen cells)
    frames_ts7_hl0  u8[K, 7v, 7v, 3]                        Grid.render(7, agents), no highlight
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gen_golden as gg  # noqa: E402,F401  (puts the reference and oracle/standins on sys.path)
from multigrid.core.agent import Agent  # noqa: E402
from multigrid.core.constants import Color  # noqa: E402
from multigrid.core.grid import Grid  # noqa: E402
from multigrid.core.world_object import WorldObj  # noqa: E402

from multigrid_amd.spec import EnvSpec  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tests import util  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "render", "view_frames.npz")
KEEP = 12


class _NoCache(dict):
    def __setitem__(self, key, value):
        pass


Grid._tile_cache = _NoCache()


def _agent(index, colour, direction, pos):
    a = Agent(index)
    a.state.color = Color.from_index(int(colour)).value
    a.state.dir = int(direction)
    a.state.pos = pos
    return a


def draw(image, direction, colour, ts, highlight):
    """The view through the reference: cells into a v x v Grid, agent cells into Agents turned into the viewer's frame (the viewer
    faces up), the viewer last -- over what its cell holds, the carried object."""
    v = image.shape[0]
    grid, agents = Grid(v, v), []
    for i in range(v):
        for j in range(v):
            t, c, s = (int(x) for x in image[i, j])
            if t == 10:
                agents.append(_agent(len(agents) + 1, c, (s - int(direction) + 3) % 4, (i, j)))
            elif t not in (0, 1):
                grid.set(i, j, WorldObj.decode(t, c, s))
    agents.append(_agent(0, colour, 3, (v // 2, v - 1)))
    mask = (image[..., 0] != 0) if highlight else None
    img = grid.render(ts, agents=agents, highlight_mask=mask)
    assert img.dtype == np.uint8 and img.shape == (v * ts, v * ts, 3)
    return img


def features(image, direction):
    v = image.shape[0]
    f = set()
    own = image[v // 2, v - 1]
    if int(own[0]) in (5, 6, 7):
        f.add(("carried", int(own[0])))
    for i in range(v):
        for j in range(v):
            t, c, s = (int(x) for x in image[i, j])
            if t == 10 and (i, j) != (v // 2, v - 1):
                f.add(("agent", (s - int(direction) + 3) % 4))
            if t == 4:
                f.add(("door", s & 3))
            if t == 0:
                f.add(("unseen",))
    return f


def main():
    spec = EnvSpec(12, 10, 5, 7, max_steps=50)
    st = util.random_state(spec, 8, seed=3)
    obs, dirs = ob.gen_obs_batch(spec.as_dict(), st["grid"], st["agents"])
    images = obs.reshape(-1, 7, 7, 3)
    dirs = dirs.reshape(-1)
    colours = st["agents"][:, :, 0].reshape(-1)
    feats = [features(images[k], dirs[k]) for k in range(len(images))]
    chosen, have = [], set()
    while True:                                                    # greedy cover of every feature the 40 views hold
        gain, k = max((len(feats[k] - have), -k) for k in range(len(images)) if k not in chosen)
        if gain == 0:
            break
        chosen.append(-k)
        have |= feats[-k]
    chosen += [k for k in range(len(images)) if k not in chosen][:max(0, KEEP - len(chosen))]
    chosen = sorted(chosen)
    assert len({f for f in have if f[0] == "agent"}) >= 3 and {("carried", 5), ("carried", 6), ("carried", 7)} <= have
    assert {("door", 0), ("door", 1), ("door", 2), ("unseen",)} <= have, have
    rec = dict(image=images[chosen], dir=dirs[chosen], colour=colours[chosen])
    rec["frames_ts8_hl1"] = np.stack([draw(images[k], dirs[k], colours[k], 8, True) for k in chosen])
    rec["frames_ts7_hl0"] = np.stack([draw(images[k], dirs[k], colours[k], 7, False) for k in chosen])
    np.savez_compressed(OUT, **rec)
    size = os.path.getsize(OUT)
    print(f"{os.path.basename(OUT)}: {len(chosen)} views {chosen}, features {sorted(have)}, {size / 1024:.1f} KiB")
    assert size < 384 * 1024, "the view fixture must stay smaller than the largest render fixture"


if __name__ == "__main__":
    main()
