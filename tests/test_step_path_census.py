"""A census of the step's order-dependent paths over the reference-recorded corpora (tests/golden/randstate_*.npz and conflict_*.npz).

The fused step kernel evaluates every agent against the pre-step state and then decides per env whether that is still exact
(mgx_rules.h: spec_cell_conflict, spec_needs_fallback, event_cutoff, prefix_blocked).  Those decisions only matter where the
visiting order changes the outcome, and random states almost never get there -- so this test COUNTS, with the host shim's path
report (tests/hostshim: step_env(..., path=True)), how often the corpora reach each decision, per kernel form, and asserts minima.
The minima are conditions on the corpus: where one fails, oracle/gen_golden.py: record_conflicts is extended, not the number.

Every env-step counted here is also replayed against the reference's bytes, in the same form, by tests/test_rules_host.py."""
import collections
import os

import numpy as np

from tests import hostshim, util

CENSUS = os.path.join(util.GOLDEN_DIR, "conflict_census.txt")
MIN = 8
ACT = {0: "left", 1: "right", 2: "forward", 3: "pickup", 4: "drop", 5: "toggle", 6: "done"}
TYPE = {1: "empty", 4: "door", 5: "key", 6: "ball", 7: "box"}
STATE = {0: "open", 1: "closed", 2: "locked"}

#: the conflict pair kinds of the scenario table: (writer's action, reader's action, front cell type, door state or None, filled box)
KINDS = {
    "pickup x pickup": (3, 3, 5, None, False),
    "pickup x forward": (3, 2, 5, None, False),
    "drop x forward": (4, 2, 1, None, False),
    "drop x drop": (4, 4, 1, None, False),
    "drop x pickup": (4, 3, 1, None, False),
    "toggle(open door) x forward": (5, 2, 4, 0, False),
    "toggle(closed door) x forward": (5, 2, 4, 1, False),
    "unlock x toggle": (5, 5, 4, 2, False),
    "unlock x forward": (5, 2, 4, 2, False),
    "toggle(box) x pickup": (5, 3, 7, None, False),
    "pickup x toggle(box)": (3, 5, 7, None, False),
    "toggle(box) x forward": (5, 2, 7, None, False),
}
FILLED_KINDS = {
    "toggle(filled box) x pickup": (5, 3, 7, None, True),
    "pickup x toggle(filled box)": (3, 5, 7, None, True),
    "toggle(filled box) x forward": (5, 2, 7, None, True),
    "pickup x pickup (filled box)": (3, 3, 7, None, True),
}
#: the rows of the scenario table that the C2 / C4 spec (agents may overlap, success 'any', failure 'all', no filled boxes) admits
C24_ROWS = ["pickup_pickup", "pickup_forward", "drop_forward", "drop_drop", "drop_pickup", "toggle_open_forward",
            "toggle_closed_forward", "toggle_toggle", "unlock_forward", "togglebox_pickup", "togglebox_forward",
            "drop_before_arriving", "drop_behind_leaving", "goal_other_acts", "goal_beside_conflict", "lava_beside_conflict"]


def group_of(spec):
    """Which fallback commit the kernels run this spec with (mgx_fused_body.inc, P1s): (group, the host shim's form)."""
    if spec.num_agents <= 2:
        return "A<=2", "first"
    if spec.view_size > 7 or spec.num_agents > 4:
        return "prefix", "prefix"
    return "first, A>2", "first"


class Count:
    def __init__(self):
        self.steps = self.fallback = self.suppressing = self.fallback_event = 0
        self.why = collections.Counter()
        self.pairs = collections.Counter()
        self.cutoff = collections.Counter()              # "0", "mid", "A"

    def add(self, p, A):
        self.steps += 1
        self.fallback += p["fallback"]
        for w in p["why"]:
            self.why[w] += 1
        for key in set(p["pairs"]):
            self.pairs[key] += 1                         # env-steps, not pairs
        if p["fallback"]:
            c = p["commit_cutoff"]
            self.cutoff["0" if c == 0 else "A" if c == A else "mid"] += 1
            self.fallback_event += p["ends_all"] or p["ends_self"]
        else:
            self.suppressing += p["suppressed"] > 0

    def kind(self, k):
        w, r, t, s, filled = k
        return sum(n for (pw, pr, pt, ps, pf), n in self.pairs.items() if (pw, pr, pt, pf) == (w, r, t, filled) and s in (None, ps))


def census_of(path, form):
    z, d, spec = util.load_golden(path)
    B, T, A = z["grid0"].shape[0], z["actions"].shape[0], spec.num_agents
    cnt = Count()
    for b in range(B):
        tile, rows = z["grid0"][b].copy(), z["agents0"][b].copy()
        rng, sc, aux = z["rng0"][b].copy(), int(z["step_count0"][b]), z["aux"][b].copy()
        for t in range(T):
            out = hostshim.step_env(spec, tile, rows, np.ascontiguousarray(z["actions"][t, b]), rng, sc, aux, form=form, path=True)
            sc = out["step_count"]
            np.testing.assert_array_equal(tile, z["grid"][t, b])          # (the path counted is one that computes the reference's state)
            np.testing.assert_array_equal(rows, z["agents"][t, b])
            cnt.add(out["path"], A)
    return cnt, z, spec


def merge(counts):
    m = Count()
    for c in counts:
        for f in ("steps", "fallback", "suppressing", "fallback_event"):
            setattr(m, f, getattr(m, f) + getattr(c, f))
        for f in ("why", "pairs", "cutoff"):
            getattr(m, f).update(getattr(c, f))
    return m


def line(name, c, kinds):
    return (f"{name:34s} {c.steps:6d} {c.fallback:6d} {c.why['bad']:4d} {c.why['conflict']:5d} {c.why['presence']:5d} "
            f"{c.cutoff['0']:5d} {c.cutoff['mid']:5d} {c.cutoff['A']:5d} {c.suppressing:6d} {c.fallback_event:6d}  "
            + " ".join(f"{c.kind(k):4d}" for k in kinds.values()))


def census():
    """(the table as text, per file: (group, form, Count, arrays, spec), the files of each group, the groups' merged counts)"""
    per_file, groups = {}, collections.defaultdict(list)
    for path in util.RANDSTATE_GOLDEN + util.CONFLICT_GOLDEN:
        name = os.path.basename(path)[:-4]
        spec = util.load_golden(path)[2]
        g, form = group_of(spec)
        per_file[name] = (g, form) + census_of(path, form)
        groups[g].append(name)
    kinds = dict(KINDS, **FILLED_KINDS)
    head = (f"{'':34s} {'steps':>6s} {'fallbk':>6s} {'bad':>4s} {'confl':>5s} {'pres':>5s} {'cut=0':>5s} {'mid':>5s} {'cut=A':>5s} "
            f"{'suppr':>6s} {'fb+evt':>6s}  pair kinds, in the order of the legend")
    text = ["Census of the step's order-dependent paths (tests/test_step_path_census.py prints this table and compares it).",
            "Columns: env-steps; of them through the sequential fallback; why (unknown action, cell conflict, presence & moved);",
            "the fallback's commit cutoff (0, strictly inside (0, A), A); no-fallback env-steps whose event cutoff suppressed an",
            "effective action; fallback env-steps with an event; env-steps per conflict pair kind (writer x reader).",
            "Pair kinds: " + "; ".join(f"{i + 1} {k}" for i, k in enumerate(kinds)), "", head]
    for corpus in ("randstate_", "conflict_"):
        for name, (g, form, c, z, spec) in per_file.items():
            if name.startswith(corpus):
                text.append(line(f"{name} [{form}]", c, kinds))
        text.append(line(f"  all {corpus}*", merge(v[2] for n, v in per_file.items() if n.startswith(corpus)), kinds))
    text.append("")
    merged = {g: merge(per_file[n][2] for n in names) for g, names in groups.items()}
    for g, c in merged.items():
        text.append(line(f"group {g}", c, kinds))
    return "\n".join(text) + "\n", per_file, groups, merged


def test_the_corpora_reach_every_order_dependent_path():
    text, per_file, groups, merged = census()
    print(text)
    filled_groups = {g for g, names in groups.items() if any(n.startswith("conflict_") and n.endswith("_boxes") for n in names)}

    for g, c in merged.items():
        A_max = max(per_file[n][4].num_agents for n in groups[g])
        for k, kind in KINDS.items():
            assert c.kind(kind) >= MIN, f"group {g}: conflict pair kind '{k}' in {c.kind(kind)} env-steps"
        if g in filled_groups:
            for k, kind in FILLED_KINDS.items():
                assert c.kind(kind) >= MIN, f"group {g}: conflict pair kind '{k}' in {c.kind(kind)} env-steps"
        # the first-agent shortcut starts the loop at 0 or 1; the prefix form anywhere up to A
        want = ("0", "mid", "A") if g == "prefix" else ("0", "mid") if A_max > 2 else ("0",)
        for v in want:
            assert c.cutoff[v] > 0, f"group {g}: no fallback with commit cutoff {v}"
        if g == "A<=2":                                   # (at A = 2 the shortcut's other value, 1, is no value strictly inside (0, A)
            assert sum(c.cutoff.values()) > c.cutoff["0"]  # in the sense above -- it is the 'mid' bucket here all the same)
        assert c.suppressing >= MIN, f"group {g}: the event cutoff suppressed an effective action in {c.suppressing} env-steps"
        assert c.fallback_event >= MIN, f"group {g}: {c.fallback_event} fallback env-steps with an event"
    assert filled_groups, "no conflict file with filled boxes"

    # the C2 / C4 shape, alone: every row of the table its spec admits, and every minimum above from its own file
    g, form, c, z, spec = per_file["conflict_16x16_a4_v7"]
    assert (spec.width, spec.height, spec.num_agents, spec.view_size) == (16, 16, 4, 7)
    assert sorted(util.load_golden(util.CONFLICT_GOLDEN[util.CONFLICT_IDS.index("conflict_16x16_a4_v7")])[1]["conflict_rows"]) \
        == sorted(C24_ROWS)
    held = collections.Counter(r for s in z["scenario"] for r in str(s).split("+"))
    for row in C24_ROWS:
        assert held[row] >= MIN, f"conflict_16x16_a4_v7 holds row {row} {held[row]} times"
    for k, kind in KINDS.items():
        assert c.kind(kind) >= MIN, (k, c.kind(kind))
    assert c.cutoff["0"] > 0 and c.cutoff["mid"] > 0
    assert c.suppressing >= MIN and c.fallback_event >= MIN

    with open(CENSUS) as f:
        assert f.read() == text, "tests/golden/conflict_census.txt is out of date: it is this test's printed table"
