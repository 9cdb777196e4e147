"""tests/pip_model.py against plain arithmetic, and the scenario table of tests/pip_cases.py against the model: the table
meets every (site, branch) pair of the cooperative bucket kernels' workgroup algorithm.  No library, no GPU."""
import random

import pytest

import pip_cases as pcs
import pip_model as pm
from oracle.curves import CURVES

ORDERS = {name: c.r for name, c in CURVES.items()}


@pytest.mark.parametrize("curve", sorted(ORDERS))
def test_model_sums_are_the_plain_sums(curve):
    r = ORDERS[curve]
    for s in pcs.table(r) + pcs.seq_table(r):
        total, met = pm.window_sum(s.items, r)
        assert total == pm.plain_sum(s.items, r), s
        assert met <= pm.ALL_PAIRS, s
    rng = random.Random(3)
    for n in (0, 1, 63, 64, 65, 700, pm.TILE + 5):
        items = [(rng.randrange(r), rng.randrange(256)) for _ in range(n)]
        assert pm.window_sum(items, r)[0] == pm.plain_sum(items, r), n


@pytest.mark.parametrize("curve", sorted(ORDERS))
def test_the_table_meets_every_pair(curve):
    r = ORDERS[curve]
    met = set()
    by_name = {}
    for s in pcs.table(r) + pcs.seq_table(r):
        by_name[s.name] = pm.window_sum(s.items, r)[1]
        met |= by_name[s.name]
    missing = pm.ALL_PAIRS - met - set(pcs.UNREACHABLE)
    assert not missing, sorted(missing)
    # a pair declared unreachable is not met, is not "generic", and no site is declared unreachable as a whole
    assert not (set(pcs.UNREACHABLE) & met)
    assert all(b != "generic" and (s, b) in pm.ALL_PAIRS and why for (s, b), why in pcs.UNREACHABLE.items())
    for site in pm.SITES:
        assert any((site, b) not in pcs.UNREACHABLE for b in pm.BRANCHES if b != "generic")
        assert sum((site, b) in pcs.UNREACHABLE for b in pm.BRANCHES) < len(pm.BRANCHES) - 1, site


@pytest.mark.parametrize("curve", sorted(ORDERS))
def test_the_shapes_meet_what_they_are_built_for(curve):
    """The hand-built shapes, each against the pair it is named after."""
    r = ORDERS[curve]
    met = {s.name: pm.window_sum(s.items, r)[1] for s in pcs.table(r)}
    for off in pm.SCAN_OFFS:
        b = [b for b, o in [(64 * (i % 4) + 3, o) for i, o in enumerate(pm.SCAN_OFFS)] if o == off][0]
        assert ("scan:%d" % off, "equal") in met["same(%d, %d)" % (b, off)]
        assert ("scan:%d" % off, "equal") in met["same_repr(%d, %d)" % (b, off)]
        assert ("scan:%d" % off, "opposite") in met["opposite(%d, %d)" % (b, off)]
    for b, off in ((63, 1), (127, 1), (191, 1), (40, 32), (100, 128)):
        assert ("hop", "equal") in met["same(%d, %d)" % (b, off)] and ("hop", "opposite") in met["opposite(%d, %d)" % (b, off)]
    for i, off in enumerate(pm.TREE_OFFS):
        for kind in ("p identity", "opposite"):
            assert ("tree:%d" % off, kind) in met["tree_two(wave %d, %d, %s)" % (1 + i % 3, off, kind)], (off, kind)
    want = {"h = s": [("final:1", "equal")], "h = -63 s": [("final:1", "p identity"), ("final:2", "equal")],
            "h = -127 s": [("final:1", "opposite"), ("final:2", "p identity")],
            "h = -191 s": [("final:2", "opposite"), ("final:3", "p identity")],
            "h = 64 A - 191 s": [("final:3", "equal")], "h = -64 A - 191 s": [("final:3", "opposite")]}
    for name, pairs in want.items():
        assert all(p in met["final_three(%s)" % name] for p in pairs), (name, sorted(met["final_three(%s)" % name]))
    assert {("bucket", "equal")} <= met["bucket equal"] and {("bucket", "opposite")} <= met["bucket opposite"]
    assert ("bucket", "q identity") in met["identity points"]
