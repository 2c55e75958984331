"""The table that says who leaves with a bridge (jg.islandTable: ONE DFS from the slack, the side of a bridge without the slack as an interval of preorder
numbers) against the restatement, which deletes the branch and SEARCHES for the slack's component (tests/dc_island_reference.py).  Host code only."""
import numpy as np
import pytest

import dc_island_reference as I
from conftest import load_case


def check_table(jg, t):
    s = jg.powerSystem(t)
    tb = jg.islandTable(s)
    n, nb = s.bus.number, s.branch.number
    assert tb.preorder.shape == (n,) and tb.lo.shape == tb.hi.shape == tb.side.shape == tb.m.shape == (nb,)
    assert np.array_equal(np.sort(tb.preorder), np.arange(n))           # connected grids: a numbering of every bus
    assert tb.preorder[s.bus.layout.slack - 1] == 0
    is_bridge = jg.bridges(s)                                            # the low-link walk the project already had, rooted elsewhere
    assert np.array_equal(tb.lo <= tb.hi, is_bridge) and np.array_equal(tb.side != 0, is_bridge)
    f, to = s.branch.layout.from_, s.branch.layout.to
    for k in np.flatnonzero(is_bridge):
        gone = ~I.component(t, out=int(k))
        inside = (tb.preorder >= tb.lo[k]) & (tb.preorder <= tb.hi[k])
        assert np.array_equal(inside, gone), k
        assert np.array_equal(np.sort(tb.order[tb.lo[k]:tb.hi[k] + 1]), np.flatnonzero(gone)), k
        m, other = (f[k], to[k]) if tb.side[k] > 0 else (to[k], f[k])
        assert tb.m[k] == m and not gone[m - 1] and gone[other - 1], k
    return tb, is_bridge


@pytest.mark.parametrize("case,bridges", [("case14", 1), ("case118", 9), ("case_ACTIVSg10k", 12706 - 8729)])
def test_every_bridge_interval_is_the_complement_of_the_slacks_component(jg, case, bridges):
    t = load_case(case)
    _, is_bridge = check_table(jg, t)
    assert int(is_bridge.sum()) == bridges


def test_hand_built_grid_doubled_branch_open_loop_and_a_bridge_at_the_slack(jg):
    t, marks, perm = I.hand_grid()
    tb, is_bridge = check_table(jg, t)
    assert not is_bridge[marks["doubled"]].any()                         # two parallel branches: neither islands anything
    assert is_bridge[marks["behind_doubled"][0]]                         # ... because the branch that would close the loop is out of service
    assert not is_bridge[marks["open_loop"][0]] and tb.side[marks["open_loop"][0]] == 0
    t2 = {k: np.array(v) for k, v in t.items()}
    t2["br_status"][marks["open_loop"][0]] = 1
    assert not jg.islandTable(jg.powerSystem(t2)).side[marks["behind_doubled"][0]]
    k = marks["at_slack"][0]
    slack = int(np.flatnonzero(t["bus_type"] == 3)[0]) + 1
    assert is_bridge[k] and tb.m[k] == slack and tb.hi[k] == tb.lo[k]
    k = marks["pocket"][0]
    assert tb.side[k] == -1 and tb.hi[k] - tb.lo[k] + 1 == 85            # the to-end stays; 85 buses leave
    assert [int(tb.hi[k] - tb.lo[k] + 1) for k in marks["chain"]] == [2, 1]
    assert [int(tb.hi[k] - tb.lo[k] + 1) for k in marks["far"]] == list(range(10, 0, -1))
    assert np.all(tb.side[marks["chain"]] == 1) and np.all(tb.side[marks["far"]] == 1)


def test_outage_list_can_keep_the_bridges(jg):
    s = jg.powerSystem(load_case("case118"))
    assert not jg.bridges(s)[jg.outageList(s, 186) - 1].any()
    kept = jg.outageList(s, 186, keepBridges=True)
    assert np.unique(kept).size == 186 and jg.bridges(s)[kept - 1].sum() == 9


def test_an_unknown_islands_value_is_refused_before_the_device_is_touched(jg, monkeypatch):
    s = jg.powerSystem(load_case("case14"))
    def boom(*a, **k):
        raise AssertionError("a device handle was asked for")
    monkeypatch.setattr(jg.dcpowerflow, "dcPowerFlow", boom)
    with pytest.raises(ValueError):
        jg.contingencyAnalysis(s, [1, 2], method="dc", islands="drop")
    with pytest.raises(ValueError):
        jg.dcpowerflow.dcContingencyAnalysis(s, [1, 2], islands="SHED")
    with pytest.raises(ValueError):
        jg.contingencyAnalysis(s, [1, 2], method="nr", islands="shed")     # the AC screens have no such mode
