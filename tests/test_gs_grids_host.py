"""Gauss-Seidel power flow on the grids of tests/gs_grids.py, host side: what makes the device comparisons of tests/test_gs_grids_gpu.py meaningful.

The numpy restatement (tests/gs_reference.py) is run on every family, on its base lane and on every outage lane of gs_grids.labels; its statuses and
sweep counts are the literals below (as CASE14_COUNTS in tests/test_gs_gpu.py).  A lane either converges clear of the tolerance on both sides
(gs_reference.margins_hold, the +-1e-6 rule), so that a count can be compared exactly, or it is recorded as status 1 (the limit: an island without the
slack that stagnates) or 3 (a bus without admittance: a mismatch that is not finite).  A bridge outage never converges -- that is what it is listed
for -- so the kinds of outage that must converge somewhere are the twin, the branch at the slack, the out-of-service copy and the tapped / shifted one.

Voltage bound of the device tests, 1e-10: rounding of 1e-15 per sweep settles near 1e-15 / (1 - rho), rho the contraction of the lane (the ratio of its
last two mismatch maxima); the bound is justified where that is <= 1e-12, which is asserted for every converged lane of every family.

On the grids with an empty bus list, one sweep and one mismatch are also compared with a second statement that shares nothing with the first: a dense
complex Y built from the table, and a bus-by-bus loop in plain Python.
"""
import numpy as np
import pytest

import gs_grids as G
import gs_reference as R

TOL = G.TOL

# the sweep limit a family is run with, on the host and on the device
LIMIT = {"one bus": 10, "two buses, PQ": 20, "two buses, PV": 20, "star 33, hub slack": 20, "star 71, hub last": 1700, "star 40, hub first PV": 1200,
         "all PV ring 9": 700, "all PQ mesh 4x4": 200, "ring 12 with twins": 2100, "path 12": 2300, "two cliques 5+6": 1100, "pegaseShaped 60": 3500}

# family -> {outage label (0: the base grid): (status, sweeps)}, what the restatement gives
COUNTS = {
    "one bus": {0: (0, 0)},
    "two buses, PQ": {0: (0, 4), 1: (0, 4), 2: (0, 4), 3: (0, 4)},
    "two buses, PV": {0: (0, 9), 1: (0, 9), 2: (0, 9), 3: (0, 9)},
    "star 33, hub slack": {0: (0, 8), 7: (0, 8), 20: (0, 8), 33: (0, 8), 34: (0, 8), 1: (3, 1), 36: (0, 8), 12: (3, 1)},
    "star 71, hub last": {0: (0, 658), 6: (0, 1198), 13: (0, 653), 41: (0, 654), 71: (0, 1521), 74: (0, 658), 5: (1, 1700), 25: (3, 1)},
    "star 40, hub first PV": {0: (0, 379), 17: (0, 373), 39: (0, 621), 40: (0, 1044), 41: (0, 352), 43: (0, 379), 21: (3, 1)},
    "all PV ring 9": {0: (0, 163), 1: (0, 568), 3: (0, 193), 2: (0, 424), 4: (0, 145), 5: (0, 177)},
    "all PQ mesh 4x4": {0: (0, 114), 4: (0, 157), 12: (0, 112), 7: (0, 115), 1: (0, 114), 2: (0, 127), 3: (0, 127)},
    "ring 12 with twins": {0: (0, 557), 1: (0, 680), 7: (0, 518), 13: (0, 620), 14: (0, 528), 15: (0, 557), 6: (0, 830), 2: (0, 1914), 3: (0, 1661),
                           4: (0, 1307)},
    "path 12": {0: (0, 1296), 1: (0, 2068), 6: (0, 1235), 11: (0, 1205), 12: (0, 1404), 15: (0, 1296), 4: (1, 2300)},
    "two cliques 5+6": {0: (0, 899), 2: (0, 948), 8: (0, 941), 19: (0, 674), 26: (1, 1100), 1: (0, 902), 3: (0, 901), 4: (0, 924)},
    "pegaseShaped 60": {0: (0, 2433), 1: (0, 2433), 5: (0, 2359), 11: (0, 2424), 21: (0, 2417), 47: (0, 3263), 55: (3, 2), 3: (0, 2196), 6: (0, 2430),
                        7: (0, 2404)},
}

NAMES = list(G.FAMILIES)


def test_the_tables_cover_the_families():
    assert set(COUNTS) == set(LIMIT) == set(NAMES) and len(NAMES) == 12


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_on_every_family(name):
    """problem, lanes and run of the restatement on the grid; statuses and counts are the literals; the margins hold; at least three quarters of the
    lanes converge, the base lane among them; the contraction justifies the 1e-10 voltage bound"""
    t = G.family(name)
    lab = G.labels(t)
    assert tuple(COUNTS[name]) == lab, lab                        # the list the rule gives IS the recorded one, in its order
    g = R.problem(G.system(name))
    typ = t["bus_type"]
    assert g.pq.size == np.sum(typ == 1) and g.pv.size == np.sum(typ == 2) == g.vg.size and g.pad.shape == (g.n, g.deg.max())
    assert all(g.rowval[g.diag[i]] == i and g.colptr[i] <= g.diag[i] < g.colptr[i + 1] for i in range(g.n))
    out, v = G.restated(name, LIMIT[name])
    got = {int(l): (int(out.status[k]), int(out.iteration[k])) for k, l in enumerate(lab)}
    rho = G.contraction(out)
    print(name, got, "contraction", np.round(rho, 5).tolist())
    assert R.margins_hold(out, TOL)                               # FIRST: no count hangs on a rounding
    assert got == COUNTS[name]
    assert set(out.status) <= {0, 1, 3} and out.status[0] == 0
    assert np.mean(out.status == 0) >= 0.75
    ok = out.status == 0
    assert np.all(np.isfinite(v[ok])) and np.all(rho[ok] < 1.0)
    assert np.all(1e-15 / (1.0 - rho[ok]) <= 1e-12), rho


def test_the_families_reach_the_gaps_they_are_named_for():
    """bus lists, row shapes and outage kinds, read off the tables; every kind of outage that can converge does so in some family"""
    prob = {name: R.problem(G.system(name)) for name in NAMES}
    size = {name: (prob[name].n, prob[name].pq.size, prob[name].pv.size) for name in NAMES}
    assert size["one bus"] == (1, 0, 0) and prob["one bus"].yt.size == 1
    assert size["two buses, PQ"] == (2, 1, 0) and size["two buses, PV"] == (2, 0, 1)
    assert size["all PV ring 9"] == (9, 0, 8) and size["all PQ mesh 4x4"] == (16, 15, 0)
    slack = {name: int(np.flatnonzero(G.family(name)["bus_type"] == 3)[0]) for name in NAMES}
    g = prob["star 33, hub slack"]
    assert slack["star 33, hub slack"] == 0 and g.deg[0] == 33
    g = prob["star 71, hub last"]                                 # the hub: last bus, a demand bus, 71 entries, the diagonal last; the slack a leaf
    assert g.deg[70] == 71 and g.diag[70] == g.colptr[71] - 1 and 70 in g.pq and g.deg[slack["star 71, hub last"]] == 2
    g = prob["star 40, hub first PV"]                             # the hub: first bus, a generator bus, the diagonal first; the slack the last bus
    assert g.deg[0] == 40 and g.diag[0] == g.colptr[0] and 0 in g.pv and slack["star 40, hub first PV"] == 39
    assert prob["path 12"].deg[slack["path 12"]] == 2
    converged = set()
    for name in NAMES:
        t = G.family(name)
        kd, lab = G.kinds(t), G.labels(t)
        have = [kd[k] for k in lab[1:]]
        everywhere = {kind for s in kd.values() for kind in s}
        for kind in ("twin", "off", "bridge"):                    # one of each where the family has one
            assert kind not in everywhere or any(kind in s for s in have), (name, kind)
        if t["br_from"].size:
            assert any("slack" in s and "off" not in s for s in have), name
            assert any(("tap" in s or "shift" in s) and "off" not in s for s in have), name
        for k in lab[1:]:
            if COUNTS[name][k][0] == 0:
                converged |= {"tap or shift" if kind in ("tap", "shift") else kind for kind in kd[k]}
            if "bridge" in kd[k]:
                assert COUNTS[name][k][0] in (1, 3), (name, k)
    kd = G.kinds(G.family("ring 12 with twins"))                  # two parallel pairs, one of them at the slack, one copy out of service, shifters
    assert sum("twin" in s for s in kd.values()) == 4 and sum({"twin", "slack"} <= s for s in kd.values()) == 2
    assert sum("off" in s for s in kd.values()) == 1 and sum("shift" in s for s in kd.values()) >= 2
    assert converged >= {"twin", "slack", "off", "tap or shift"}, converged


@pytest.mark.parametrize("name", NAMES)
def test_the_patch_equals_a_rebuilt_system_on_every_family(name):
    """every label of the family, twins, slack branches and the out-of-service copy included: the 4 positions + deltas of transposedOutageTable applied
    to nodalMatrixTranspose.nzval give the values of a system rebuilt with updateBranch_(status = 0), to 1e-15; for the copy the delta is exactly 0"""
    from juliagrid.jl_amd.gaussseidel import transposedOutageTable
    t = G.family(name)
    lab = G.labels(t)[1:]
    if not lab:
        assert name == "one bus"
        return
    s = G.system(name)
    kd = G.kinds(t)
    ptr, dy = transposedOutageTable(s)
    base = np.array(s.model.ac.nodalMatrixTranspose.nzval)
    rebuilt = R.lane_values(s, lab)
    worst = 0.0
    for row, k in zip(rebuilt, lab):
        got = base.copy()
        np.add.at(got, ptr[k - 1] - 1, dy[k - 1])
        if "off" in kd[k]:
            assert np.all(dy[k - 1] == 0) and np.array_equal(row, base) and np.array_equal(got, base)
        else:
            assert not np.array_equal(row, base)
        if "twin" in kd[k]:                                       # the other branch of the pair stays: the off-diagonal entries are not cancelled
            assert np.all(got[ptr[k - 1, 2:] - 1] != 0)
        worst = max(worst, float(np.abs(got - row).max()))
    print(name, "worst |patched - rebuilt|", worst)
    assert worst <= 1e-15


def _dense(t, out=0):
    """dense Y of the table with branch `out` (a label, 0: none) left out -- the unified branch model written out once more, on its own"""
    n = t["bus_type"].size
    Y = np.zeros((n, n), dtype=np.complex128)
    for i in range(n):
        Y[i, i] = complex(t["bus_gs"][i], t["bus_bs"][i])
    for k in range(t["br_from"].size):
        if t["br_status"][k] != 1 or k + 1 == out:
            continue
        i, j = int(t["br_from"][k]) - 1, int(t["br_to"][k]) - 1
        y = 1.0 / complex(t["br_r"][k], t["br_x"][k])
        ratio = t["br_tap"][k] * np.exp(1j * t["br_shift"][k])
        Y[i, i] += (y + 0.5 * complex(t["br_g"][k], t["br_b"][k])) / abs(ratio) ** 2
        Y[j, j] += y + 0.5 * complex(t["br_g"][k], t["br_b"][k])
        Y[i, j] += -y / np.conj(ratio)
        Y[j, i] += -y / ratio
    return Y


def _plain_step(t, Y, v):
    """(stopP, stopQ) at v, then one sweep of v in place: buses one by one, scalars only"""
    n = t["bus_type"].size
    S = np.zeros(n, dtype=np.complex128)
    for k in range(t["gen_bus"].size):
        S[int(t["gen_bus"][k]) - 1] += complex(t["gen_pg"][k], t["gen_qg"][k])
    for i in range(n):
        S[i] -= complex(t["bus_pd"][i], t["bus_qd"][i])
    sp = sq = 0.0
    for i in range(n):
        if t["bus_type"][i] == 3:
            continue
        m = v[i] * np.conj(sum(Y[i, j] * v[j] for j in range(n))) - S[i]
        sp = max(sp, abs(m.real))
        if t["bus_type"][i] == 1:
            sq = max(sq, abs(m.imag))
    for i in range(n):
        if t["bus_type"][i] == 1:
            v[i] += (np.conj(S[i]) / np.conj(v[i]) - sum(Y[i, j] * v[j] for j in range(n))) / Y[i, i]
    first = {}
    for k in range(t["gen_bus"].size):
        first.setdefault(int(t["gen_bus"][k]) - 1, t["gen_vg"][k])
    for i in range(n):
        if t["bus_type"][i] == 2:
            cur = sum(Y[i, j] * v[j] for j in range(n))
            q = -(np.conj(v[i]) * cur).imag
            v[i] += (complex(S[i].real, -q) / np.conj(v[i]) - cur) / Y[i, i]
    for i in range(n):
        if t["bus_type"][i] == 2:
            v[i] = first[i] * v[i] / abs(v[i])
    return sp, sq


@pytest.mark.parametrize("name", ["one bus", "two buses, PQ", "two buses, PV"])
def test_an_empty_bus_list_against_a_second_statement(name):
    """three steps of the restatement against the dense bus-by-bus statement on every lane of the family.  1e-13: the two sum a row of at most two
    terms of size 10 in different orders and form the admittances differently, a few roundings of 1e-15 each per step"""
    t = G.family(name)
    lab = G.labels(t)
    s = G.system(name)
    g = R.problem(s)
    yt, v, P, Q = R.lanes(g, len(lab), R.lane_values(s, lab))
    n = g.n
    for k, out in enumerate(lab):
        Y = _dense(t, out)
        sparse = np.zeros((n, n), dtype=np.complex128)
        for i in range(n):
            sparse[i, g.rowval[g.colptr[i]:g.colptr[i + 1]]] = yt[k, g.colptr[i]:g.colptr[i + 1]]
        assert np.abs(sparse - Y).max() <= 1e-13 * max(1.0, np.abs(Y).max())
        w = np.array(g.v0)
        slack = int(np.flatnonzero(t["bus_type"] == 3)[0])
        assert abs(w[slack] - t["gen_vg"][0]) <= 1e-15            # the slack starts at its unit's set-point and never moves
        for step in range(3):
            rp, rq = R.mismatch(g, yt[k:k + 1], v[k:k + 1], P[k:k + 1], Q[k:k + 1])
            sp, sq = _plain_step(t, Y, w)
            R.sweep(g, yt[k:k + 1], v[k:k + 1], P[k:k + 1], Q[k:k + 1])
            assert abs(rp[0] - sp) <= 1e-13 and abs(rq[0] - sq) <= 1e-13, (out, step)
            assert np.abs(v[k] - w).max() <= 1e-13, (out, step)
            assert v[k, slack] == g.v0[slack]
        if name != "one bus":
            assert np.abs(v[k] - g.v0).max() > 1e-4               # the steps did move the other bus
