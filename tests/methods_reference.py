"""What tests/test_oracle_methods.py (CPU) and tests/test_methods_grids_gpu.py (GPU) share for the Orthogonal / PetersWilkinson tags on the 118- and
300-bus grids: the grids with their power-flow state, the measurement tables, the seeded rule that gives every lane of a batch readings of its own, and
the dense oracle's answer per lane -- each computed once per session and left unchanged.

DEV_REF is the yardstick of the GPU file: max|orth - pw| / max|orth| of the oracle's two dense increments at the start point, as
test_oracle_methods.test_dense_increments_agree_on_the_grids measured and printed it on the CPU (numpy / LAPACK QR against scipy's LU + the normal
equations in L).  A device increment may sit 10 x DEV_REF from the dense QR: another summation order on top of the gap between the two reference solvers."""
import numpy as np

DEV_REF = {"case118": 2.5e-15, "case300": 4.2e-15}
MIN_CURRENT = 1e-6                 # ammeters and branch PMUs on (numerically) dead branches are left out, as addAmmeter_(mon, pf, minMagnitude=1e-6) does
NOISE_STEP = 0.25                  # lane b reads z + NOISE_STEP * (b % 5) * sigma * N(0, 1)
SPREAD_STEP = 100.0                # ... and with this step the lanes stop at different iterations
SPREAD_SEED = 6                    # the seed under which test_oracle_methods.test_spread_lanes_stop_clear_of_the_tolerance holds (3 and 6 of 1 ... 12 do)
# batch of 65, by name: ((lane, lane whose readings it repeats) ..., lanes compared with an oracle run of their own)
SPREAD = {"second_group_first": (((64, 0),), (0, 2, 3, 4, 63, 64)),                 # lanes 0 ... 63 by the rule, lane 64 reads exactly
          "first_group_first": (tuple((b, 0) for b in range(1, 64)), (0, 63, 64))}  # lanes 0 ... 63 read exactly, lane 64 by the rule
LANE_SEED = 2118

_GRIDS, _LANES = {}, {}


def increment_bound(case):
    """relative to max|ref|: 10 x DEV_REF, never looser than 1e-6"""
    return min(10.0 * DEV_REF[case], 1e-6)


def state_bound(case):
    """absolute, on V (pu) and theta (rad): 10 x DEV_REF, floored at 1e-9 (the runs stop at a step of 1e-8)"""
    return max(10.0 * DEV_REF[case], 1e-9)


def grid(oracle, name):
    """(case tables, OracleSystem with the power flow's bus types and slack, vm, va) of a solved power flow; shared, read-only"""
    if name not in _GRIDS:
        from conftest import load_case
        t = load_case(name)
        s = oracle.OracleSystem(t)
        pf = oracle.OracleNR(s)
        assert pf.power_flow() == 0
        vm, va = pf.voltage()
        s.type = pf.type.copy(); s.slack = pf.slack
        _GRIDS[name] = (t, s, vm, va)
    return _GRIDS[name]


def all_families(oracle, s, vm, va, min_current=MIN_CURRENT):
    """voltmeters, ammeters, wattmeters, varmeters and PMUs from the power flow; current magnitudes below min_current keep no ammeter and no branch PMU
    (MeterTable has no such filter of its own)"""
    tab = oracle.MeterTable()
    for fam in ("voltmeter", "ammeter", "wattmeter", "varmeter", "pmu"):
        oracle.add_from_power_flow(tab, s, vm, va, fam)
    tab.rows = [r for r in tab.rows if not ((r[0] == 2 or (r[0] == 5 and r[1] != 0)) and r[3] < min_current)]
    return tab


def device_rows(tab):
    """the table's devices in the order both sides number them: by family, insertion order inside"""
    return sorted(tab.rows, key=lambda r: r[0])


def contributions_per_bus(colptr, rowval, n):
    """how many measurement rows touch each bus, from the CSC pattern of H (1-based): the length of the bus row's right-hand-side contribution list"""
    colptr, rowval = np.asarray(colptr) - 1, np.asarray(rowval) - 1
    return np.array([np.union1d(rowval[colptr[i]:colptr[i + 1]], rowval[colptr[i + n]:colptr[i + n + 1]]).size for i in range(n)])


def lane_readings(tab, lanes, seed=LANE_SEED, repeats=(), step=NOISE_STEP):
    """(n1, n2) [len(lanes), devices]: the first and second reading of every device for the given lane numbers.  Lane b draws from its own generator
    (seed, b) and reads z + step * (b % 5) * sigma * N(0, 1): the same in every batch, exactly where b % 5 == 0.  repeats: (lane, lane it copies) pairs."""
    rows = device_rows(tab)
    z1, v1 = np.array([r[3] for r in rows]), np.array([r[4] for r in rows])
    z2, v2 = np.array([r[6] for r in rows]), np.array([r[7] for r in rows])
    pmu = np.array([r[0] == 5 for r in rows])
    src = dict(repeats)
    n1, n2 = np.empty((len(lanes), z1.size)), np.empty((len(lanes), z1.size))
    for q, b in enumerate(lanes):
        b = src.get(b, b)
        rng = np.random.default_rng([seed, b])
        scale = step * (b % 5)
        n1[q] = z1 + scale * np.sqrt(v1) * rng.standard_normal(z1.size)
        n2[q] = z2 + np.where(pmu, scale * np.sqrt(v2) * rng.standard_normal(z1.size), 0.0)
    return n1, n2


def lane_table(oracle, tab, n1, n2):
    """a fresh MeterTable that holds one lane's readings"""
    tb = oracle.MeterTable()
    tb.rows = [r[:3] + (float(n1[d]),) + r[4:6] + (float(n2[d]),) + r[7:] for d, r in enumerate(device_rows(tab))]
    return tb


def upload_lanes(an, n1, n2):
    """hand every lane its readings: the value rules of the analysis on [batch, devices] readings, then one upload"""
    z1, v1, s1, z2, v2, s2 = an._z
    if an.batch == 1:
        n1, n2 = n1[0], n2[0]
    mean, wd, wo, _ = an._values(an.monitoring, an._devs, an._dev_row, an.dims["m"], n1, v1, s1, n2, v2, s2)
    an._upload_measurement(mean, wd, wo)


class LaneAnswer:
    """the dense oracle on one lane's own table: the first Orthogonal increment, then stateEstimation! around it"""

    def __init__(self, oracle, s, tab):
        gn = oracle.OracleGN(s, tab)
        self.first = gn.increment_orthogonal()
        self.ok, self.iteration = gn.state_estimation_with(gn.increment_orthogonal)
        v = gn.vectors()
        self.magnitude, self.angle = v["magnitude"], v["angle"]
        self.checks = list(gn.checks)


def lane_answer(oracle, case, b, seed=LANE_SEED, step=NOISE_STEP):
    """LaneAnswer of lane b of the all-families table of `case` under lane_readings(seed, step); computed once"""
    key = (case, b, seed, step)
    if key not in _LANES:
        t, s, vm, va = grid(oracle, case)
        tab = all_families(oracle, s, vm, va)
        n1, n2 = lane_readings(tab, [b], seed, step=step)
        _LANES[key] = LaneAnswer(oracle, s, lane_table(oracle, tab, n1[0], n2[0]))
    return _LANES[key]


def margins_hold(answer, tolerance=1e-8, factor=2.0):
    """the lane stopped clear of the tolerance on both sides: its last check at least `factor` below it, the check before at least `factor` above"""
    c = answer.checks
    return bool(answer.ok and len(c) >= 2 and c[-1] * factor <= tolerance and c[-2] >= tolerance * factor)


# ---- rows out of service, and one gross error -------------------------------------------------------------------------------------------------
GN_ROWS = 16                       # measurement rows per workgroup of the row kernels (csrc/jg_gn.hip)


def masked_table(oracle, s, vm, va):
    """about every seventh meter out of service (PMUs by their magnitude or their angle channel in turn); the devices that own the measurement rows
    GN_ROWS - 1, GN_ROWS and m - 1 stay in service and their neighbours go out"""
    tab = all_families(oracle, s, vm, va)
    rows = device_rows(tab)
    nd = len(rows)
    assert all(r[0] == 1 for r in rows[:GN_ROWS + 2]) and rows[-1][0] == 5 and rows[-2][0] == 5     # rows 14 ... 17 are voltmeters, the last two devices PMUs
    out1 = {d for d in range(nd) if d % 7 == 3 and (rows[d][0] != 5 or d % 14 == 3)}
    out2 = {d for d in range(nd) if d % 7 == 3 and rows[d][0] == 5 and d % 14 == 10}
    out1 -= {GN_ROWS - 1, GN_ROWS, nd - 1}; out2 -= {nd - 1}
    out1 |= {GN_ROWS - 2, GN_ROWS + 1, nd - 2}
    tab.rows = [r[:5] + (0 if d in out1 else 1,) + r[6:8] + (0 if d in out2 else 1,) + r[9:] for d, r in enumerate(rows)]
    return tab


BAD_WATTMETER, BAD_ERROR = 200, 5.0          # the planted gross error: wattmeter number (from 1) and what is added to its reading (pu; sigma = 0.01)


def bad_table(oracle, s, vm, va):
    """(table with the planted error, 0-based measurement row of that wattmeter)"""
    tab = all_families(oracle, s, vm, va)
    rows = device_rows(tab)
    d = [i for i, r in enumerate(rows) if r[0] == 3][BAD_WATTMETER - 1]
    rows[d] = rows[d][:3] + (rows[d][3] + BAD_ERROR,) + rows[d][4:]
    tab.rows = rows
    return tab, d                                                  # every device before the wattmeters owns one row: device number = row


def without_row(tab, d):
    tb = type(tab)()
    tb.rows = [r[:5] + (0,) + r[6:] if i == d else r for i, r in enumerate(device_rows(tab))]
    return tb


def reestimate_deviation(oracle, case="case118"):
    """max |estimate - power flow| the oracle's own Orthogonal run leaves on bad_table with the flagged row out of service"""
    key = (case, "reestimate")
    if key not in _LANES:
        t, s, vm, va = grid(oracle, case)
        tab, d = bad_table(oracle, s, vm, va)
        gn = oracle.OracleGN(s, without_row(tab, d))
        ok, _ = gn.state_estimation_with(gn.increment_orthogonal)
        assert ok
        v = gn.vectors()
        _LANES[key] = max(np.abs(v["magnitude"] - vm).max(), np.abs(v["angle"] - va).max())
    return _LANES[key]
