"""numpy restatement of the batched PMU least-absolute-value estimator (csrc/jg_pmulav.hip on the iteration of csrc/jg_dclav.hip), dense, f64, one lane,
and the same LP through scipy's HiGHS.

The model is the reference's pmuLavStateEstimation (src/stateEstimation/pmuStateEstimation.jl:223-338), unweighted, with NO fixed state:

    minimise  sum_i (u_i + v_i)   subject to   h_i x + u_i - v_i = z_i,  u, v >= 0        (= min |z - H x|_1),   x = (re V, im V)

  two_port(t)                 the pi-model's yff, yft, ytf, ytt, y and the tap of every branch of a case table (zero where out of service)
  pmu_table(t, vm, va)        a bus PMU at every bus and a PMU at both ends of every in-service branch, exact polar readings of the state (vm, va)
  pmulav_rows(t, pmus)        H (dense [2 pmus, 2 buses]), z (rectangular) and the row status: two rows per PMU, out only with BOTH channels in service
  pmulav_ipm(H, z, on, ...)   the iteration of tests/dclav_reference.py: its fixed state is given a column of zeros appended to H, so G carries a 1
                              there and nothing of the 2 n real states is fixed -- the statements, their order and the stopping tests are that file's
  pmulav_linprog(H, z, on)    scipy.optimize.linprog(method="highs") on the primal LP, every state free
  flows(t, V)                 branch currents and powers, series and charging quantities and bus injections from complex voltages
  rho(r)                      the phasor residual per device
"""
from types import SimpleNamespace as NS

import numpy as np

import dclav_reference as L


def two_port(t):
    f8 = lambda k: np.asarray(t[k], dtype=np.float64)
    on = np.asarray(t["br_status"]).astype(int) == 1
    y = 1.0 / (f8("br_r") + 1j * f8("br_x"))
    tap = f8("br_tap")
    tr = np.exp(-1j * f8("br_shift")) / tap                          # 1 / (tau e^{j phi})
    ytt = y + 0.5 * (f8("br_g") + 1j * f8("br_b"))
    yff = ytt / tap ** 2
    yft, ytf = -np.conj(tr) * y, -tr * y
    z = lambda a: np.where(on, a, 0.0)
    return NS(y=z(y), yff=z(yff), yft=z(yft), ytf=z(ytf), ytt=z(ytt), tij=tr, on=on, f=np.asarray(t["br_from"]).astype(int) - 1,
              t=np.asarray(t["br_to"]).astype(int) - 1, charging=f8("br_g") + 1j * f8("br_b"), tinv=1.0 / tap)


def pmu_table(t, vm, va):
    """kind (0 bus, 1 from, 2 to), index (1-based bus or branch), magnitude, angle, the two channel statuses: all buses, then per in-service branch its
    from end and its to end (the order of addPmu!)"""
    p = two_port(t)
    V = np.asarray(vm) * np.exp(1j * np.asarray(va))
    kind, index, ph = [], [], []
    for b in range(V.size):
        kind.append(0); index.append(b + 1); ph.append(V[b])
    for k in np.flatnonzero(p.on):
        kind += [1, 2]; index += [k + 1, k + 1]
        ph += [V[p.f[k]] * p.yff[k] + V[p.t[k]] * p.yft[k], V[p.f[k]] * p.ytf[k] + V[p.t[k]] * p.ytt[k]]
    ph = np.array(ph)
    return NS(kind=np.array(kind), index=np.array(index), magnitude=np.abs(ph), angle=np.angle(ph), status_magnitude=np.ones(len(kind), dtype=int),
              status_angle=np.ones(len(kind), dtype=int))


def pmulav_rows(t, pmus, magnitude=None, angle=None):
    """-> H [2 pmus, 2 buses], z [2 pmus] (readings: the table's or the given polar ones), on [2 pmus]"""
    p = two_port(t)
    n = np.asarray(t["bus_type"]).size
    m = pmus.kind.size
    H = np.zeros((2 * m, 2 * n))
    for i in range(m):
        k = int(pmus.index[i]) - 1
        if pmus.kind[i] == 0:
            H[2 * i, k] = H[2 * i + 1, n + k] = 1.0
            continue
        ya, yb = (p.yff[k], p.yft[k]) if pmus.kind[i] == 1 else (p.ytf[k], p.ytt[k])
        for bus, yy in ((p.f[k], ya), (p.t[k], yb)):
            H[2 * i, bus] += yy.real; H[2 * i, n + bus] += -yy.imag
            H[2 * i + 1, bus] += yy.imag; H[2 * i + 1, n + bus] += yy.real
    mag = pmus.magnitude if magnitude is None else np.asarray(magnitude, dtype=np.float64)
    ang = pmus.angle if angle is None else np.asarray(angle, dtype=np.float64)
    z = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1).reshape(mag.shape[:-1] + (2 * m,))
    on = np.repeat((pmus.status_magnitude * pmus.status_angle) == 1, 2)
    return H, z, on


def pmulav_ipm(H, z, on=None, iteration=50, tolerance=1e-8, x0=None):
    """dclav_reference.lav_ipm with nothing fixed: theta -> x [2 buses]"""
    m, n = H.shape
    Ha = np.hstack([H, np.zeros((m, 1))])
    a = L.lav_ipm(Ha, z, on, slack=n, iteration=iteration, tolerance=tolerance, theta0=None if x0 is None else np.r_[x0, 0.0])
    a.x = a.theta[:n]
    return a


def polar(x):
    n = x.size // 2
    return np.hypot(x[:n], x[n:]), np.arctan2(x[n:], x[:n])


def pmulav_linprog(H, z, on=None):
    """-> NS(x, objective): variables (x, u, v) of the in-service rows, every state free"""
    from scipy.optimize import linprog
    m, n = H.shape
    on = np.ones(m, dtype=bool) if on is None else np.asarray(on, dtype=bool)
    Hs, zs = H[on], z[on]
    k = Hs.shape[0]
    A = np.hstack([Hs, np.eye(k), -np.eye(k)])
    out = linprog(np.r_[np.zeros(n), np.ones(2 * k)], A_eq=A, b_eq=zs, bounds=[(None, None)] * n + [(0.0, None)] * (2 * k), method="highs")
    assert out.status == 0, out.message
    return NS(x=out.x[:n], objective=float(out.fun))


def flows(t, V, status=None):
    """V complex [..., buses] -> currents and powers per branch and the injected power per bus; `status` overrides the table's branch status"""
    tt = dict(t)
    if status is not None:
        tt["br_status"] = np.asarray(status)
    p = two_port(tt)
    Vf, Vt = V[..., p.f], V[..., p.t]
    Iij, Iji = Vf * p.yff + Vt * p.yft, Vf * p.ytf + Vt * p.ytt
    Vs = p.tij * Vf - Vt
    Is = p.y * Vs
    Sij, Sji = Vf * np.conj(Iij), Vt * np.conj(Iji)
    ch = np.where(p.on, 0.5 * np.conj(p.charging) * (np.abs(p.tinv * Vf) ** 2 + np.abs(Vt) ** 2), 0.0)
    inj = np.zeros(V.shape, dtype=np.complex128)
    for k in range(p.f.size):
        inj[..., p.f[k]] += Sij[..., k]
        inj[..., p.t[k]] += Sji[..., k]
    inj += np.abs(V) ** 2 * np.conj(np.asarray(t["bus_gs"], dtype=np.float64) + 1j * np.asarray(t["bus_bs"], dtype=np.float64))
    return NS(fromCurrent=Iij, toCurrent=Iji, seriesCurrent=Is, from_=Sij, to=Sji, series=Vs * np.conj(Is), charging=ch, injection=inj, on=p.on)


def rho(r, on):
    """r [..., 2 pmus] -> the phasor residual per device, 0 outside the model"""
    return np.hypot(r[..., 0::2], r[..., 1::2]) * on[0::2]
