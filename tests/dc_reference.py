"""numpy / scipy restatement of the reference's DC power flow (behaviour only), the check of tests/test_dc_host.py and tests/test_dc_gpu.py.

  model(t)            dcModel!: admittances, shiftPower, the nodal matrix in the reference's CSC order (diagonal entry first in a column, then the
                      branch stamps in branch order, stably sorted by row, duplicates summed in that order; out-of-service branches as stored zeros)
  solve(t, out=k)     solve!: slack row and column removed, slack diagonal 1, theta = B^-1 rhs, + the slack's angle.  An outage REBUILDS the matrix
                      with the branch's status 0 and refactorises (scipy splu) -- never the compensation formula the library uses
  power(t, theta, out=k)   power!: injection, supply, generator, from (to = -from)

`t` is a table dict of tests/conftest.py: load_case.  It is pinned to the reference's own vectors by tests/test_dc_host.py.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla


def slack_of(t):
    s = np.flatnonzero(t["bus_type"] == 3)
    rule = t.get("slack_rule")
    last = rule is not None and str(np.asarray(rule).reshape(-1)[0]) == "last"
    return int(s[-1 if last else 0]) if s.size else 0


def admittance(t, out=None):
    st = np.asarray(t["br_status"]).astype(np.int64).copy()
    if out is not None:
        st[out] = 0
    y = np.zeros(st.size)
    on = st == 1
    y[on] = 1.0 / (np.asarray(t["br_tap"], dtype=np.float64)[on] * np.asarray(t["br_x"], dtype=np.float64)[on])
    return y


def model(t, out=None):
    """(colptr, rowval, nzval) 1-based CSC, admittance, shiftPower -- a plain loop in the reference's insertion order"""
    n = t["bus_type"].size
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    shift = np.asarray(t["br_shift"], dtype=np.float64)
    y = admittance(t, out)
    on = np.asarray(t["br_status"]).astype(np.int64) == 1
    if out is not None:
        on[out] = False
    psh = np.zeros(n)
    cols = [[[i, 0.0]] for i in range(n)]                       # column -> [row, value] in insertion order; the diagonal first
    for k in range(f.size):
        if on[k]:
            psh[f[k]] -= shift[k] * y[k]
            psh[to[k]] += shift[k] * y[k]
            cols[f[k]][0][1] += y[k]
            cols[to[k]][0][1] += y[k]
        cols[to[k]].append([f[k], -y[k]])
        cols[f[k]].append([to[k], -y[k]])
    colptr, rowval, nzval = [1], [], []
    for j in range(n):
        ent = sorted(range(len(cols[j])), key=lambda q: (cols[j][q][0], q))
        last = None
        for q in ent:
            r, v = cols[j][q]
            if r == last:
                nzval[-1] += v
            else:
                rowval.append(r + 1)
                nzval.append(v)
                last = r
        colptr.append(len(rowval) + 1)
    return (np.array(colptr, dtype=np.int64), np.array(rowval, dtype=np.int64), np.array(nzval)), y, psh


def assemble(t, out=None):
    """the same matrix for the solves, assembled by scipy (duplicates summed in scipy's order): B (csc), admittance, shiftPower"""
    n = t["bus_type"].size
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    y = admittance(t, out)
    sh = np.asarray(t["br_shift"], dtype=np.float64) * y
    psh = np.zeros(n)
    np.add.at(psh, f, -sh)
    np.add.at(psh, to, sh)
    B = sp.coo_matrix((np.r_[y, y, -y, -y], (np.r_[f, to, f, to], np.r_[f, to, to, f])), shape=(n, n)).tocsc()
    return B, y, psh


def supply(t):
    s = np.zeros(t["bus_type"].size)
    on = np.asarray(t["gen_status"]) == 1
    np.add.at(s, np.asarray(t["gen_bus"]).astype(np.int64)[on] - 1, np.asarray(t["gen_pg"], dtype=np.float64)[on])
    return s


def rhs_of(t, psh, injection=None):
    net = supply(t) - t["bus_pd"] if injection is None else np.asarray(injection, dtype=np.float64)
    return net - t["bus_gs"] - psh


def solve(t, out=None, injection=None):
    """theta [n], from [branches] with branch `out` (0-based, or None) out of service; (None, None) if the rebuilt matrix is singular"""
    B, y, psh = assemble(t, out)
    n = t["bus_type"].size
    slack = slack_of(t)
    keep = np.r_[0:slack, slack + 1:n]
    rhs = rhs_of(t, psh, injection)
    th = np.zeros(n)
    try:
        lu = sla.splu(B[keep][:, keep].tocsc())
    except RuntimeError:
        return None, None
    th[keep] = lu.solve(rhs[keep])
    th += np.asarray(t["bus_va"], dtype=np.float64)[slack]
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    return th, y * (th[f] - th[to] - np.asarray(t["br_shift"], dtype=np.float64))


def power(t, th, out=None, injection=None):
    """dict(injection, supply, generator, from_) of power!(analysis)"""
    B, y, psh = assemble(t, out)
    n = t["bus_type"].size
    B = B.tocsr()
    slack = slack_of(t)
    sup = supply(t)
    inj = (sup - t["bus_pd"]) if injection is None else np.asarray(injection, dtype=np.float64).copy()
    inj[slack] = B[slack].dot(th)[0] + t["bus_gs"][slack] + psh[slack]
    sup = sup.copy()
    sup[slack] = t["bus_pd"][slack] + inj[slack]
    gen_bus = np.asarray(t["gen_bus"]).astype(np.int64) - 1
    on = np.asarray(t["gen_status"]) == 1
    pg = np.asarray(t["gen_pg"], dtype=np.float64)
    g = np.where(on, pg, 0.0)
    at_slack = [k for k in range(gen_bus.size) if on[k] and gen_bus[k] == slack]
    if at_slack:
        g[at_slack[0]] = inj[slack] + t["bus_pd"][slack] - sum(pg[k] for k in at_slack[1:])
    f = np.asarray(t["br_from"]).astype(np.int64) - 1
    to = np.asarray(t["br_to"]).astype(np.int64) - 1
    return dict(injection=inj, supply=sup, generator=g, from_=y * (th[f] - th[to] - np.asarray(t["br_shift"], dtype=np.float64)))


def isapprox(a, b):
    """the reference's own test criterion: isapprox with the default rtol = sqrt(eps)"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return np.linalg.norm(a - b) <= 1.5e-8 * max(np.linalg.norm(a), np.linalg.norm(b))


def worst(a, ref):
    """max |a - ref| / max(1, max |ref|): held against 1e-9, the tolerance the project holds its linear step to"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))
