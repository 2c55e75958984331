"""The records of a screen call's row block at the edges of the ONE extraction the pair, series and transfer screens share (csrc/jg_dc_records.hpp:
k_dc_rows, dc_block_records), which the screens' own tests reach only by accident: blocks of 1, 5 and 7 rows (idle waves in the last workgroup),
capacity 0, a capacity that ends in the middle of a row's hits and one that ends at a row boundary, a threshold / amount under which every cell hits
and one under which none does, the pair's empty last row k = nk - 1 and its rows with (k + 1) % 64 == 0, its two lists overflowing independently, and the
all-NaN row of a bridge candidate among the rows of a workgroup (series, transfer).

Every call is judged against the dense arrays THE SAME CALL returns (they come from the screen kernels, not from the extraction): the expected list is
the hits of the dense result in (row, column) order, the totals are their number whatever the capacity, the delivered list is its first min(total,
capacity) entries, nothing is written behind them (the buffers are filled with a sentinel first), and the per-row reduction is the maximum / minimum of
the row, NaN aside.  Equality is exact: == on integers and on the bits of doubles.  The one thing the dense result does not hold is column 4 of a
transfer record, the sensitivity g of the limiting branch: it is held against the uncut whole-range list of the same build, bit for bit.

The calls go through the library's C entry points, on one dcPowerFlow handle per grid and one build per (screen, T)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
import dc_transfer_reference as X
from conftest import load_case

pytestmark = pytest.mark.gpu

SENT = -7.0                                                            # no record, label, loading or capability of these grids is -7
ROOM = 5                                                               # entries of a record buffer behind the capacity: they must stay untouched


@pytest.fixture(scope="module", params=["case30test", "case118"])
def g(jg, request):
    t = load_case(request.param)
    s = jg.powerSystem(t)
    an = jg.dcPowerFlow(s)
    L, check = jg._lib.lib(), jg._lib.check
    keep = NS(rhs=np.ascontiguousarray(jg.dcpowerflow._base_rhs(s), dtype=np.float64), rating=np.ascontiguousarray(P.rating_of(t), dtype=np.float64))
    vp = lambda a: None if a is None else a.ctypes.data_as(jg._lib.VP)
    check(L.jg_dc_set_rhs(an._h, keep.rhs))
    check(L.jg_dc_set_rating(an._h, vp(keep.rating)))
    every = jg.shedCandidates(s)
    yield NS(case=request.param, t=t, s=s, L=L, check=check, vp=vp, h=an._h, keep=keep, pair=jg.pairCandidates(s), every=every,
             bridges=np.flatnonzero(np.isin(every, np.flatnonzero(jg.bridges(s)) + 1)))
    an.close()


def bits(a):
    """the 8-byte words of a float64 or int64 array"""
    return np.ascontiguousarray(a).view(np.int64)


def listed(hit, entry):
    """the entries [rows, columns, w] of the cells `hit` marks, rows first, columns ascending"""
    return entry[hit]                                                  # (boolean indexing walks in C order)


def held_list(got, want, total, kept, cap, columns=slice(None)):
    """`got` is the call's buffer [cap + ROOM, w] (sentinel-filled before the call)"""
    assert total == want.shape[0] and kept == min(total, cap)
    assert got.dtype == want.dtype and np.array_equal(bits(got[:kept, columns]), bits(want[:kept, columns]))
    assert (got[kept:] == SENT).all()


def capacities(hit):
    """0, one that ends in the middle of a row's hits, one that ends at a row boundary behind a row with hits (both inside the list), the exact
    number, and one more"""
    count = hit.sum(axis=1)
    off = np.concatenate([[0], np.cumsum(count)])
    total = int(off[-1])
    caps = {0, total, total + 1}
    mid = [int(off[i] + count[i] // 2) for i in range(count.size) if count[i] >= 2]
    edge = [int(off[i + 1]) for i in range(count.size - 1) if count[i] >= 1 and off[i + 1] < total]
    return sorted(caps | set(mid[:1]) | set(mid[-1:]) | set(edge[:1]) | set(edge[-1:])), bool(mid), bool(edge)


# ---- the pair screen --------------------------------------------------------------------------------------------------------------------------------
def pair_call(g, cand, k0, k1, thr, cap, icap):
    nk, rb = int(cand.size), k1 - k0
    rec, isl, tot, worst = np.full((cap + ROOM, 5), SENT), np.full((icap + ROOM, 2), int(SENT), dtype=np.int64), np.zeros(6, dtype=np.int64), np.zeros(nk)
    d = NS(loading=np.zeros((rb, nk)), branch=np.zeros((rb, nk), dtype=np.int32), count=np.zeros((rb, nk), dtype=np.int32))
    g.check(g.L.jg_dc_pair_screen(g.h, k0, k1, thr, cap, g.vp(rec), icap, g.vp(isl), tot, g.vp(worst), g.vp(d.loading), g.vp(d.branch), g.vp(d.count), None))
    return d, rec, isl, tot, worst


def pair_held(g, cand, k0, k1, thr, cap, icap):
    nk, rb = int(cand.size), k1 - k0
    d, rec, isl, tot, worst = pair_call(g, cand, k0, k1, thr, cap, icap)
    upper = np.arange(nk)[None, :] > np.arange(k0, k1)[:, None]
    assert (d.loading[~upper] == 0).all()
    with np.errstate(invalid="ignore"):
        viol, island = upper & (d.loading > thr), upper & np.isnan(d.loading)
    lab_k, lab_l = np.broadcast_to(cand[k0:k1, None], (rb, nk)), np.broadcast_to(cand[None, :], (rb, nk))
    want = listed(viol, np.stack([lab_k.astype(np.float64), lab_l.astype(np.float64), d.branch.astype(np.float64), d.loading, d.count.astype(np.float64)], axis=2))
    want_isl = listed(island, np.stack([lab_k, lab_l], axis=2).astype(np.int64))
    held_list(rec, want, int(tot[1]), int(tot[3]), cap)
    held_list(isl, want_isl, int(tot[2]), int(tot[4]), icap)
    assert int(tot[0]) == int(upper.sum()) and int(tot[5]) == (1 if want.shape[0] > cap else 0) | (2 if want_isl.shape[0] > icap else 0)
    m = np.where(upper & ~np.isnan(d.loading), d.loading, 0.0)         # worst[j]: over the block's pairs that hold candidate j, as k (the row's reduction) or as l
    w = m.max(axis=0)
    w[k0:k1] = np.maximum(w[k0:k1], m.max(axis=1))
    assert np.array_equal(bits(worst), bits(w))
    return viol, island, tot


def test_pair_records_at_the_edges_of_the_extraction(g):
    cand, nk = g.pair, int(g.pair.size)
    g.check(g.L.jg_dc_pair_build(g.h, nk, cand, 0, None, 0, np.zeros(8)))
    big = nk * nk
    d = pair_call(g, cand, 0, nk, 1.0, 0, 0)[0]
    thr = float(np.nanmedian(d.loading[np.arange(nk)[None, :] > np.arange(nk)[:, None]]))      # about half of the pairs violate
    blocks = [(0, nk), (nk - 1, nk), (nk - 5, nk), (3, 4), (2, 7), (1, 8)]                      # the whole triangle; the empty last row alone and as wave 0 of a second workgroup; 1, 5, 7 rows
    if nk > 128:
        blocks += [(63, 64), (59, 66), (123, 130)]                     # rows with (k + 1) % 64 == 0: their walk starts at the next chunk
    seen = NS(mid=False, edge=False, both=False, empty=False, chunk=False)
    for k0, k1 in blocks:
        viol, island, tot = pair_held(g, cand, k0, k1, thr, big, big)
        print(g.case, "pair rows", (k0, k1), "totals", list(tot))
        assert tot[5] == 0
        seen.empty = seen.empty or (k1 == nk and not viol[-1].any() and not island[-1].any())
        seen.chunk = seen.chunk or any((k + 1) % 64 == 0 for k in range(k0, k1))
        caps, mid, edge = capacities(viol)
        seen.mid, seen.edge = seen.mid or mid, seen.edge or edge
        for cap in caps:
            pair_held(g, cand, k0, k1, thr, cap, big)
        for icap in capacities(island)[0]:
            pair_held(g, cand, k0, k1, thr, big, icap)
        if tot[1] > 1 and tot[2] > 1:                                  # the two lists overflow independently, and together
            for cap, icap, flag in ((1, big, 1), (big, 1, 2), (int(tot[1]) // 2, int(tot[2]) // 2, 3)):
                assert pair_held(g, cand, k0, k1, thr, cap, icap)[2][5] == flag
                seen.both = True
        all_tot = pair_held(g, cand, k0, k1, 0.0, big, big)[2]         # every pair with a loading violates
        none_tot = pair_held(g, cand, k0, k1, 1e300, big, 0)[2]        # none does
        assert all_tot[1] + all_tot[2] >= tot[1] + tot[2] and none_tot[1] == 0
    print(g.case, "pair: seen", vars(seen))
    assert seen.mid and seen.edge and seen.empty and seen.chunk == (nk > 128)
    if g.case == "case30test":
        assert seen.both                                               # (28 islanding pairs among its non-bridges)
    g.check(g.L.jg_dc_pair_release(g.h))


# ---- the series and the transfer screen ---------------------------------------------------------------------------------------------------------------
def series_call(g, cand, T, k0, k1, thr, cap):
    nk, rb = int(cand.size), k1 - k0
    rec, isl, tot, worst = np.full((cap + ROOM, 5), SENT), np.zeros(rb, dtype=np.int64), np.zeros(5, dtype=np.int64), np.full(nk, SENT)
    d = NS(loading=np.zeros((rb, T)), branch=np.zeros((rb, T), dtype=np.int32), count=np.zeros((rb, T), dtype=np.int32))
    g.check(g.L.jg_dc_series_screen(g.h, k0, k1, thr, cap, g.vp(rec), g.vp(isl), tot, g.vp(worst), None, None, None, g.vp(d.loading), g.vp(d.branch), g.vp(d.count)))
    return d, rec, isl[:tot[2]], tot, worst


def series_held(g, cand, T, k0, k1, thr, cap):
    rb = k1 - k0
    d, rec, isl, tot, worst = series_call(g, cand, T, k0, k1, thr, cap)
    with np.errstate(invalid="ignore"):
        viol = d.loading > thr
    lab_k, prof = np.broadcast_to(cand[k0:k1, None], (rb, T)), np.broadcast_to(np.arange(T)[None, :], (rb, T))
    want = listed(viol, np.stack([lab_k.astype(np.float64), prof.astype(np.float64), d.branch.astype(np.float64), d.loading, d.count.astype(np.float64)], axis=2))
    held_list(rec, want, int(tot[1]), int(tot[3]), cap)
    nan_row = np.isnan(d.loading).all(axis=1)
    assert int(tot[0]) == rb * T and int(tot[4]) == (1 if want.shape[0] > cap else 0)
    assert np.array_equal(isl, cand[k0:k1][nan_row]) and not np.isnan(d.loading[~nan_row]).any()      # a bridge's row is NaN throughout, no other cell is
    w = np.full(cand.size, SENT)
    w[k0:k1] = np.where(np.isnan(d.loading), 0.0, d.loading).max(axis=1)                                # the row's maximum from 0, NaN aside; other rows untouched
    assert np.array_equal(bits(worst), bits(w))
    return viol, nan_row, tot


def transfer_call(g, cand, T, k0, k1, amount, cap):
    nk, rb = int(cand.size), k1 - k0
    rec, isl, tot, worst = np.full((cap + ROOM, 5), SENT), np.zeros(rb, dtype=np.int64), np.zeros(5, dtype=np.int64), np.full(nk, SENT)
    d = NS(tc=np.zeros((rb, T)), branch=np.zeros((rb, T), dtype=np.int32))
    g.check(g.L.jg_dc_transfer_screen(g.h, k0, k1, X.CUTOFF, g.vp(amount), cap, g.vp(rec), g.vp(isl), tot, g.vp(worst), None, None, None, None, g.vp(d.tc), g.vp(d.branch)))
    return d, rec, isl[:tot[2]], tot, worst


def transfer_held(g, cand, T, k0, k1, amount, cap, whole=None):
    """whole: the uncut list of the rows [0, nk) under the same amount, for column 4"""
    rb = k1 - k0
    d, rec, isl, tot, worst = transfer_call(g, cand, T, k0, k1, amount, cap)
    with np.errstate(invalid="ignore"):
        below = d.tc < amount[None, :]
    lab_k, tr = np.broadcast_to(cand[k0:k1, None], (rb, T)), np.broadcast_to(np.arange(T)[None, :], (rb, T))
    want = listed(below, np.stack([lab_k.astype(np.float64), tr.astype(np.float64), d.branch.astype(np.float64), d.tc, np.zeros((rb, T))], axis=2))
    kept = int(tot[3])
    held_list(rec, want, int(tot[1]), kept, cap, columns=slice(0, 4))
    assert (rec[kept:] == SENT).all() and not (rec[:kept] == SENT).any()
    if whole is not None:                                              # g of the limiting branch: the same bits as in the uncut list of the whole range
        mine = whole[np.isin(whole[:, 0], cand[k0:k1])]
        assert np.array_equal(bits(rec[:kept]), bits(mine[:kept]))
    nan_row = np.isnan(d.tc).all(axis=1)
    assert int(tot[0]) == rb * T and int(tot[4]) == (1 if want.shape[0] > cap else 0)
    assert np.array_equal(isl, cand[k0:k1][nan_row]) and not np.isnan(d.tc[~nan_row]).any()
    w = np.full(cand.size, SENT)
    w[k0:k1] = np.where(nan_row, np.nan, np.where(np.isnan(d.tc), np.inf, d.tc).min(axis=1))          # the row's minimum from +inf; NaN on a bridge
    assert np.array_equal(bits(worst), bits(w))
    return below, nan_row, tot, rec[:kept]


def rect_blocks(g, nk):
    """the whole range; a bridge candidate's row alone, as wave 2 of a block of 5 and inside a block of 7; 1, 5 and 7 rows without one where the grid has them"""
    b = int(g.bridges[g.bridges >= 3][0])
    return [(0, nk), (b, b + 1), (b - 2, b + 3), (b - 3, b + 4), (nk - 1, nk), (nk - 5, nk), (nk - 7, nk)], b


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_series_records_at_the_edges_of_the_extraction(g, T):
    cand, nk = g.every, int(g.every.size)
    rhs = np.ascontiguousarray(S.profiles(g.t, T) - g.s.bus.shunt.conductance[None, :] - g.s.model.dc.shiftPower[None, :])
    g.check(g.L.jg_dc_series_set_island_mode(g.h, 0))
    g.check(g.L.jg_dc_series_build(g.h, nk, cand, 0, None, T, rhs.reshape(-1), 0, np.zeros(12)))
    big = nk * T
    thr = float(np.nanmedian(series_call(g, cand, T, 0, nk, 1.0, 0)[0].loading))
    blocks, b = rect_blocks(g, nk)
    seen = NS(mid=False, edge=False, nan=False)
    for k0, k1 in blocks:
        viol, nan_row, tot = series_held(g, cand, T, k0, k1, thr, big)
        print(g.case, "series T", T, "rows", (k0, k1), "totals", list(tot), "NaN rows", int(nan_row.sum()))
        seen.nan = seen.nan or (nan_row.any() and not nan_row.all())
        assert nan_row[b - k0] if k0 <= b < k1 else True
        assert not viol[nan_row].any()
        caps, mid, edge = capacities(viol)
        seen.mid, seen.edge = seen.mid or mid, seen.edge or edge
        for cap in caps:
            series_held(g, cand, T, k0, k1, thr, cap)
        all_tot = series_held(g, cand, T, k0, k1, 0.0, big)[2]
        none_tot = series_held(g, cand, T, k0, k1, 1e300, 0)[2]
        assert all_tot[1] >= tot[1] and none_tot[1] == 0
    assert seen.nan and seen.edge and (seen.mid or T == 1)
    g.check(g.L.jg_dc_series_release(g.h))


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_transfer_records_at_the_edges_of_the_extraction(g, T):
    cand, nk = g.every, int(g.every.size)
    g.check(g.L.jg_dc_transfer_set_island_mode(g.h, 0))
    g.check(g.L.jg_dc_transfer_build(g.h, nk, cand, 0, None, T, np.ascontiguousarray(X.directions(g.t, T)).reshape(-1), None, 0, np.zeros(12)))
    big = nk * T
    tc = transfer_call(g, cand, T, 0, nk, np.full(T, -np.inf), 0)[0].tc
    amount = np.full(T, float(np.median(tc[np.isfinite(tc)])))         # about half of the cases cannot carry it
    every, nothing = np.full(T, np.inf), np.full(T, -np.inf)
    whole = {id(a): transfer_held(g, cand, T, 0, nk, a, big)[3] for a in (amount, every)}
    blocks, b = rect_blocks(g, nk)
    seen = NS(mid=False, edge=False, nan=False)
    for k0, k1 in blocks:
        below, nan_row, tot, _ = transfer_held(g, cand, T, k0, k1, amount, big, whole[id(amount)])
        print(g.case, "transfer T", T, "rows", (k0, k1), "totals", list(tot), "NaN rows", int(nan_row.sum()))
        seen.nan = seen.nan or (nan_row.any() and not nan_row.all())
        assert nan_row[b - k0] if k0 <= b < k1 else True
        assert not below[nan_row].any()
        caps, mid, edge = capacities(below)
        seen.mid, seen.edge = seen.mid or mid, seen.edge or edge
        for cap in caps:
            transfer_held(g, cand, T, k0, k1, amount, cap, whole[id(amount)])
        all_tot = transfer_held(g, cand, T, k0, k1, every, big, whole[id(every)])[2]       # every finite capability lies below +inf
        none_tot = transfer_held(g, cand, T, k0, k1, nothing, 0)[2]
        assert all_tot[1] >= tot[1] and none_tot[1] == 0
    assert seen.nan and seen.edge and (seen.mid or T == 1)
    g.check(g.L.jg_dc_transfer_release(g.h))
