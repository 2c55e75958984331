"""The row block of a screen call, REUSED: jg_dc_pair_screen, jg_dc_series_screen and jg_dc_transfer_screen called several times on ONE build with blocks
of 3, then 8, then 3 rows, so the block's buffers are allocated, grown, and used again larger than the call needs (csrc/jg_dc_records.hpp: dc_block_grow,
dc_list_grow).  The Python drivers never do that (they release after every call and only their last block is smaller), so the calls go through the
library's C entry points directly, on one dcPowerFlow handle that stays open.

case14test, T = 65 profiles / transfers (ldt = 128, the last group of 64 lanes holds one), overlapping row ranges whose first row is no multiple of a tile.
Held bit for bit (NaN positions included) against the same rows of ONE whole-range call on a fresh build of the same handle: every dense array, the record
list, the islanding list and the totals.  Free device memory is not looked at: the device is shared."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import dc_pair_reference as P
import dc_series_reference as S
import dc_transfer_reference as X
from conftest import load_case

pytestmark = pytest.mark.gpu

T = 65
BLOCKS = ((1, 4), (2, 10), (9, 12))                                     # 3, 8, 3 rows; they overlap, and 1, 2, 9 are no multiples of 4
CAP = 4096                                                             # room for every record of the grid (18 candidates x 65 cases)


@pytest.fixture(scope="module")
def g(jg):
    t = load_case("case14test")
    s = jg.powerSystem(t)
    an = jg.dcPowerFlow(s)
    L, check = jg._lib.lib(), jg._lib.check
    keep = NS(rhs=np.ascontiguousarray(jg.dcpowerflow._base_rhs(s), dtype=np.float64), rating=np.ascontiguousarray(P.rating_of(t), dtype=np.float64))
    vp = lambda a: None if a is None else a.ctypes.data_as(jg._lib.VP)
    check(L.jg_dc_set_rhs(an._h, keep.rhs))
    check(L.jg_dc_set_rating(an._h, vp(keep.rating)))
    rhs = np.ascontiguousarray(S.profiles(t, T) - s.bus.shunt.conductance[None, :] - s.model.dc.shiftPower[None, :])
    yield NS(L=L, check=check, vp=vp, h=an._h, keep=keep, pair=jg.pairCandidates(s), every=jg.shedCandidates(s), rhs=rhs, dirs=np.ascontiguousarray(X.directions(t, T)),
             bridges=np.flatnonzero(jg.bridges(s)) + 1)
    an.close()


def rows_of(whole, cand, k0, k1):
    """what a call on the rows [k0, k1) has to give, out of the whole-range call (its rows start at 0): dense rows, records, islanding entries"""
    dense, rec, isl, _ = whole
    lab = cand[k0:k1]
    return {n: a[k0:k1] for n, a in dense.items()}, rec[np.isin(rec[:, 0], lab)], isl[np.isin(isl if isl.ndim == 1 else isl[:, 0], lab)]


def held(got, want, cases, tail):
    dense, rec, isl, tot = got
    wd, wr, wi = want
    for n, a in dense.items():
        assert a is None or np.array_equal(a, wd[n], equal_nan=True), n
    assert np.array_equal(rec, wr, equal_nan=True) and np.array_equal(isl, wi)
    assert list(tot) == [cases, len(wr), len(wi), len(wr)] + tail, (list(tot), cases, len(wr), len(wi))


def test_the_pair_screen_on_a_block_it_grows_and_reuses(g):
    cand, nk = g.pair, int(g.pair.size)
    upper = np.arange(nk)[None, :] > np.arange(nk - 1)[:, None]

    def build():
        g.check(g.L.jg_dc_pair_build(g.h, nk, cand, 0, None, 0, np.zeros(8)))

    def call(k0, k1, thr, det):
        rb = k1 - k0
        rec, isl, tot = np.zeros((CAP, 5)), np.zeros((CAP, 2), dtype=np.int64), np.zeros(6, dtype=np.int64)
        d = dict(loading=np.zeros((rb, nk)), branch=np.zeros((rb, nk), dtype=np.int32), count=np.zeros((rb, nk), dtype=np.int32),
                 determinant=np.zeros((rb, nk)) if det else None)
        g.check(g.L.jg_dc_pair_screen(g.h, k0, k1, thr, CAP, g.vp(rec), CAP, g.vp(isl), tot, None, g.vp(d["loading"]), g.vp(d["branch"]), g.vp(d["count"]),
                                      g.vp(d["determinant"])))
        return d, rec[:tot[3]], isl[:tot[4]], tot

    build()
    thr = float(np.nanmedian(call(0, nk - 1, 1.0, False)[0]["loading"][upper]))          # splits the pairs: about half of them are records
    build()
    whole = call(0, nk - 1, thr, True)
    print("pair screen: threshold", thr, "totals of the whole range", list(whole[3]))
    assert 0 < whole[3][1] < whole[3][0] and whole[3][5] == 0
    build()
    for (k0, k1), det in zip(BLOCKS, (False, True, False)):            # the determinants only on the second call: allocated then, kept for the third
        want = rows_of(whole, cand, k0, k1)
        held(call(k0, k1, thr, det), want, sum(nk - 1 - k for k in range(k0, k1)), [len(want[2]), 0])
    g.check(g.L.jg_dc_pair_release(g.h))


@pytest.mark.parametrize("mode", [0, 1])
def test_the_series_screen_on_a_block_it_grows_and_reuses(g, mode):
    cand, nk = g.every, int(g.every.size)
    assert np.isin(g.bridges, cand).all() and np.isin(g.bridges, cand[2:10]).any()

    def build():
        g.check(g.L.jg_dc_series_set_island_mode(g.h, mode))
        g.check(g.L.jg_dc_series_build(g.h, nk, cand, 0, None, T, g.rhs.reshape(-1), 0, np.zeros(12)))

    def call(k0, k1, thr):
        rb = k1 - k0
        rec, isl, tot = np.zeros((CAP, 5)), np.zeros(rb, dtype=np.int64), np.zeros(5, dtype=np.int64)
        d = dict(loading=np.zeros((rb, T)), branch=np.zeros((rb, T), dtype=np.int32), count=np.zeros((rb, T), dtype=np.int32))
        g.check(g.L.jg_dc_series_screen(g.h, k0, k1, thr, CAP, g.vp(rec), g.vp(isl), tot, None, None, None, None, g.vp(d["loading"]), g.vp(d["branch"]), g.vp(d["count"])))
        return d, rec[:tot[3]], isl[:tot[2]], tot

    build()
    thr = float(np.nanmedian(call(0, nk, 1.0)[0]["loading"]))
    build()
    whole = call(0, nk, thr)
    print("series screen, island mode", mode, ": threshold", thr, "totals of the whole range", list(whole[3]))
    assert 0 < whole[3][1] < whole[3][0] and whole[3][4] == 0 and whole[3][2] == (0 if mode else g.bridges.size)
    build()
    for k0, k1 in BLOCKS:
        held(call(k0, k1, thr), rows_of(whole, cand, k0, k1), (k1 - k0) * T, [0])
    g.check(g.L.jg_dc_series_release(g.h))


@pytest.mark.parametrize("mode", [0, 1])
def test_the_transfer_screen_on_a_block_it_grows_and_reuses(g, mode):
    cand, nk = g.every, int(g.every.size)

    def build():
        g.check(g.L.jg_dc_transfer_set_island_mode(g.h, mode))
        g.check(g.L.jg_dc_transfer_build(g.h, nk, cand, 0, None, T, g.dirs.reshape(-1), None, 0, np.zeros(12)))

    def call(k0, k1, amount):
        rb = k1 - k0
        rec, isl, tot = np.zeros((CAP, 5)), np.zeros(rb, dtype=np.int64), np.zeros(5, dtype=np.int64)
        d = dict(capabilityCases=np.zeros((rb, T)), branch=np.zeros((rb, T), dtype=np.int32))
        g.check(g.L.jg_dc_transfer_screen(g.h, k0, k1, X.CUTOFF, g.vp(amount), CAP, g.vp(rec), g.vp(isl), tot, None, None, None, None, None,
                                          g.vp(d["capabilityCases"]), g.vp(d["branch"])))
        return d, rec[:tot[3]], isl[:tot[2]], tot

    build()
    tc = call(0, nk, None)[0]["capabilityCases"]
    amount = np.full(T, float(np.median(tc[np.isfinite(tc)])))          # about half of the cases cannot carry it
    build()
    whole = call(0, nk, amount)
    print("transfer screen, island mode", mode, ": amount", amount[0], "totals of the whole range", list(whole[3]))
    assert 0 < whole[3][1] < whole[3][0] and whole[3][4] == 0 and whole[3][2] == (0 if mode else g.bridges.size)
    build()
    for k0, k1 in BLOCKS:
        held(call(k0, k1, amount), rows_of(whole, cand, k0, k1), (k1 - k0) * T, [0])
    g.check(g.L.jg_dc_transfer_release(g.h))
