"""The builder's claims of tests/pair_layout_cases.py, on the CPU: the rows,
the pair count, the exactness of the selector values, the threshold round
trip (also at the 64-bit placements), helpers.pair_index against the header's
closed form, and that every boundary situation the GPU tests rely on is really
in the dataset."""
import numpy as np

from musicrecommendation_amd import evaluation
from musicrecommendation_amd.ensemble import pair_uniform

import pair_layout_cases as pl
from helpers import pair_index, reference_combination


def test_rows_and_pair_count():
    c = pl.build()
    ds = c.ds
    assert (ds.n_songs, ds.n_test, ds.n_train) == (4500, 19, 5)
    assert ds.n_pairs() == 73847 == pl.N_PAIRS
    row = lambda u: ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]].tolist()  # noqa: E731
    every = range(4500)
    assert row(0) == [0] and row(1) == [4499] and row(2) == [0, 4499]
    assert row(3) == [2047, 2048, 2049]
    assert row(4) == list(range(2040, 2057))
    assert row(5) == [255, 256, 511, 512, 513]
    assert row(6) == list(range(2048, 4096))
    assert row(7) == list(range(256, 512))
    assert row(8) == list(range(1990, 2310, 2))
    assert row(9) == [s for s in every if s != 2048]
    assert row(10) == [s for s in every if s not in (0, 4499)]
    assert row(11) == [s for s in every if s % 256 == 0]
    assert row(12) == [s for s in every if s % 256 == 255]
    assert row(13) == [2047, 2048, 4095, 4096]
    assert [len(row(u)) for u in range(14, 19)] == list(pl.RANDOM_SIZES)
    assert int(ds.tr_off[1]) == 4500  # a train user who heard every song
    assert pl.build() is c  # built once


def test_labels():
    c = pl.build()
    ds = c.ds
    heard = ds.heard_mask()
    lab = evaluation.label_matrix(ds)
    for u in range(ds.n_test):
        mine = ds.lab_songs[ds.lab_off[u]:ds.lab_off[u + 1]]
        assert (mine >= ds.n_songs).sum() == 1                      # one label-only song
        inside = mine[mine < ds.n_songs]
        assert heard[u, inside].sum() == 1                          # one heard label: nothing to count
        for s in pl.SPECIAL:                                        # the boundary pairs are read
            assert heard[u, s] or lab[u, s], (u, s)
        for a, b in pl.runs(c.rows[u]):                             # and both neighbours of every run
            for s in (a - 1, b + 1):
                assert not 0 <= s < 4500 or lab[u, s], (u, s)
        assert c.labels[u]["random"].size == min(3, 4500 - c.rows[u].size - c.labels[u]["boundary"].size)
    assert ds.n_extra_songs == 3 and ds.n_label_songs == int((evaluation.label_pos(ds) > 0).sum()) + 3


def test_selector_values_exact_in_f32():
    ctx = pl.context()
    for nan_at_heard in (True, False):
        ubm, ibm = pl.selector(ctx, nan_at_heard)
        assert np.nanmax(ibm) == 2 * (18 * 4500 + 4499) + 1 < 2 ** 24
        for m in (ubm, ibm):
            assert np.array_equal(m.astype(np.float32).astype(np.float64), m, equal_nan=True)
            assert np.array_equal(np.isnan(m), ctx.heard if nan_at_heard else np.zeros_like(ctx.heard))
        ok = ~np.isnan(ubm)
        assert np.all(ubm[ok] % 2 == 0) and np.all(ibm[ok] % 2 == 1)
        # a user block and a shard carry the full model's values
        sub = pl.context((7, 16), (2045, 4500))
        assert np.array_equal(pl.selector(sub, nan_at_heard)[0], ubm[7:16, 2045:4500], equal_nan=True)


def test_pair_index_is_the_closed_form():
    ds = pl.build().ds
    idx = pair_index(ds)
    assert np.array_equal(idx, pl.closed_form_index(ds))
    assert np.array_equal(idx < 0, ds.heard_mask())
    assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(ds.n_pairs()))
    for a, b in pl.USER_BLOCKS + pl.SINGLE_USERS:
        for lo, hi in ((0, 4500), (2045, 4500)):
            ctx = pl.context((a, b), (lo, hi))
            assert ctx.pair_base == a * 4500 - int(ds.te_off[a])
            assert np.array_equal(ctx.idx, idx[a:b, lo:hi])
            assert np.array_equal(ctx.idx, pl.closed_form_index(ctx.ds, ctx.pair_base)[:, lo:hi])


def test_threshold_round_trip():
    ds = pl.build().ds
    thr = pl.thresholds_of_interest(ds)
    assert thr[0] == 0 and thr[-1] == ds.n_pairs() and np.all(np.diff(thr) > 0)
    assert thr.size == 685, thr.size  # eleven sweep calls of at most 64 parameters
    for t in thr.tolist():
        p = pl.param_of(t, ds.n_pairs())
        assert int(p * ds.n_pairs()) == t and 0.0 <= p <= 1.0
    idx = pair_index(ds)
    for u in range(ds.n_test):  # the pair before and after every run is bracketed by thresholds
        for a, b in pl.runs(pl.build().rows[u]):
            for s in (a - 1, b + 1):
                if 0 <= s < 4500:
                    assert idx[u, s] in thr and idx[u, s] + 1 in thr, (u, s)


def test_wide_placements():
    for crossing in (2 ** 31, 2 ** 32):
        ctx, thr = pl.wide_context(crossing)
        assert ctx.n_pairs == 2 ** 32 + 10 ** 6 and ctx.shape == (9, 4500) and ctx.pair_base > 0
        assert ctx.idx[11 - 7, 2050] == crossing and ctx.idx[11 - 7, 2048] == -1
        row = ctx.idx[11 - 7]
        assert row[row >= 0].min() < crossing < row.max()            # inside one row
        assert ctx.idx.max() < ctx.n_pairs
        assert np.array_equal(ctx.idx, pl.closed_form_index(ctx.ds, ctx.pair_base))
        takes = set()
        for t in thr:
            p = pl.param_of(t, ctx.n_pairs)
            assert int(p * float(ctx.n_pairs)) == t
            takes.add(int(((ctx.idx >= 0) & (ctx.idx < t)).sum()))
        assert len(takes) == len(thr)                                # every threshold selects another set
        assert 0 in takes and int((ctx.idx >= 0).sum()) in takes     # none and all of the context
    # 2^32: pair_base itself does not fit 32 bits
    assert pl.wide_context(2 ** 32)[0].pair_base > 2 ** 31


def test_draws_are_pair_uniform():
    rng = np.random.default_rng(3)
    idx = np.concatenate([np.arange(0, 200), rng.integers(0, 2 ** 33, size=300), [2 ** 31 - 1, 2 ** 31, 2 ** 32, -1]])
    for seed in (0, 3, 2 ** 64 - 1):
        got = pl.draws(seed, idx)
        exp = [pair_uniform(seed, int(i)) if i >= 0 else 2.0 for i in idx]
        assert got.tolist() == exp
    ctx = pl.context((16, 19))
    ubm, ibm = pl.selector(ctx)
    exp = reference_combination("stochastic", ubm, ibm, 0.37, ctx.idx, ctx.n_pairs, seed=5)
    assert np.array_equal(pl.restate(ctx, "stochastic", ubm, ibm, 0.37, "f64", seed=5), exp, equal_nan=True)


def test_boundary_situations_are_present():
    c = pl.build()
    ds = c.ds
    heard = ds.heard_mask()
    assert heard[:, 0].any() and heard[:, 4499].any()                # the model's first and last song
    # adjacent heard songs across every 2048- and 256-song block boundary
    for cut in (2048, 4096):
        assert (heard[:, cut - 1] & heard[:, cut]).any()
    for cut in (256, 512):
        assert (heard[:, cut - 1] & heard[:, cut]).any()
    # a heard song on a block's first and last song with the neighbour across the boundary unheard
    assert (heard[:, 2048] & ~heard[:, 2047]).any() and (heard[:, 2047] & ~heard[:, 2048]).any()
    assert (heard[:, 256] & ~heard[:, 255]).any() and (heard[:, 255] & ~heard[:, 256]).any()
    # whole blocks without a pair, and more than 18 heard songs in a block
    assert heard[6, 2048:4096].all() and heard[7, 256:512].all()
    assert heard[8, 0:2048].sum() > 18
    # rows with one and two pairs
    assert (~heard[9]).sum() == 1 and (~heard[10]).sum() == 2
    for lo, hi in pl.SHARDS:
        assert heard[:, lo].any() and heard[:, hi - 1].any(), (lo, hi)      # on the shard's first / last song
        assert (~heard[:, lo]).any() and (~heard[:, hi - 1]).any(), (lo, hi)
    assert heard[6, 2048:4096].all()                                 # (2048, 4096): user 7 has no pair
    # a heard song on the first song of a 2048-song block counted from a shard's song_lo
    for lo, hi in pl.SHARDS:
        starts = range(lo, hi, pl.BLOCK)
        assert any(heard[:, s].any() for s in starts), (lo, hi)
    assert heard[:, 2045 + 2048].any()                               # (2045, 4500): its second block
    # the evaluation's two paths: 19 users take 2 user blocks, every block at most 16 one
    assert (ds.n_test + 15) // 16 == 2 and all((b - a + 15) // 16 == 1 for a, b in pl.USER_BLOCKS)
    assert pl.USER_BLOCKS[2] == pl.WIDE_BLOCK == (7, 16)


def test_value_models():
    for dtype, npt in (("f32", np.float32), ("f64", np.float64)):
        ctx = pl.context()
        m = pl.value_models(ctx, dtype)
        for name, x in m.items():
            assert x.dtype == npt and np.array_equal(np.isnan(x), ctx.heard) or name == "empty", name
        assert np.nanmax(m["negative"]) < 0
        zeros = m["mixed"][m["mixed"] == 0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
        assert pl.extremes(m["mixed"].astype(np.float64)) == (-2.5, 1.5)
        mn, mx = pl.extremes(m["boundary"].astype(np.float64))
        assert mn < 0 < mx and (mn, mx) == (float(npt(-0.3137)), float(npt(0.7731)))
        den = m["denormal"].astype(np.float64)
        assert 0 < np.nanmin(den) and np.nanmax(den) < float(np.finfo(npt).tiny)
        assert np.unique(den[~np.isnan(den)]).size == 40                 # distinct levels
        pred, _tp = pl.counts(ctx, den, *pl.extremes(den))
        flushed = np.where(np.isnan(den), np.nan, 0.0)
        pred0, _tp0 = pl.counts(ctx, flushed, *pl.extremes(flushed))
        assert pred.any() and not pred0.any()                            # a flushed reading counts nothing
        for name, ext in (("plus_inf", np.inf), ("minus_inf", -np.inf)):
            x = m[name].astype(np.float64)
            e = pl.extremes(x)
            assert ext in e and np.isfinite(e).sum() == 1
            pred, tp = pl.counts(ctx, x, *e)
            assert not pred.any() and not tp.any()                       # as the expression gives
        assert pl.extremes(m["empty"].astype(np.float64)) == (np.inf, -np.inf)
