"""GPU: the pair index of csrc/mr_ensemble.hip (k_combine, k_combine3,
k_sweep_minmax, k_sweep_pred, k_sweep_tp) and the evaluation kernels on the
hand-built heard layout of tests/pair_layout_cases.py, bit for bit against the
numpy statement (helpers.pair_index, reference_combination,
evaluation.threshold_counts / map_from_counts): heard songs on the first and
last song of a block and of a shard, runs across block boundaries, blocks and
a whole shard without a pair, rows with one and two pairs, shards of width 1
and 2, user blocks on both evaluation paths, pair indices past 2^31 and 2^32,
models that are finite at heard songs (the masks the kernels form themselves),
and values the level test has not met: negative ranges, both zeros, ranges
that straddle zero, denormals, infinities and a model without a pair.

The selector models (ubm = 2g, ibm = 2g + 1) show take_ibm of every pair in
the parity of a materialised output; the indicator models (0 / 1) show it in
the counts. Extremes are compared with == (the sign of a zero extreme is not
defined by the order of the reduction), everything else exactly."""
import functools

import numpy as np
import pytest
import torch

from musicrecommendation_amd import _lib
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import sweep_kind

import pair_layout_cases as pl

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f64")
KINDS = ("linear", "aggregation", "stochastic")
SEEDS = (3, 2 ** 63 + 11)
FULL = (0, pl.N_TEST)
ALL_SONGS = (0, pl.N_SONGS)
CLASSES = np.arange(pl.N_SONGS, dtype=np.int32)   # the whole pred / tp tables come back
# a partition of the songs that holds both shards of width 1 and the shard in which user 7 has no pair
PARTITION = ((0, 255), (255, 256), (256, 2048), (2048, 4096), (4096, 4499), (4499, 4500))


@functools.lru_cache(maxsize=None)
def ctx_of(users=FULL, shard=ALL_SONGS):
    return pl.context(users, shard)


@functools.lru_cache(maxsize=None)
def wide(crossing):
    return pl.wide_context(crossing)


MODELS = {"selector": pl.selector, "indicator": pl.indicator}


class Dev:
    """One engine context (a block of test users x a song shard, one dtype)
    and the entry points under test, with host arrays out."""

    def __init__(self, users, shard, dtype):
        ctx = ctx_of(users, shard)
        self.dtype, self.npt = dtype, np.float32 if dtype == "f32" else np.float64
        self.ds = ctx.ds
        self.e = Engine(ctx.ds, out_dtype=dtype, song_lo=shard[0], song_hi=shard[1], ibm_route="two_hop")
        assert (self.e.song_lo, self.e.song_hi, self.e.n_test) == (shard[0], shard[1], users[1] - users[0])
        self.shape = ctx.shape
        self.full_width = shard == ALL_SONGS
        self._up = {}

    def up(self, x):
        t = torch.from_numpy(np.array(x, dtype=self.npt)).cuda()   # (a copy: the case arrays are read-only)
        torch.cuda.synchronize()
        return t

    def models(self, ctx, name, nan_at_heard=True):
        """The (ubm, ibm) device tensors of a named exact model, uploaded once."""
        key = (name, nan_at_heard)
        if key not in self._up:
            self._up[key] = tuple(self.up(m) for m in MODELS[name](ctx, nan_at_heard))
        return self._up[key]

    def out(self):
        t = torch.full(self.shape, -7.0, dtype=torch.float32 if self.dtype == "f32" else torch.float64, device="cuda")
        torch.cuda.synchronize()
        return t

    @staticmethod
    def host(t):
        return t.cpu().numpy().astype(np.float64)

    def combine(self, ctx, kind, u_t, i_t, p, seed=0):
        o = self.out()
        self.e.combine(sweep_kind(kind), p, u_t.data_ptr(), i_t.data_ptr(), o.data_ptr(), seed=seed,
                       pair_base=ctx.pair_base, n_pairs=ctx.n_pairs)
        return o

    def combine_all(self, ctx, u_t, i_t, alpha, pct, prob, seed=0):
        outs = (self.out(), self.out(), self.out())
        mm = self.e.combine_all(alpha, pct, prob, u_t.data_ptr(), i_t.data_ptr(), tuple(o.data_ptr() for o in outs),
                                seed=seed, pair_base=ctx.pair_base, n_pairs=ctx.n_pairs)
        return outs, mm

    def counts(self, t, mn, mx, n_thr=10):
        return self.e.eval_counts(t.data_ptr(), mn, mx, self.ds.lab_off, self.ds.lab_songs, n_thresholds=n_thr)

    def class_counts(self, ts, mns, mxs, n_thr=10):
        block = torch.full((len(ts), 2, pl.N_SONGS, n_thr), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.e.eval_class_counts([t.data_ptr() for t in ts], mns, mxs, self.ds.lab_off, self.ds.lab_songs, CLASSES,
                                 block.data_ptr(), n_thresholds=n_thr)
        return block.cpu().numpy()

    def eval_map(self, t, mn, mx, n_thr=10):
        return self.e.eval_map(t.data_ptr(), mn, mx, self.ds.lab_off, self.ds.lab_songs, pos_of(self.ds),
                               self.ds.n_label_songs, n_thresholds=n_thr)

    def sweep_kw(self, ctx, seed):
        return dict(seed=seed, pair_base=ctx.pair_base, n_pairs=ctx.n_pairs)

    def sweep_minmax(self, ctx, kind, u_t, i_t, params, seed=0):
        return self.e.sweep_minmax(sweep_kind(kind), params, u_t.data_ptr(), i_t.data_ptr(), **self.sweep_kw(ctx, seed))

    def sweep_counts(self, ctx, kind, u_t, i_t, params, mns, mxs, seed=0, n_thr=10):
        block = torch.full((len(params), 2, pl.N_SONGS, n_thr), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.e.sweep_class_counts(sweep_kind(kind), params, u_t.data_ptr(), i_t.data_ptr(), mns, mxs, self.ds.lab_off,
                                  self.ds.lab_songs, CLASSES, block.data_ptr(), n_thresholds=n_thr,
                                  **self.sweep_kw(ctx, seed))
        return block.cpu().numpy()

    def sweep_map(self, ctx, kind, u_t, i_t, params, seed=0, n_thr=10):
        return self.e.sweep_map(sweep_kind(kind), params, u_t.data_ptr(), i_t.data_ptr(), self.ds.lab_off,
                                self.ds.lab_songs, pos_of(self.ds), self.ds.n_label_songs, n_thresholds=n_thr,
                                minmax=True, **self.sweep_kw(ctx, seed))


_pos = {}


def pos_of(ds):
    if id(ds) not in _pos:
        from musicrecommendation_amd import evaluation

        _pos[id(ds)] = (ds, evaluation.label_pos(ds))
    return _pos[id(ds)][1]


_devs = {}


def dev(users, shard, dtype) -> Dev:
    """Engine contexts are created once per module (closed by the fixture below)."""
    key = (users, shard, dtype)
    if key not in _devs:
        _devs[key] = Dev(users, shard, dtype)
    return _devs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for d in _devs.values():
        d._up.clear()
        d.e.close()
    _devs.clear()


def block_of(ctx, pred, tp):
    """The class block (classes = every song) a context's counts give: 0 outside its songs."""
    out = np.zeros((2, pl.N_SONGS, pred.shape[1]), dtype=np.int64)
    out[0, ctx.lo:ctx.hi], out[1, ctx.lo:ctx.hi] = pred, tp
    return out


def thresholds_in(ctx, cap=64):
    """The thresholds of interest whose pair (the first ubm pair, or the last
    ibm pair) lies in the context; evenly thinned to at most `cap`, both ends kept."""
    thr = pl.thresholds_of_interest(pl.build().ds)
    mine = ctx.idx[ctx.idx >= 0]
    thr = thr[np.isin(thr, mine) | np.isin(thr - 1, mine)]
    if thr.size > cap:
        thr = thr[np.unique(np.linspace(0, thr.size - 1, cap).astype(int))]
    return thr.tolist()


def few(seq, n):
    seq = list(seq)
    return [seq[i] for i in sorted(set(np.linspace(0, len(seq) - 1, min(n, len(seq))).astype(int).tolist()))]


def check_materialised(users, shard, ctx, model, cases, nan_at_heard=True, n_thrs=(10,)):
    """mr_combine_device per case (kind, param, seed) and every mr_eval_* call
    on its output, both dtypes, against numpy. Returns {dtype: [output tensors]}."""
    ubm, ibm = MODELS[model](ctx, nan_at_heard)
    outs = {}
    for dtype in DTYPES:
        d = dev(users, shard, dtype)
        u_t, i_t = d.models(ctx, model, nan_at_heard)
        outs[dtype] = []
        for kind, p, seed in cases:
            x = pl.restate(ctx, kind, ubm, ibm, p, dtype, seed)
            what = (users, shard, model, dtype, kind, p, seed)
            if kind != "linear":   # the mask is the kernel's own when the models are finite at heard songs
                assert np.array_equal(np.isnan(x), ctx.heard), what
                if model == "selector":   # the parity of an output is take_ibm
                    key = ctx.idx if kind == "aggregation" else pl.draws(seed, ctx.idx)
                    take = key < (int(p * ctx.n_pairs) if kind == "aggregation" else p)
                    assert np.array_equal((x % 2 == 1)[~ctx.heard], take[~ctx.heard]), what
            o = d.combine(ctx, kind, u_t, i_t, p, seed)
            assert np.array_equal(d.host(o), x, equal_nan=True), what
            ext = pl.extremes(x)
            assert d.e.eval_minmax(o.data_ptr()) == ext, what
            for n_thr in n_thrs:
                pred, tp = pl.counts(ctx, x, *ext, n_thr)
                got_p, got_t = d.counts(o, *ext, n_thr)
                assert np.array_equal(got_p, pred) and np.array_equal(got_t, tp), what + (n_thr,)
                if d.full_width and ext[0] <= ext[1]:
                    assert d.eval_map(o, *ext, n_thr) == pl.mean_ap(ctx, pred, tp), what + (n_thr,)
            outs[dtype].append((o, x, ext))
    return outs


def check_two_models(users, shard, ctx, outs, n_thr=10):
    """mr_eval_class_counts_device with two models in one call."""
    for dtype in DTYPES:
        d = dev(users, shard, dtype)
        (o1, x1, e1), (o2, x2, e2) = outs[dtype][0], outs[dtype][-1]
        block = d.class_counts([o1, o2], [e1[0], e2[0]], [e1[1], e2[1]], n_thr)
        for m, (x, e) in enumerate(((x1, e1), (x2, e2))):
            assert np.array_equal(block[m], block_of(ctx, *pl.counts(ctx, x, *e, n_thr))), (users, shard, dtype, m)


def check_combine_all(users, shard, ctx, model, alpha, pct, prob, seed, nan_at_heard=True):
    """mr_combine_all_device: the three outputs and the carried min / max."""
    ubm, ibm = MODELS[model](ctx, nan_at_heard)
    for dtype in DTYPES:
        d = dev(users, shard, dtype)
        u_t, i_t = d.models(ctx, model, nan_at_heard)
        outs, mm = d.combine_all(ctx, u_t, i_t, alpha, pct, prob, seed)
        for kind, p, o, got_mm in zip(KINDS, (alpha, pct, prob), outs, mm):
            x = pl.restate(ctx, kind, ubm, ibm, p, dtype, seed)
            what = (users, shard, model, dtype, kind, p)
            assert np.array_equal(d.host(o), x, equal_nan=True), what
            assert got_mm == pl.extremes(x), what


def check_sweep(users, shard, ctx, model, kind, params, seed=0, nan_at_heard=True, n_thr=10, glob=None,
                with_counts=True):
    """mr_sweep_minmax_device, mr_sweep_class_counts_device and (a context over
    every song) mr_sweep_map_device at `params`, both dtypes, against numpy.
    glob: {param: (mn, mx)} the extremes handed to the counts (default: the
    context's own). with_counts=False: the extremes only. Returns {dtype:
    (mins, maxs, block)}."""
    ubm, ibm = MODELS[model](ctx, nan_at_heard)
    xs = [pl.restate(ctx, kind, ubm, ibm, p, "f64", seed) for p in params]   # exact in f32 for these models
    if kind == "linear":
        assert all(np.array_equal(x.astype(np.float32).astype(np.float64), x, equal_nan=True) for x in xs)
    exts = [pl.extremes(x) for x in xs]
    use = exts if glob is None else [glob[p] for p in params]
    mns, mxs = np.array([e[0] for e in use]), np.array([e[1] for e in use])
    blocks = with_counts and np.stack([block_of(ctx, *pl.counts(ctx, x, mn, mx, n_thr))
                                       for x, mn, mx in zip(xs, mns, mxs)])
    got = {}
    for dtype in DTYPES:
        d = dev(users, shard, dtype)
        u_t, i_t = d.models(ctx, model, nan_at_heard)
        what = (users, shard, model, dtype, kind, seed, nan_at_heard)
        mn, mx = d.sweep_minmax(ctx, kind, u_t, i_t, params, seed)
        assert list(zip(mn.tolist(), mx.tolist())) == exts, what
        if not with_counts:
            got[dtype] = (mn, mx, None)
            continue
        block = d.sweep_counts(ctx, kind, u_t, i_t, params, mns, mxs, seed, n_thr)
        for j in range(len(params)):
            assert np.array_equal(block[j], blocks[j]), what + (j, params[j])
        if d.full_width and glob is None and all(a <= b for a, b in exts):
            maps, mm = d.sweep_map(ctx, kind, u_t, i_t, params, seed, n_thr)
            assert maps == [pl.mean_ap(ctx, b[0], b[1]) for b in blocks], what
            assert list(zip(mm[:, 0].tolist(), mm[:, 1].tolist())) == exts, what
        got[dtype] = (mn, mx, block)
    return got


def agg_params(ctx, n):
    return [pl.param_of(t, ctx.n_pairs) for t in few(thresholds_in(ctx), n)]


# ---------------------------------------------------------------------------
# full range
# ---------------------------------------------------------------------------
def test_full_range_materialised():
    ctx = ctx_of()
    cases = [("linear", 0.5, 0), ("linear", 0.37, 0)]
    cases += [("aggregation", p, 0) for p in agg_params(ctx, 6) + [0.5]]
    cases += [("stochastic", p, seed) for seed in SEEDS for p in (0.37, 0.9)]
    outs = check_materialised(FULL, ALL_SONGS, ctx, "selector", cases, n_thrs=(10, 11))
    check_two_models(FULL, ALL_SONGS, ctx, outs)
    check_two_models(FULL, ALL_SONGS, ctx, outs, n_thr=11)
    for seed in SEEDS:
        for pct in agg_params(ctx, 3):
            check_combine_all(FULL, ALL_SONGS, ctx, "selector", 0.37, pct, 0.37, seed)
    check_materialised(FULL, ALL_SONGS, ctx, "indicator", [("aggregation", 0.5, 0), ("stochastic", 0.5, SEEDS[0])])


N_INTEREST = 685   # thresholds of interest (tests/test_pair_layout_cases_cpu.py): eleven calls of at most 64


@pytest.mark.parametrize("call", range((N_INTEREST + 63) // 64))
def test_full_range_aggregation_at_every_threshold_of_interest(call):
    """The indicator models: pred[s][t] is the number of users that took ibm at
    s, so the counts show every pair's selection; 64 parameters per call."""
    ctx = ctx_of()
    every = pl.thresholds_of_interest(pl.build().ds).tolist()
    assert len(every) == N_INTEREST
    thr = every[64 * call:64 * call + 64]
    got = check_sweep(FULL, ALL_SONGS, ctx, "indicator", "aggregation", [pl.param_of(t, ctx.n_pairs) for t in thr])
    block = got["f64"][2]
    for j, t in enumerate(thr):   # what the statement means, said directly once more
        took = ((ctx.idx >= 0) & (ctx.idx < t)).sum(axis=0)
        if 0 < t < ctx.n_pairs:    # extremes (0, 1): predicted at every level below 1.0
            assert np.array_equal(block[j, 0, :, 0], took) and np.array_equal(block[j, 0, :, 9], took), t
    assert block[:, 1].any()       # true positives are counted (the labels sit on the boundary pairs)


def test_full_range_sweep_selector_and_stochastic():
    ctx = ctx_of()
    check_sweep(FULL, ALL_SONGS, ctx, "selector", "aggregation", agg_params(ctx, 64))
    check_sweep(FULL, ALL_SONGS, ctx, "selector", "linear", [1.0, 0.5, 0.0])
    for seed in SEEDS:
        for model in MODELS:
            check_sweep(FULL, ALL_SONGS, ctx, model, "stochastic", [0.0, 0.1, 0.37, 0.5, 0.9, 1.0], seed)
    check_sweep(FULL, ALL_SONGS, ctx, "indicator", "stochastic", [0.25, 0.5, 0.75], SEEDS[0], n_thr=11)


def test_sweep_counts_are_the_materialised_outputs_counts():
    """Sweep counts of the indicator models = the counts of the materialised
    outputs (device against device), both = numpy's (the checks above)."""
    ctx = ctx_of()
    params = agg_params(ctx, 5)
    got = check_sweep(FULL, ALL_SONGS, ctx, "indicator", "aggregation", params)
    for dtype in DTYPES:
        d = dev(FULL, ALL_SONGS, dtype)
        u_t, i_t = d.models(ctx, "indicator")
        mn, mx, block = got[dtype]
        for j, p in enumerate(params):
            o = d.combine(ctx, "aggregation", u_t, i_t, p)
            assert d.e.eval_minmax(o.data_ptr()) == (mn[j], mx[j])
            pred, tp = d.counts(o, mn[j], mx[j])
            assert np.array_equal(block[j, 0], pred) and np.array_equal(block[j, 1], tp), (dtype, j)


# ---------------------------------------------------------------------------
# song shards and user blocks
# ---------------------------------------------------------------------------
def layout_cases(ctx, n_agg=4):
    agg = agg_params(ctx, n_agg) or [0.5]   # a context without a threshold of its own still runs
    return ([("linear", 0.37, 0)] + [("aggregation", p, 0) for p in agg]
            + [("stochastic", 0.37, seed) for seed in SEEDS]), agg


@pytest.mark.parametrize("shard", pl.SHARDS[1:])
def test_song_shard(shard):
    ctx = ctx_of(FULL, shard)
    cases, agg = layout_cases(ctx)
    outs = check_materialised(FULL, shard, ctx, "selector", cases)
    check_two_models(FULL, shard, ctx, outs)
    check_combine_all(FULL, shard, ctx, "selector", 0.37, agg[0], 0.37, SEEDS[0])
    check_sweep(FULL, shard, ctx, "indicator", "aggregation", agg_params(ctx, 64) or [0.5])
    check_sweep(FULL, shard, ctx, "selector", "aggregation", agg)
    check_sweep(FULL, shard, ctx, "indicator", "stochastic", [0.1, 0.5, 0.9], SEEDS[0])


@pytest.mark.parametrize("users", pl.USER_BLOCKS + pl.SINGLE_USERS)
def test_user_block(users):
    ctx = ctx_of(users, ALL_SONGS)
    cases, agg = layout_cases(ctx)
    outs = check_materialised(users, ALL_SONGS, ctx, "selector", cases)
    check_two_models(users, ALL_SONGS, ctx, outs)
    check_combine_all(users, ALL_SONGS, ctx, "selector", 0.37, agg[-1], 0.37, SEEDS[1])
    check_sweep(users, ALL_SONGS, ctx, "indicator", "aggregation", agg_params(ctx, 64))
    check_sweep(users, ALL_SONGS, ctx, "selector", "aggregation", agg)
    check_sweep(users, ALL_SONGS, ctx, "indicator", "stochastic", [0.1, 0.5, 0.9], SEEDS[1])


@pytest.mark.parametrize("kind,model", [("aggregation", "indicator"), ("aggregation", "selector"),
                                        ("stochastic", "indicator")])
@pytest.mark.parametrize("what", ["song shards", "user blocks"])
def test_parts_combine_to_the_full_range(what, kind, model):
    """Each context alone, the extremes combined with min / max and the class
    blocks added: the full-range results (every part checked against numpy,
    the sums formed from the device's own blocks)."""
    ctx = ctx_of()
    params = agg_params(ctx, 16) if kind == "aggregation" else [0.1, 0.5, 0.9]
    seed = SEEDS[0]
    full = check_sweep(FULL, ALL_SONGS, ctx, model, kind, params, seed)
    glob = {p: (full["f64"][0][j], full["f64"][1][j]) for j, p in enumerate(params)}
    layout = [(FULL, s) for s in PARTITION] if what == "song shards" else [(u, ALL_SONGS) for u in pl.USER_BLOCKS]
    parts = [(check_sweep(u, s, ctx_of(u, s), model, kind, params, seed, with_counts=False),
              check_sweep(u, s, ctx_of(u, s), model, kind, params, seed, glob=glob)) for u, s in layout]
    for dtype in DTYPES:
        mn = np.min([own[dtype][0] for own, _g in parts], axis=0)
        mx = np.max([own[dtype][1] for own, _g in parts], axis=0)
        assert np.array_equal(mn, full[dtype][0]) and np.array_equal(mx, full[dtype][1]), dtype
        total = sum(g[dtype][2].astype(np.int64) for _own, g in parts)
        assert np.array_equal(total, full[dtype][2]), dtype


# ---------------------------------------------------------------------------
# pair indices past 32 bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("crossing", [2 ** 31, 2 ** 32])
def test_wide_placement(crossing):
    """The block [7, 16) placed so that pair index 2^31 / 2^32 falls inside
    one of its rows, in a model of 2^32 + 10^6 pairs: all five index kernels."""
    ctx, thr = wide(crossing)
    users = pl.WIDE_BLOCK
    params = [pl.param_of(t, ctx.n_pairs) for t in thr]
    cases = [("aggregation", p, 0) for p in params] + [("stochastic", 0.37, SEEDS[0])]
    check_materialised(users, ALL_SONGS, ctx, "selector", cases)                                  # k_combine
    for pct in params[:3]:
        check_combine_all(users, ALL_SONGS, ctx, "selector", 0.37, pct, 0.37, SEEDS[0])            # k_combine3
    got = {}
    for model in MODELS:                                              # k_sweep_minmax, k_sweep_pred, k_sweep_tp
        got[model] = check_sweep(users, ALL_SONGS, ctx, model, "aggregation", params)
        check_sweep(users, ALL_SONGS, ctx, model, "stochastic", [0.37, 0.9], SEEDS[0])
    took = [int(got["indicator"]["f64"][2][j, 0, :, 0].sum()) for j in range(len(thr))]   # indicator: users that took ibm
    assert took == [int(((ctx.idx >= 0) & (ctx.idx < t)).sum()) if 0 < t - ctx.pair_base < (ctx.idx >= 0).sum()
                    else 0 for t in thr]     # (none or all take ibm: the range is degenerate, nothing passes)
    assert len(set(took[:3])) == 3           # one pair more per threshold across the crossing


# ---------------------------------------------------------------------------
# models that are finite at heard songs: the masks the kernels form themselves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("users,shard", [(FULL, ALL_SONGS), (FULL, (2045, 4500)), (FULL, (255, 256)),
                                         (FULL, (2048, 4096)), ((7, 16), ALL_SONGS), ((0, 6), ALL_SONGS)])
def test_finite_at_heard(users, shard):
    """Aggregation and stochastic outputs are NaN exactly at heard songs
    (k_combine / k_combine3 mask them); linear keeps them. The sweep forms the
    value mr_combine_device would store, so its extremes, counts and mAP are
    those of the materialised output — for linear the heard positions count."""
    ctx = ctx_of(users, shard)
    agg = agg_params(ctx, 5) + [1.0]   # at 1.0 every pair takes ibm: an unmasked heard song would count
    cases = ([("linear", 0.5, 0), ("linear", 1.0, 0)] + [("aggregation", p, 0) for p in agg]
             + [("stochastic", p, SEEDS[0]) for p in (0.37, 1.0)])
    for model in MODELS:
        outs = check_materialised(users, shard, ctx, model, cases, nan_at_heard=False)
        check_combine_all(users, shard, ctx, model, 0.5, agg[0], 0.37, SEEDS[0], nan_at_heard=False)
        by_kind = {"linear": [1.0, 0.5], "aggregation": agg, "stochastic": [0.37, 1.0]}
        for kind, params in by_kind.items():
            got = check_sweep(users, shard, ctx, model, kind, params, SEEDS[0], nan_at_heard=False)
            for dtype in DTYPES:   # device against device: the sweep and the materialised path agree
                d = dev(users, shard, dtype)
                mn, mx, block = got[dtype]
                for j, p in enumerate(params):
                    o, _x, ext = outs[dtype][cases.index((kind, p, 0 if kind != "stochastic" else SEEDS[0]))]
                    assert (mn[j], mx[j]) == ext, (dtype, kind, p)
                    pred, tp = d.counts(o, *ext)
                    assert np.array_equal(block[j], block_of(ctx, pred, tp)), (dtype, model, kind, p)
    # linear: the heard positions count (selector values there are finite and pass levels)
    ubm, ibm = pl.selector(ctx, nan_at_heard=False)
    x = pl.restate(ctx, "linear", ubm, ibm, 0.5, "f64")
    pred, _tp = pl.counts(ctx, x, *pl.extremes(x))
    masked = np.where(ctx.heard, np.nan, x)
    pred_m, _tp_m = pl.counts(ctx, masked, *pl.extremes(x))
    assert pred.sum() > pred_m.sum()


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
VALUE_CONTEXTS = [(FULL, s) for s in pl.SHARDS] + [(u, ALL_SONGS) for u in pl.USER_BLOCKS + pl.SINGLE_USERS]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["negative", "mixed", "boundary", "denormal", "plus_inf", "minus_inf", "empty"])
def test_values(name, dtype):
    """Min / max, counts, the device AP fold and the sweep's linear kind at 1.0
    (x * 1.0 + 0 * 0.0: x itself) against the fp64 expression of MR:529 in
    numpy, on every context."""
    for users, shard in VALUE_CONTEXTS:
        ctx = ctx_of(users, shard)
        d = dev(users, shard, dtype)
        x = pl.value_models(ctx, dtype)[name]
        x64 = x.astype(np.float64)
        what = (name, dtype, users, shard)
        ext = pl.extremes(x64)
        n_valid = int((~np.isnan(x64)).sum())
        if name == "empty":
            assert ext == (np.inf, -np.inf)
        elif name == "plus_inf" and n_valid > 1:
            assert ext[1] == np.inf and np.isfinite(ext[0])
        elif name == "minus_inf" and n_valid > 1:
            assert ext[0] == -np.inf and np.isfinite(ext[1])
        x_t = d.up(x)
        zero = np.zeros(ctx.shape)
        zero[ctx.heard] = np.nan
        z_t = d.up(zero)
        assert d.e.eval_minmax(x_t.data_ptr()) == ext, what
        smn, smx = d.sweep_minmax(ctx, "linear", x_t, z_t, [1.0])
        assert (smn[0], smx[0]) == ext, what
        for n_thr in (10, 11):
            pred, tp = pl.counts(ctx, x64, *ext, n_thr)
            if name in ("plus_inf", "minus_inf", "empty"):
                assert not pred.any() and not tp.any(), what   # as the expression gives
            if name == "denormal" and n_valid > 2:
                assert pred.any(), what                        # a flushed-to-zero reading would count nothing
            got_p, got_t = d.counts(x_t, *ext, n_thr)
            assert np.array_equal(got_p, pred) and np.array_equal(got_t, tp), what + (n_thr,)
            block = d.sweep_counts(ctx, "linear", x_t, z_t, [1.0], [ext[0]], [ext[1]], n_thr=n_thr)
            assert np.array_equal(block[0], block_of(ctx, pred, tp)), what + (n_thr,)
            if d.full_width and name != "empty":
                exp = pl.mean_ap(ctx, pred, tp)
                assert d.eval_map(x_t, *ext, n_thr) == exp, what + (n_thr,)
                maps, mm = d.sweep_map(ctx, "linear", x_t, z_t, [1.0], n_thr=n_thr)
                assert maps == [exp] and (mm[0, 0], mm[0, 1]) == ext, what + (n_thr,)
        if d.full_width and name == "empty":
            with pytest.raises(_lib.EngineError, match=r"parameter 0 \(1\)") as err:
                d.sweep_map(ctx, "linear", x_t, z_t, [1.0])
            assert err.value.code == _lib.MR_E_INVALID
