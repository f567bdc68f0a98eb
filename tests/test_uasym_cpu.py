"""The asymmetric-cosine, locality-q user-based model on the host:
evaluation.asym_user_model — the numpy twin mr_ubm_asym_device is compared
against — against an independent brute force over Python sets with the same
scalar operations, against the fixed-point oracle's UserBasedModel at (0.5, 1),
column slice by column slice and row by row; the resolution of the fixed-point
keys as inequalities; the --asym-user front end, the twin's and the library's
argument checks that need no GPU. Every comparison is bitwise."""
import ctypes
import math

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation
from oracle import native

from helpers import dataset_from_lines, kat, synth_fixture

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

GRID = [(0.5, 1), (0.15, 3), (0.0, 1), (1.0, 2), (0.85, 8)]
_ds = {}


def dataset(name):
    if name not in _ds:
        if name == "small":
            _ds[name] = synth_fixture("small")[0]
        else:
            K = kat() if name == "kat" else kat()["dup"]
            _ds[name] = dataset_from_lines(K["train"], K["test"], K["labels"])
    return _ds[name]


def same_bits(a, b):
    """NaN in the same places, every other value bit-equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


def brute_force(train, test, ds, alpha, q, F):
    """score(u, s) straight from the lines: histories as Python sets, lengths
    as line counts, the tables of the three exact cases by hand (the general
    case reads the library's, as the contract says), one scalar operation at a
    time, Python integers for the sums."""
    S, tr_len = {}, {}
    for line in train:
        v, s, _ = line.split("\t")
        S.setdefault(v, set()).add(s)
        tr_len[v] = tr_len.get(v, 0) + 1
    T, te_len = {}, {}
    for line in test:
        u, s, _ = line.split("\t")
        T.setdefault(u, set()).add(s)
        te_len[u] = te_len.get(u, 0) + 1
    songs = [ds.song_names(i) for i in range(ds.n_songs)]
    tests = [ds.test_names(i) for i in range(ds.n_test)]
    trains = [ds.train_names(i) for i in range(ds.n_train)]
    assert [te_len[u] for u in tests] == np.asarray(ds.te_len).tolist()
    assert [tr_len[v] for v in trains] == np.asarray(ds.tr_len).tolist()
    if alpha == 0.5:
        pa = {u: math.sqrt(float(te_len[u])) for u in tests}
        pb = {v: math.sqrt(float(tr_len[v])) for v in trains}
    elif alpha == 0.0:
        pa, pb = {u: 1.0 for u in tests}, {v: float(tr_len[v]) for v in trains}
    elif alpha == 1.0:
        pa, pb = {u: float(te_len[u]) for u in tests}, {v: 1.0 for v in trains}
    else:
        pa = dict(zip(tests, evaluation.asym_tables(alpha, ds.te_len)[0].tolist()))
        pb = dict(zip(trains, evaluation.asym_tables(alpha, ds.tr_len)[1].tolist()))
    two_f, inv_f = math.ldexp(1.0, F), math.ldexp(1.0, -F)
    out = np.empty((ds.n_test, ds.n_songs))
    n_keys = 0
    for ui, u in enumerate(tests):
        key = {}
        for v in trains:
            y = len(T[u] & S[v])
            if y == 0:
                continue
            den = pa[u] * pb[v]
            w = float(y) / den if den != 0.0 else 0.0
            t = w
            for _ in range(q - 1):
                t = t * w
            key[v] = int(np.rint(np.float64(t * two_f)))  # round-half-even
            n_keys += 1
        for si, s in enumerate(songs):
            if s in T[u]:
                out[ui, si] = np.nan
                continue
            acc = sum(k for v, k in key.items() if s in S[v])  # a Python integer: exact
            assert -2 ** 63 <= acc < 2 ** 63
            out[ui, si] = float(np.float64(np.int64(acc))) * inv_f
    assert n_keys > 0
    return out


@pytest.mark.parametrize("F", [32, 52])
@pytest.mark.parametrize("variant", ["kat", "kat_dup"])
@pytest.mark.parametrize("alpha,q", GRID)
def test_twin_equals_the_brute_force_bitwise(variant, alpha, q, F):
    K = kat() if variant == "kat" else kat()["dup"]
    ds = dataset(variant)
    twin = evaluation.asym_user_model(ds, alpha, q, F)
    assert twin.dtype == np.float64 and twin.shape == (ds.n_test, ds.n_songs)
    assert same_bits(twin, brute_force(K["train"], K["test"], ds, alpha, q, F))
    assert np.array_equal(np.isnan(twin), ds.heard_mask())
    assert np.count_nonzero(np.nan_to_num(twin)) > 0 and not (np.nan_to_num(twin) < 0).any()


def test_the_duplicate_line_variant_has_lengths_above_the_distinct_counts():
    ds = dataset("kat_dup")  # so that te_len / tr_len, not the CSR degrees, are what the tables read
    assert (np.asarray(ds.tr_len) > np.diff(ds.tr_off)).any() or (np.asarray(ds.te_len) > np.diff(ds.te_off)).any()


@pytest.mark.parametrize("F", [8, 32, 40])
@pytest.mark.parametrize("name", ["kat", "kat_dup", "small"])
def test_twin_at_half_one_is_the_fixed_point_user_based_model(name, F):
    ds = dataset(name)
    twin = evaluation.asym_user_model(ds, 0.5, 1, F)
    fp = native.fp_model(ds, "ubm", frac_bits=F)[0]
    assert same_bits(twin, fp) and np.count_nonzero(np.nan_to_num(twin)) > 0


@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3)])
def test_column_slices_and_rows(alpha, q):
    ds = dataset("small")
    full = evaluation.asym_user_model(ds, alpha, q, 40)
    n = ds.n_songs
    for lo, hi in ((0, 333), (333, 900), (900, n), (7, 7)):
        assert same_bits(evaluation.asym_user_model(ds, alpha, q, 40, song_lo=lo, song_hi=hi), full[:, lo:hi])
    some = [ds.n_test - 1, 0, 0]
    assert same_bits(evaluation.asym_user_model(ds, alpha, q, 40, users=some), full[some])
    assert same_bits(evaluation.asym_user_model(ds, alpha, q, 40, song_lo=5, song_hi=n - 5, users=some),
                     full[some][:, 5:n - 5])
    keys = evaluation.asym_user_keys(ds, alpha, q, 40)
    part = evaluation.asym_user_keys(ds, alpha, q, 40, users=some)
    for (v, k), u in zip(part, some):
        assert np.array_equal(v, keys[u][0]) and np.array_equal(k, keys[u][1]) and k.dtype == np.int64


def test_resolution_terms_below_half_an_ulp_of_the_fixed_point_vanish():
    """At q = 8 small weights fall below 2^-(F+1) and round to key 0: the count
    of such neighbours does not grow with F and is 0 at F = 52."""
    ds = dataset("small")
    for alpha in (0.5, 0.85):
        zeros = []
        for F in (32, 40, 52):
            keys = evaluation.asym_user_keys(ds, alpha, 8, F)
            assert sum(len(k) for _v, k in keys) > 0 and all((k >= 0).all() for _v, k in keys)
            zeros.append(sum(int((k == 0).sum()) for _v, k in keys))
        print(f"alpha {alpha} q 8: neighbours with key 0 at F = 32, 40, 52: {zeros}")
        assert zeros[0] >= zeros[1] >= zeros[2] == 0


def test_twin_argument_checks():
    ds = dataset("kat")
    for kw in (dict(q=0), dict(q=9), dict(frac_bits=7), dict(frac_bits=53), dict(song_lo=5, song_hi=4),
               dict(song_hi=ds.n_songs + 1), dict(alpha=1.5), dict(alpha=float("nan"))):
        args = dict(alpha=0.5, q=1, frac_bits=32)
        args.update(kw)
        with pytest.raises((ValueError, _lib.EngineError)):
            evaluation.asym_user_model(ds, **args)


def test_asym_user_option_parsing():
    assert driver.parse_asym_user("0.3:2") == (0.3, 2, None) and driver.parse_asym_user("0.3:2:40") == (0.3, 2, 40)
    assert driver.parse_asym_user((0.5, 1)) == (0.5, 1, None) and driver.parse_asym_user((0.5, 1, 52)) == (0.5, 1, 52)
    assert driver.parse_asym_user("0:1:8") == (0.0, 1, 8) and driver.parse_asym_user("1:8:52") == (1.0, 8, 52)
    for bad in ("0.5", "0.5:", ":2", "x:2", "0.5:y", "-0.1:2", "1.1:2", "nan:2", "0.5:0", "0.5:9", "0.5:1.5", "",
                "0.5:1:7", "0.5:1:53", "0.5:1:x", "0.5:1:", "0.5:1:40:2"):
        with pytest.raises(ValueError, match="--asym-user"):
            driver.parse_asym_user(bad)
    with pytest.raises(SystemExit):
        driver.main(["10", "2", "--asym-user", "0.5:1:60"])


def test_driver_passes_asym_user_through(monkeypatch):
    seen = {}
    monkeypatch.setattr(driver, "run", lambda *a, **kw: seen.update(kw) or {})
    driver.main(["50", "5", "--asym-user", "0.3:2:40", "--asym", "0.15:3"])
    assert seen["asym_user"] == (0.3, 2, 40) and seen["asym"] == (0.15, 3)
    driver.main(["50", "5"])
    assert seen["asym_user"] is None and seen["asym"] is None


def test_library_rejects_bad_arguments_without_a_gpu():
    """The documented order: NULL ctx, alpha, q, frac_bits, NULL dense_dev, then
    the context's state — so a handle that is never dereferenced serves for the
    argument checks where no context can be created."""
    L = _lib.lib()
    assert "mr_ubm_asym_device" in _lib.SIGNATURES
    buf = np.zeros(8, dtype=np.float64)
    assert L.mr_ubm_asym_device(None, 0.5, 1, 0, P(buf)) == _lib.MR_E_INVALID
    assert b"context" in L.mr_last_error()
    fake = np.zeros(64, dtype=np.int64)
    for alpha in (-0.1, 1.1, float("nan")):
        assert L.mr_ubm_asym_device(P(fake), alpha, 1, 0, P(buf)) == _lib.MR_E_INVALID
        assert b"alpha" in L.mr_last_error()
    for q in (0, 9, -3):
        assert L.mr_ubm_asym_device(P(fake), 0.5, q, 0, P(buf)) == _lib.MR_E_INVALID
        assert b"q=" in L.mr_last_error()
    for F in (-1, 1, 7, 53, 64):
        assert L.mr_ubm_asym_device(P(fake), 0.5, 1, F, P(buf)) == _lib.MR_E_INVALID
        assert b"frac_bits" in L.mr_last_error()
    for F in (0, 8, 52):
        assert L.mr_ubm_asym_device(P(fake), 0.5, 1, F, None) == _lib.MR_E_INVALID
        assert b"dense_dev" in L.mr_last_error()
    assert not fake.any() and not buf.any()
    opt = _lib.MrOptions()
    assert L.mr_options_default(ctypes.byref(opt)) == _lib.MR_OK
    h = ctypes.c_void_p()
    if L.mr_create(ctypes.byref(opt), ctypes.byref(h)) != _lib.MR_OK:
        return  # no device to create a context on: the checks above are all that runs here
    try:
        assert L.mr_ubm_asym_device(h, 0.5, 1, 53, P(buf)) == _lib.MR_E_INVALID
        assert L.mr_ubm_asym_device(h, 0.5, 1, 0, P(buf)) == _lib.MR_E_STATE  # before mr_load
        assert not buf.any()
    finally:
        L.mr_destroy(h)
