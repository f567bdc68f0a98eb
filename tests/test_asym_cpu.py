"""The asymmetric-cosine, locality-q item-based model on the host: the
library's host-only mr_asym_tables (exact special cases, the general case
against np.power, argument checks); evaluation.asym_item_model — the numpy twin
mr_ibm_asym_device is compared against — against an independent brute force
over Python sets, against the sequential fold of evaluation.song_similarity's
rows at (0.5, 1), and column slice by column slice; the --asym front end and
the library's argument checks that need no GPU."""
import ctypes
import math

import numpy as np
import pytest

from musicrecommendation_amd import _lib, driver, evaluation

from helpers import dataset_from_lines, kat, synth_fixture

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """NaN in the same places, every other value bit-equal."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return np.array_equal(bits(a[ok]), bits(b[ok]))


def tables(alpha, counts):
    c = np.ascontiguousarray(counts, dtype=np.int32)
    pa, pb = np.full(c.size, -1.0), np.full(c.size, -1.0)
    assert _lib.lib().mr_asym_tables(alpha, c.size, P(c), P(pa), P(pb)) == _lib.MR_OK
    return pa, pb


COUNTS = np.array([0, 1, 2, 3, 4, 5, 7, 9, 10, 16, 17, 100, 999, 5000, 5001, 65536, 131071, 1 << 20, 48373586, 2 ** 31 - 1],
                  dtype=np.int32)


def test_tables_special_cases_are_exact():
    cd = COUNTS.astype(np.float64)
    pa, pb = tables(0.5, COUNTS)
    assert np.array_equal(bits(pa), bits(np.sqrt(cd))) and np.array_equal(bits(pb), bits(np.sqrt(cd)))
    pa, pb = tables(0.0, COUNTS)
    assert np.array_equal(bits(pa), bits(np.ones_like(cd))) and np.array_equal(bits(pb), bits(cd))
    pa, pb = tables(1.0, COUNTS)
    assert np.array_equal(bits(pa), bits(cd)) and np.array_equal(bits(pb), bits(np.ones_like(cd)))
    a, b = evaluation.asym_tables(0.5, COUNTS)  # the twin's accessor hands out the same values
    assert np.array_equal(bits(a), bits(np.sqrt(cd))) and np.array_equal(bits(b), bits(np.sqrt(cd)))


@pytest.mark.parametrize("alpha", [0.15, 0.25, 0.85, 1.0 / 3.0, 0.999])
def test_tables_general_case_is_within_4_ulp_of_numpy(alpha):
    """A sanity bound on libm, not a parity claim: the twin and the device both
    read the library's tables."""
    cd = COUNTS.astype(np.float64)
    pa, pb = tables(alpha, COUNTS)
    for got, exp in ((pa, np.power(cd, alpha)), (pb, np.power(cd, 1.0 - alpha))):
        ulp = np.abs(got - exp) / np.spacing(np.abs(exp))
        print(f"alpha={alpha}: max {ulp.max()} ulp")
        assert (ulp <= 4).all()
    assert pa[0] == 0.0 and pb[0] == 0.0 and pa[1] == 1.0 and pb[1] == 1.0


def test_tables_reject_bad_arguments():
    L = _lib.lib()
    c = np.ones(3, dtype=np.int32)
    pa, pb = np.full(3, -1.0), np.full(3, -1.0)
    assert L.mr_asym_tables(0.3, 3, None, P(pa), P(pb)) == _lib.MR_E_INVALID
    assert L.mr_asym_tables(0.3, 3, P(c), None, P(pb)) == _lib.MR_E_INVALID
    assert L.mr_asym_tables(0.3, 3, P(c), P(pa), None) == _lib.MR_E_INVALID
    assert L.mr_asym_tables(0.3, -1, P(c), P(pa), P(pb)) == _lib.MR_E_INVALID
    assert L.mr_last_error()
    for alpha in (-0.1, 1.1, float("nan")):
        assert L.mr_asym_tables(alpha, 3, P(c), P(pa), P(pb)) == _lib.MR_E_INVALID
    assert (pa == -1.0).all() and (pb == -1.0).all()  # nothing written
    assert L.mr_asym_tables(0.3, 0, P(c), P(pa), P(pb)) == _lib.MR_OK and (pa == -1.0).all()


def brute_force(train, test, ds, alpha, q):
    """score(u, s) straight from the lines: listeners as Python sets, the
    tables of the three exact cases by hand (the general case reads the
    library's, as the contract says), a sequential Python fold."""
    listeners, count = {}, {}
    for line in train:
        u, s, _ = line.split("\t")
        listeners.setdefault(s, set()).add(u)
        count[s] = count.get(s, 0) + 1
    heard = {}
    for line in test:
        u, s, _ = line.split("\t")
        heard.setdefault(u, set()).add(s)
        count[s] = count.get(s, 0) + 1
    names = [ds.song_names(i) for i in range(ds.n_songs)]
    assert sorted(count) == names and [count[n] for n in names] == np.asarray(ds.song_count).tolist()
    if alpha == 0.5:
        pa = pb = {n: math.sqrt(float(count[n])) for n in names}
    elif alpha == 0.0:
        pa, pb = {n: 1.0 for n in names}, {n: float(count[n]) for n in names}
    elif alpha == 1.0:
        pa, pb = {n: float(count[n]) for n in names}, {n: 1.0 for n in names}
    else:
        ta, tb = evaluation.asym_tables(alpha, ds.song_count)
        pa, pb = dict(zip(names, ta.tolist())), dict(zip(names, tb.tolist()))
    out = np.empty((ds.n_test, ds.n_songs))
    for ui in range(ds.n_test):
        mine = heard[ds.test_names(ui)]
        for si, s in enumerate(names):
            if s in mine:
                out[ui, si] = np.nan
                continue
            acc = 0.0
            for s2 in sorted(mine):  # names sort as their ids do
                c = len(listeners.get(s, set()) & listeners.get(s2, set()))
                den = pa[s] * pb[s2]
                w = float(c) / den if den != 0.0 else 0.0
                t = w
                for _ in range(q - 1):
                    t = t * w
                acc = acc + t
            out[ui, si] = acc
    return out


@pytest.mark.parametrize("variant", ["kat", "kat_dup"])
@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3), (0.0, 1), (1.0, 2)])
def test_twin_equals_the_brute_force_bitwise(variant, alpha, q):
    K = kat() if variant == "kat" else kat()["dup"]
    ds = dataset_from_lines(K["train"], K["test"], K["labels"])
    twin = evaluation.asym_item_model(ds, alpha, q)
    assert twin.dtype == np.float64 and twin.shape == (ds.n_test, ds.n_songs)
    exp = brute_force(K["train"], K["test"], ds, alpha, q)
    assert same_bits(twin, exp)
    assert np.array_equal(np.isnan(twin), ds.heard_mask())
    assert np.count_nonzero(np.nan_to_num(twin)) > 0 and not (np.nan_to_num(twin) < 0).any()


def similarity_fold(ds, rows_of, lo=0, hi=None):
    """The NumPy left fold, ascending s2, of similar-song rows over T(u)."""
    hi = ds.n_songs if hi is None else hi
    out = np.empty((ds.n_test, hi - lo))
    for u in range(ds.n_test):
        mine = np.sort(np.asarray(ds.te_songs[ds.te_off[u]:ds.te_off[u + 1]]))
        acc = np.zeros(hi - lo)
        for s2 in mine.tolist():
            acc = acc + np.nan_to_num(rows_of(s2))  # the row's own NaN (s == s2) is a heard column
        acc[mine[(mine >= lo) & (mine < hi)] - lo] = np.nan
        out[u] = acc
    return out


def test_twin_at_half_one_is_the_fold_of_the_similarity_rows():
    ds, _ = synth_fixture("small")
    q = np.unique(ds.te_songs)
    rows = evaluation.song_similarity(ds, q)
    at = {int(s): i for i, s in enumerate(q)}
    exp = similarity_fold(ds, lambda s2: rows[at[s2]])
    twin = evaluation.asym_item_model(ds, 0.5, 1)
    assert same_bits(twin, exp) and np.count_nonzero(np.nan_to_num(twin)) > 0


@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3)])
def test_column_slices_equal_the_twin_of_that_range(alpha, q):
    ds, _ = synth_fixture("small")
    full = evaluation.asym_item_model(ds, alpha, q)
    n = ds.n_songs
    for lo, hi in ((0, 333), (333, 900), (900, n), (7, 7)):
        assert same_bits(evaluation.asym_item_model(ds, alpha, q, song_lo=lo, song_hi=hi), full[:, lo:hi])
    some = [ds.n_test - 1, 0, 0]
    assert same_bits(evaluation.asym_item_model(ds, alpha, q, song_lo=5, song_hi=n - 5, users=some), full[some][:, 5:n - 5])
    with pytest.raises(ValueError):
        evaluation.asym_item_model(ds, alpha, q, song_lo=5, song_hi=4)
    with pytest.raises(ValueError):
        evaluation.asym_item_model(ds, alpha, 9)


def test_asym_option_parsing():
    assert driver.parse_asym("0.15:3") == (0.15, 3) and driver.parse_asym((0.5, 1)) == (0.5, 1)
    assert driver.parse_asym("0:1") == (0.0, 1) and driver.parse_asym("1:8") == (1.0, 8)
    for bad in ("0.5", "0.5:", ":2", "x:2", "0.5:y", "-0.1:2", "1.1:2", "nan:2", "0.5:0", "0.5:9", "0.5:1.5", ""):
        with pytest.raises(ValueError, match="--asym"):
            driver.parse_asym(bad)
    with pytest.raises(SystemExit):
        driver.main(["10", "2", "--asym", "0.5:9"])


def test_driver_passes_asym_through(monkeypatch):
    seen = {}
    monkeypatch.setattr(driver, "run", lambda *a, **kw: seen.update(kw) or {})
    driver.main(["50", "5", "--asym", "0.15:3", "--recommend", "20"])
    assert seen["asym"] == (0.15, 3) and seen["recommend"] == (20, None)
    driver.main(["50", "5"])
    assert seen["asym"] is None


def test_library_rejects_bad_arguments_without_a_gpu():
    """The documented order: NULL ctx, alpha, q, NULL dense_dev, then the
    context's state — so a handle that is never dereferenced serves for the
    argument checks where no context can be created."""
    L = _lib.lib()
    assert _lib.MR_ASYM_MAX_Q == 8 and {"mr_asym_tables", "mr_ibm_asym_device"} <= set(_lib.SIGNATURES)
    buf = np.zeros(8, dtype=np.float64)
    assert L.mr_ibm_asym_device(None, 0.5, 1, P(buf)) == _lib.MR_E_INVALID
    assert b"context" in L.mr_last_error()
    fake = np.zeros(64, dtype=np.int64)
    for alpha in (-0.1, 1.1, float("nan")):
        assert L.mr_ibm_asym_device(P(fake), alpha, 1, P(buf)) == _lib.MR_E_INVALID
        assert b"alpha" in L.mr_last_error()
    for q in (0, 9, -3):
        assert L.mr_ibm_asym_device(P(fake), 0.5, q, P(buf)) == _lib.MR_E_INVALID
        assert b"q=" in L.mr_last_error()
    assert L.mr_ibm_asym_device(P(fake), 0.5, 1, None) == _lib.MR_E_INVALID
    assert b"dense_dev" in L.mr_last_error()
    assert not fake.any() and not buf.any()
    opt = _lib.MrOptions()
    assert L.mr_options_default(ctypes.byref(opt)) == _lib.MR_OK
    h = ctypes.c_void_p()
    if L.mr_create(ctypes.byref(opt), ctypes.byref(h)) != _lib.MR_OK:
        return  # no device to create a context on: the checks above are all that runs here
    try:
        assert L.mr_ibm_asym_device(h, 1.5, 1, P(buf)) == _lib.MR_E_INVALID
        assert L.mr_ibm_asym_device(h, 0.5, 0, P(buf)) == _lib.MR_E_INVALID
        assert L.mr_ibm_asym_device(h, 0.5, 1, None) == _lib.MR_E_INVALID
        assert L.mr_ibm_asym_device(h, 0.5, 1, P(buf)) == _lib.MR_E_STATE  # before mr_load
        assert not buf.any()
    finally:
        L.mr_destroy(h)
