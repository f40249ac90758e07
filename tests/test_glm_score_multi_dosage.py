"""pgh_glm_score_multi_dosage / Dataset.glm_score_multi_dosage: the dense logistic score test over a dataset that holds
dosage tracks.  A variant's genotype value is the explicit dosage / 16384 where a sample has one and its call
otherwise (pgh_glm's rule); a sample with neither is missing.  Every row is checked against the FP64 oracle of the
score tests (tests/glm_score_oracle.py, which takes real-valued x with -9 = missing) within test_glm_score_sparse's
1e-9 on check_rows' scale; obs_ct, a1_freq and the count decisions equal pgh_glm's logistic fit over the same file bit
for bit; a variant without a track and a variant whose track restates its calls equal pgh_glm_score_multi's row for the
same calls bit for bit; and a row does not depend on the other phenotypes, the range, the window, the blocks, the
chunks, the scratch budget or the tracks of its neighbours."""

import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_score_oracle as O
import pgen_writer as W
import subset_shapes as SS
from test_dosage_tracks import make_dosage_file

NAN = float("nan")
NAME = "pgh_glm_score_multi_dosage"
REL = 1e-9  # test_glm_score_sparse.REL
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
NONE = 0xFFFF
# make_dosage_file(path, m, n, seed, False): all three track shapes and track-less variants, presence rates 0 to 1;
# one 64-sample word of the presence bits and ranks, many words, and the 4,096-sample step of the correction kernel
MIXED = ((120, 257, 31), (80, 1003, 32), (60, 4099, 33))
MIXED_FULL_TRACKS = {257: 18, 1003: 13, 4099: 9}  # tracks with a dosage for every sample
KS = (0, 1, 3, 20)
# (case rate, NaN rate) of the five phenotypes (test_glm_score_multi.PHENO_SPECS)
PHENO_SPECS = ((0.2, 0.03), (0.5, 0.0), (0.05, 0.1), (0.35, 0.03), (0.1, 0.3))
# sample counts at and next to a 64-sample edge: the presence and rank words, the u16 row's padding, the mask's tail
EDGE_N = (63, 64, 65, 128)
EDGE_K = (0, 2)
EDGE_M = 80
EDGE_SPECS = ((0.5, 0.03), (0.35, 0.03))
# (k, what 17 phenotypes of k + 2 x-columns each do to the 16-column blocks): test_glm_score_multi.LAYOUTS
LAYOUTS = [(14, "a phenotype is one block"), (13, "every phenotype after the first straddles a block edge")]
LAYOUT_PHENOTYPES = 17
LAYOUT_N = 1003


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_symbol(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    assert f"{NAME}(" in header
    assert NAME in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.raw(), NAME)
    assert hasattr(lib.Dataset, "glm_score_multi_dosage")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_arrays_of_the_wrong_shape_are_rejected(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi_dosage(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi_dosage(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def test_a_null_dataset_is_refused_with_out_untouched(lib):
    out = np.full(lib.GLM_ROW_DTYPE.itemsize * 4, 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    rc = getattr(lib.raw(), NAME)(None, None, 0, 4, 1, y.ctypes.data_as(C.c_void_p), 0, None,
                                  out.ctypes.data_as(C.c_void_p), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and (out == 0xAB).all()


# ---- helpers -----------------------------------------------------------------------------------------------------

def _covariates(rng, k, n):
    """test_glm_score_sparse._covariates"""
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def _phenotypes(rng, n, Z, specs=PHENO_SPECS):
    return np.stack([O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in specs])


def _six(rng, n, Z):
    """test_glm_score_multi._phenotypes: the five and a sixth that shares the first one's NaN pattern."""
    ys = _phenotypes(rng, n, Z)
    shared = O.pheno(rng, n, Z, case_rate=0.3, missing=0.0)
    shared[np.isnan(ys[0])] = NAN
    return np.concatenate([ys, shared[None, :]])


def _col(out, p, rows=slice(None)):
    return {key: v[rows, p] for key, v in out.items()}


def _rows(out, rows):
    return {key: v[rows] for key, v in out.items()}


def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _counts_equal_the_dense_logistic_fit(got, want, ctx=None):
    """test_glm_score_sparse._counts_equal_the_dense_logistic_fit"""
    assert got["obs_ct"].tolist() == want["obs_ct"].tolist(), ctx
    assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True), ctx
    for code in ("TOO_FEW_SAMPLES", "CONST_ALLELE"):
        assert (got["errcode"] == code).tolist() == (want["errcode"] == code).tolist(), (code, ctx)
    assert not got["firth"].any(), ctx


def _values(geno, dos):
    """make_dosage_file's `want`: the value rows, -9.0 = neither a dosage nor a call."""
    return np.where(dos != NONE, dos.astype(np.float64) / 16384.0, np.where(geno == 3, -9.0, geno.astype(np.float64)))


def mixed_inputs(n, k):
    """(Z, Y) of the parity cases: the covariates and the five phenotypes from one generator, in that order."""
    rng = np.random.default_rng(1000 + k)
    Z = _covariates(rng, k, n)
    return Z, _phenotypes(rng, n, Z)


@functools.lru_cache(maxsize=None)
def edge_inputs(n, k):
    """test_glm_score_multi.edge_inputs"""
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    return Z, _phenotypes(rng, n, Z, specs=EDGE_SPECS)


@functools.lru_cache(maxsize=None)
def layout_inputs(k):
    """(Z, Y): six phenotypes in turn at positions 0..15, and at 16 one of its own (test_glm_score_multi.layout_inputs)."""
    rng = np.random.default_rng(100 * LAYOUT_N + k)
    Z = _covariates(rng, k, LAYOUT_N)
    six = _six(rng, LAYOUT_N, Z)
    own = O.pheno(np.random.default_rng(17_000 + k), LAYOUT_N, Z, case_rate=0.25, missing=0.05)
    return Z, np.stack([six[i % len(six)] for i in range(LAYOUT_PHENOTYPES - 1)] + [own])


class _Case:
    """One written file: its calls, its dosages (0xFFFF = none), the track kinds and the value rows."""

    def __init__(self, path, geno, dos, dkinds):
        self.path, self.geno, self.dos, self.dkinds = path, geno, dos, list(dkinds)
        self.m, self.n = geno.shape
        self.x = _values(geno, dos)
        self.track = np.array([kind != 0 for kind in dkinds])
        self.full = self.track & (dos != NONE).all(axis=1)
        self.ds = None

    def open(self, L, **kw):
        if kw:
            return L.Dataset.open(self.path, **kw)
        if self.ds is None:
            self.ds = L.Dataset.open(self.path)
        return self.ds


def _mixed_case(tmp, m, n, seed):
    path = str(tmp / f"mixed_{n}.pgen")
    geno, dos, dkinds, want = make_dosage_file(path, m, n, seed, False)
    case = _Case(path, geno, dos, dkinds)
    assert np.array_equal(case.x, want)
    return case


MADE_N = 257
MADE_ROWS = ("constant 4915", "two values", "one entry", "no entry", "entries outside S", "entries cover the missing calls",
             "all missing, no track", "all missing, empty track", "all missing, full track", "ordinary")


def made_nan_samples():
    """The samples without a phenotype of the made file's phenotypes."""
    gone = np.zeros(MADE_N, dtype=bool)
    gone[[5, 63, 64, 130, 256]] = True
    return gone


def _made_case(tmp):
    """One of each of the rows that MADE_ROWS names, at n = 257."""
    n = MADE_N
    rng = np.random.default_rng(257)
    m = len(MADE_ROWS)
    geno = rng.choice(4, size=(m, n), p=[0.5, 0.3, 0.12, 0.08]).astype(np.uint8)
    dos = np.full((m, n), NONE, dtype=np.uint16)
    dkinds = [0] * m
    dos[0], dkinds[0] = 4915, 0x40
    dos[1], dkinds[1] = np.where(rng.random(n) < 0.4, 4915, 20000), 0x40
    dos[2, 77], dkinds[2] = 12345, 0x20
    dkinds[3] = 0x60
    dos[4, made_nan_samples()], dkinds[4] = 9000, 0x20
    cover = (geno[5] == 3) | (rng.random(n) < 0.1)
    dos[5, cover], dkinds[5] = rng.integers(0, 32769, int(cover.sum()), dtype=np.uint16), 0x60
    assert (geno[5] == 3).sum() > 5
    geno[6:9] = 3
    dkinds[7] = 0x20
    dos[8], dkinds[8] = rng.integers(0, 32769, n, dtype=np.uint16), 0x40
    hit = rng.random(n) < 0.3
    dos[9, hit], dkinds[9] = rng.integers(0, 32769, int(hit.sum()), dtype=np.uint16), 0x60
    path = str(tmp / "made.pgen")
    W.write_pgen(path, geno, [0] * m, dosage=dos, dosage_kinds=dkinds)
    return _Case(path, geno, dos, dkinds)


def made_inputs():
    """(Z, Y): two covariates and two phenotypes that share made_nan_samples()."""
    rng = np.random.default_rng(2570)
    Z = _covariates(rng, 2, MADE_N)
    Y = _phenotypes(rng, MADE_N, Z, specs=((0.4, 0.0), (0.25, 0.0)))
    Y[:, made_nan_samples()] = NAN
    return Z, Y


def _restated_case(tmp, n):
    """Calls with about 8 % missing and, on three of four variants, a track of each shape that restates them: value =
    16384 x call wherever there is a call, nothing elsewhere.  Also the same calls written without tracks."""
    m = 90
    geno = SS.hard_codes(n, m=m)
    dos = np.where(geno == 3, NONE, geno.astype(np.uint16) << 14).astype(np.uint16)
    dkinds = [(0, 0x20, 0x40, 0x60)[v % 4] for v in range(m)]
    kinds = W.choose_kinds(geno, np.random.default_rng(n))
    path = str(tmp / "restated.pgen")
    W.write_pgen(path, geno, kinds, dosage=dos, dosage_kinds=dkinds)
    hard = str(tmp / "restated_hard.pgen")
    W.write_pgen(hard, geno, kinds)
    dos[[kind == 0 for kind in dkinds]] = NONE
    return _Case(path, geno, dos, dkinds), hard


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Every input file of the module, written once (no device)."""
    tmp = tmp_path_factory.mktemp("glm_score_multi_dosage")
    out = {("mixed", n): _mixed_case(tmp, m, n, seed) for m, n, seed in MIXED}
    for n in EDGE_N:
        path = str(tmp / f"edge_{n}.pgen")
        geno, dos, dkinds, _ = make_dosage_file(path, EDGE_M, n, 640 + n, False)
        out["edge", n] = _Case(path, geno, dos, dkinds)
    out["made"] = _made_case(tmp)
    out["restated"], out["restated_hard"] = _restated_case(tmp, 1003)
    twin = str(tmp / "mixed_1003_hard.pgen")
    geno = out["mixed", 1003].geno
    W.write_pgen(twin, geno, W.choose_kinds(geno, np.random.default_rng(5)))
    out["mixed_hard"] = twin
    yield out
    for c in out.values():
        if isinstance(c, _Case) and c.ds is not None:
            c.ds.close()


# ---- no device: conditions on the inputs ------------------------------------------------------------------------

def test_the_mixed_files_hold_what_the_cases_need(cases):
    for m, n, seed in MIXED:
        c = cases["mixed", n]
        assert {0, 0x20, 0x40, 0x60} == set(c.dkinds)
        assert int(c.full.sum()) == MIXED_FULL_TRACKS[n]
        on_missing = ((c.dos != NONE) & (c.geno == 3)).any(axis=1)
        empty = c.track & (c.dos == NONE).all(axis=1)
        assert on_missing.sum() >= 20 and empty.sum() >= 10, (n, on_missing.sum(), empty.sum())
    for n in EDGE_N:
        c = cases["edge", n]
        assert c.track.sum() >= 40 and {0x20, 0x40, 0x60} <= set(c.dkinds)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_the_parity_inputs_have_fitted_rows(cases, n, k):
    """So that a run that decides everything by errcode cannot pass: per phenotype the oracle fits at least half of the
    track variants and every full track, and trips none of its own asserts."""
    c = cases["mixed", n]
    Z, Y = mixed_inputs(n, k)
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None, (n, k, p, nul.status)
        fitted = np.array([O.oracle_row(c.x[i], nul)["errcode"] is None for i in range(c.m)])
        assert 2 * fitted[c.track].sum() >= c.track.sum(), (n, k, p, fitted[c.track].sum(), c.track.sum())
        assert fitted[c.full].all(), (n, k, p)


def test_the_other_inputs_have_fitted_null_models_and_fitted_rows(cases):
    for n in EDGE_N:
        for k in EDGE_K:
            Z, Y = edge_inputs(n, k)
            for p, y in enumerate(Y):
                nul = O.Null(y, Z)
                assert nul.status is None, (n, k, p, nul.status)
                c = cases["edge", n]
                fitted = sum(O.oracle_row(c.x[i], nul)["errcode"] is None for i in range(c.m))
                assert fitted >= 20, (n, k, p, fitted)
    c = cases["mixed", LAYOUT_N]
    for k, _ in LAYOUTS:
        Z, Y = layout_inputs(k)
        assert len(set(y.tobytes() for y in Y)) == 7
        for p in (0, LAYOUT_PHENOTYPES - 2, LAYOUT_PHENOTYPES - 1):
            nul = O.Null(Y[p], Z)
            assert nul.status is None, (k, p, nul.status)
            fitted = np.array([O.oracle_row(c.x[i], nul)["errcode"] is None for i in range(c.m)])
            assert 2 * fitted[c.track].sum() >= c.track.sum(), (k, p)
    Z, Y = made_inputs()
    want = {"constant 4915": "CONST_ALLELE", "two values": None, "all missing, no track": "TOO_FEW_SAMPLES",
            "all missing, empty track": "TOO_FEW_SAMPLES", "all missing, full track": None, "ordinary": None}
    c = cases["made"]
    for y in Y:
        nul = O.Null(y, Z)
        assert nul.status is None and np.array_equal(np.isnan(y), made_nan_samples())
        for name, code in want.items():
            assert O.oracle_row(c.x[MADE_ROWS.index(name)], nul)["errcode"] == code, name
    # M is empty while code 3 is present; the entries outside S change nothing that S sees
    row = MADE_ROWS.index("entries cover the missing calls")
    assert (c.geno[row] == 3).any() and not (c.x[row] == -9.0).any()
    row = MADE_ROWS.index("entries outside S")
    assert (c.dos[row] != NONE).sum() == made_nan_samples().sum() and (c.dos[row][~made_nan_samples()] == NONE).all()


# ---- on the GPU --------------------------------------------------------------------------------------------------

_RESULTS = {}


def _mixed_result(L, cases, n, k):
    """The new entry's rows over a mixed file, computed once per (n, k) for the tests that share them."""
    if (n, k) not in _RESULTS:
        Z, Y = mixed_inputs(n, k)
        _RESULTS[n, k] = cases["mixed", n].open(L).glm_score_multi_dosage(Y, Z if k else None)
    return _RESULTS[n, k]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_parity_with_the_oracle(gpu_lib, cases, n, k):
    """Every row of every phenotype.  Worst difference seen on an MI355X: see DESIGN.md 3.10."""
    c = cases["mixed", n]
    Z, Y = mixed_inputs(n, k)
    got = _mixed_result(gpu_lib, cases, n, k)
    assert got["beta"].shape == (c.m, len(Y))
    worst_all = 0.0
    for p, y in enumerate(Y):
        col = _col(got, p)
        fitted, worst = O.check_rows(col, c.x, O.Null(y, Z), rel=REL)
        worst_all = max(worst_all, worst)
        ok = col["errcode"] == None  # noqa: E711 -- check_rows found the oracle's errcodes
        print(f"n={n} k={k} phenotype {p}: {fitted} fitted of {c.m}, {ok[c.track].sum()} of {c.track.sum()} tracks, "
              f"worst {worst:.3g}")
        assert 2 * ok[c.track].sum() >= c.track.sum(), (n, k, p)
        assert ok[c.full].all(), (n, k, p)
    print(f"n={n} k={k}: worst difference {worst_all:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_counts_equal_the_dense_logistic_fit(gpu_lib, cases, n, k):
    c = cases["mixed", n]
    Z, Y = mixed_inputs(n, k)
    got = _mixed_result(gpu_lib, cases, n, k)
    ds = c.open(gpu_lib)
    for p, y in enumerate(Y):
        want = ds.glm(y, Z if k else None, model="logistic", firth=False)
        _counts_equal_the_dense_logistic_fit(_col(got, p), want, ctx=(n, k, p))


@pytest.mark.gpu
def test_made_rows(gpu_lib, cases):
    c = cases["made"]
    ds = c.open(gpu_lib)
    Z, Y = made_inputs()
    got = ds.glm_score_multi_dosage(Y, Z)
    for p, y in enumerate(Y):
        col = _col(got, p)
        fitted, worst = O.check_rows(col, c.x, O.Null(y, Z), rel=REL)
        print(f"made rows phenotype {p}: {fitted} fitted of {c.m}, worst {worst:.3g}")
        _counts_equal_the_dense_logistic_fit(col, ds.glm(y, Z, model="logistic", firth=False), ctx=p)
        codes = dict(zip(MADE_ROWS, col["errcode"]))
        assert codes["constant 4915"] == "CONST_ALLELE"
        assert codes["all missing, no track"] == codes["all missing, empty track"] == "TOO_FEW_SAMPLES"
        assert codes["two values"] is None and codes["all missing, full track"] is None
        assert col["a1_freq"][0] == 4915.0 / 32768.0
        full = MADE_ROWS.index("all missing, full track")
        assert col["obs_ct"][full] == MADE_N - made_nan_samples().sum()
        cover = MADE_ROWS.index("entries cover the missing calls")
        assert col["obs_ct"][cover] == MADE_N - made_nan_samples().sum()


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("n", EDGE_N)
def test_sample_counts_at_a_64_sample_edge(gpu_lib, cases, n, k):
    c = cases["edge", n]
    ds = c.open(gpu_lib)
    Z, Y = edge_inputs(n, k)
    zc = Z if k else None
    got = ds.glm_score_multi_dosage(Y, zc)
    assert got["beta"].shape == (c.m, len(Y))
    for p, y in enumerate(Y):
        fitted, worst = O.check_rows(_col(got, p), c.x, O.Null(y, Z), rel=REL)
        print(f"n={n} k={k} phenotype {p}: {fitted} fitted of {c.m}, worst {worst:.3g}")
        assert fitted >= 20, (n, k, p, fitted)
        _counts_equal_the_dense_logistic_fit(_col(got, p), ds.glm(y, zc, model="logistic", firth=False), ctx=(n, k, p))


@pytest.fixture(scope="module")
def six_1003():
    """The covariates and six phenotypes of the bit-for-bit tests: n = 1003, k = 3."""
    rng = np.random.default_rng(1003)
    Z = _covariates(rng, 3, 1003)
    return Z, _six(rng, 1003, Z)


@pytest.mark.gpu
def test_bit_for_bit_against_the_hardcall_route(gpu_lib, cases, six_1003):
    L = gpu_lib
    Z, Y = six_1003
    # (a) tracks that restate their calls
    c = cases["restated"]
    assert c.track.sum() > 60 and {0x20, 0x40, 0x60} <= set(c.dkinds)
    hard = L.Dataset.open(cases["restated_hard"])
    want = hard.glm_score_multi(Y, Z)
    assert (want["errcode"] == None).sum() > c.m * len(Y) // 2  # noqa: E711
    _same(c.open(L).glm_score_multi_dosage(Y, Z), want, ctx="restated")
    # (c) a file without tracks through the new entry
    _same(hard.glm_score_multi_dosage(Y, Z), want, ctx="no tracks")
    hard.close()
    # (b) the track-less variants of a mixed file
    c = cases["mixed", 1003]
    twin = L.Dataset.open(cases["mixed_hard"])
    want = twin.glm_score_multi(Y, Z)
    twin.close()
    got = c.open(L).glm_score_multi_dosage(Y, Z)
    assert (~c.track).sum() >= 10
    _same(_rows(got, ~c.track), _rows(want, ~c.track), ctx="track-less variants")
    changed = ~np.array([np.array_equal(got["beta"][v], want["beta"][v], equal_nan=True) for v in range(c.m)])
    assert changed[c.track].any() and not changed[~c.track].any()


def _raw_bytes(L, ds, Y, Z):
    y = np.ascontiguousarray(Y, dtype=np.float64)
    z = np.ascontiguousarray(Z, dtype=np.float64)
    m = ds.v_end - ds.v_begin
    out = np.full(L.GLM_ROW_DTYPE.itemsize * m * len(y), 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = getattr(L.raw(), NAME)(ds._h, None, ds.v_begin, ds.v_end, len(y), y.ctypes.data_as(C.c_void_p), len(z),
                                z.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), eb)
    assert rc == L.PGH_OK, eb.value
    return out.tobytes()


@pytest.mark.gpu
def test_a_row_depends_on_nothing_but_its_own_inputs(gpu_lib, cases, six_1003):
    L = gpu_lib
    c = cases["mixed", 1003]
    ds = c.open(L)
    Z, Y = six_1003
    whole = ds.glm_score_multi_dosage(Y, Z)
    assert (whole["errcode"] == None).sum() > c.m * len(Y) // 3  # noqa: E711
    # a repeated call's raw bytes
    assert _raw_bytes(L, ds, Y, Z) == _raw_bytes(L, ds, Y, Z)
    # a window opened at variant 37, and a sub-range of it
    part = L.Dataset.open(c.path, variant_begin=37, variant_end=c.m)
    _same(part.glm_score_multi_dosage(Y, Z), _rows(whole, slice(37, c.m)), ctx="window")
    _same(part.glm_score_multi_dosage(Y, Z, v_begin=41, v_end=63), _rows(whole, slice(41, 63)), ctx="window range")
    part.close()
    _same(ds.glm_score_multi_dosage(Y, Z, v_begin=11, v_end=12), _rows(whole, slice(11, 12)), ctx="one variant")
    # one phenotype alone, and the phenotypes in another order
    for p in range(len(Y)):
        _same(_col(ds.glm_score_multi_dosage(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))
    perm = [4, 0, 5, 2, 1, 3]
    shuffled = ds.glm_score_multi_dosage(Y[perm], Z)
    for at, p in enumerate(perm):
        _same(_col(shuffled, at), _col(whole, p), ctx=("permuted", p))
    # The scratch budget.  At n = 1003 the smallest column block is 1024 sample rows x 64 columns x 8 bytes = 524,288
    # bytes and a phenotype's mask is 256 bytes; a budget of which three quarters are less than that leaves one
    # phenotype per block, so the six run as six blocks.  What the block leaves bounds the chunk: per variant and
    # phenotype 10 sums, 14 packed entries of H_N and g_N, a count and a row (80 + 112 + 4 + 48 bytes at k = 3), plus the
    # expanded rows' 144 bytes per 64 samples and 4 bytes of list: 2,552 bytes.
    per_variant = 244 + 144 * 16 + 4
    lo, hi = 5, 75
    for budget, chunk in ((1, 1), (524_288 + 256 + 7 * per_variant, 7)):
        assert budget // 4 * 3 < 524_288 + 256 and max(1, (budget - 524_544) // per_variant) == chunk
        assert chunk < hi - lo  # more than one chunk, some with and without tracks side by side
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(ds.glm_score_multi_dosage(Y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx=budget)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["word_block", "tile_minus_one", "all_but_one", "first"])
def test_sample_subsets(gpu_lib, cases, shape):
    """Whole words, one sample short of two words, all but one sample: against the oracle on the physically subsetted
    values, pgh_glm's counts under the same subset, and a sub-range bit for bit.  One sample: one class, refused."""
    L = gpu_lib
    c = cases["mixed", 1003]
    ds = c.open(L)
    mask = SS.shapes(c.n)[shape]
    ss = ds.subset(mask)
    if shape == "first":
        with pytest.raises(L.PghArgError, match="no cases or no controls"):
            ds.glm_score_multi_dosage(np.array([[1.0], [0.0]]), None, subset=ss)
        ss.close()
        return
    rng = np.random.default_rng(7)
    Zr = _covariates(rng, 2, c.n)
    Yr = _phenotypes(rng, c.n, Zr, specs=((0.35, 0.03), (0.5, 0.0), (0.3, 0.1)))
    Z, Y = np.ascontiguousarray(Zr[:, mask]), np.ascontiguousarray(Yr[:, mask])
    got = ds.glm_score_multi_dosage(Y, Z, subset=ss)
    x = c.x[:, mask]
    total = 0
    for p, y in enumerate(Y):
        fitted, worst = O.check_rows(_col(got, p), x, O.Null(y, Z), rel=REL)
        print(f"{shape} ({int(mask.sum())} samples) phenotype {p}: {fitted} fitted, worst {worst:.3g}")
        total += fitted
        _counts_equal_the_dense_logistic_fit(_col(got, p), ds.glm(y, Z, model="logistic", firth=False, subset=ss),
                                             ctx=(shape, p))
    assert total > len(Y) * c.m // 4
    _same(ds.glm_score_multi_dosage(Y, Z, v_begin=20, v_end=50, subset=ss), _rows(got, slice(20, 50)), ctx=shape)
    ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,what", LAYOUTS)
def test_phenotypes_at_and_across_the_column_blocks(gpu_lib, cases, k, what):
    """17 phenotypes, two blocks of squared-weight columns.  k = 14: the k + 2 x-columns of a phenotype are exactly one
    16-column block; k = 13: 15 columns, so every phenotype after the first straddles a block edge."""
    c = cases["mixed", LAYOUT_N]
    Z, Y = layout_inputs(k)
    assert len(Y) == LAYOUT_PHENOTYPES and (len(Y) * (k + 2) + 15) // 16 >= 16
    assert ((k + 2) % 16 == 0) == (what == "a phenotype is one block")
    got = c.open(gpu_lib).glm_score_multi_dosage(Y, Z)
    for p in (0, LAYOUT_PHENOTYPES - 2, LAYOUT_PHENOTYPES - 1):
        fitted, worst = O.check_rows(_col(got, p), c.x, O.Null(Y[p], Z), rel=REL)
        print(f"k={k} phenotype {p}: {fitted} fitted of {c.m}, worst {worst:.3g}")
        assert fitted > c.m // 3, (k, p, fitted)
    for p in range(6, LAYOUT_PHENOTYPES - 1):
        _same(_col(got, p), _col(got, p % 6), ctx=(k, p))
    assert not np.array_equal(got["beta"][:, LAYOUT_PHENOTYPES - 1], got["beta"][:, 0], equal_nan=True)


@pytest.mark.gpu
def test_refusals(gpu_lib, tmp_path):
    """test_glm_score_multi.test_refusals' table through the new symbol, without "hardcalls only"."""
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    group = L.Dataset.open_sharded(path, [0, 0])
    n, m = dense.n_samples, dense.v_end - dense.v_begin
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    assert dense.glm_score_multi_dosage(Y, v_begin=0, v_end=8)["errcode"].shape == (8, 2)

    dose_path = str(tmp_path / "dose.pgen")
    make_dosage_file(dose_path, 20, 100, 300, True)
    dose = L.Dataset.open(dose_path)
    assert dose.info.dosage_variant_ct > 0
    y_dose = (np.arange(100) % 3 == 0).astype(np.float64)[None, :]

    def raw(ds, phen, n_pheno=None, z=None, n_covar=0, v0=0, v1=8, subset=None, name=NAME):
        out = np.full(L.GLM_ROW_DTYPE.itemsize * max(1, v1 - v0) * max(1, len(phen)), 0xAB, dtype=np.uint8)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        rc = getattr(L.raw(), name)(ds._h, subset, v0, v1, len(phen) if n_pheno is None else n_pheno, p(phen), n_covar,
                                    p(z), p(out), eb)
        return rc, eb.value.decode(), bool((out == 0xAB).all())

    y_two = Y.copy()
    y_two[1, 4] = 2.0
    y_one = Y.copy()
    y_one[1] = 1.0
    y_one[1, ::5] = NAN
    inf = np.zeros((2, n))
    inf[1, 5] = np.inf
    refused = [
        ("at least one phenotype", (dense, Y, 0)),
        ("phenotype must be 0 or 1", (dense, y_two)),
        ("no cases or no controls", (dense, y_one)),
        ("needs a dense-resident dataset", (sp, Y)),
        ("one device's dataset", (group, Y)),
        ("at most 20 covariates", (dense, Y, None, np.zeros((21, n)), 21)),
        ("covariate 1 is not finite at sample 5", (dense, Y, None, inf, 2)),
        ("outside the resident range", (dense, Y, None, None, 0, 0, m + 1)),
        ("outside the resident range", (dense, Y, None, None, 0, 9, 8)),
    ]
    for text, args in refused:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    assert "(phenotype 1)" in raw(dense, y_two)[1] and "(phenotype 1)" in raw(dense, y_one)[1]
    with pytest.raises(ValueError, match="phenotype must be 0 or 1"):
        dense.glm_score_multi_dosage(y_two)
    # an empty range is fine
    rc, msg, untouched = raw(dense, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched
    assert dense.glm_score_multi_dosage(Y, v_begin=3, v_end=3)["errcode"].shape == (0, 2)
    # the dosage file: pgh_glm_score_multi itself still refuses it, the new entry takes it
    rc, msg, untouched = raw(dose, y_dose, name="pgh_glm_score_multi")
    assert rc == L.PGH_ERR_ARG and "hardcalls only" in msg and untouched
    rc, msg, untouched = raw(dose, y_dose)
    assert rc == L.PGH_OK and not untouched, msg
    for ds in (dose, group, sp, dense):
        ds.close()
