"""pgh_glm_score_sparse_multi / Dataset.glm_score_sparse_multi: the logistic score test over a sparse-resident dataset
for many phenotypes in one walk of the entries.  Every column against the FP64 oracle (tests/glm_score_oracle.py, one
Null per phenotype) within 1e-9 on check_rows' scale; obs_ct, a1_freq and the count decisions equal pgh_glm's logistic
fit on the dense dataset of the same file; the single-phenotype route and the dense many-phenotype route agree within
2e-9 (two results, each within 1e-9 of the oracle); and a row does not depend on the other phenotypes, its place among
them, n_pheno, the phenotype block, the range, the window, the variant chunk or the scratch budget: bit for bit."""

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

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse_multi"]
REL = 1e-9          # test_glm_score_sparse.REL
M_R = 600
PHENO_BLOCK = 64    # kGlmScoreSparsePb: the phenotypes of one pair block at most
LONG = 1024         # kGlmSparseLong: the entries of one segment; longer rows go to the workgroup form
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
# (case rate, NaN rate) of the five phenotypes; a sixth shares the first one's NaN pattern (test_glm_score_multi's)
PHENO_SPECS = ((0.2, 0.03), (0.5, 0.0), (0.05, 0.1), (0.35, 0.03), (0.1, 0.3))
HET_ROWS = (7, 8)   # rare_matrix draws no het-majority rows: these two are made so
PARITY_N = (257, 4099)
PARITY_K = (0, 1, 3)
PARITY_ROWS = sorted(set(range(0, M_R, 23)) | set(HET_ROWS))
WIDTHS = [1, 2, 4, 8, 12, 16, 20]
EDGE_N = (63, 64, 65, 128)
EDGE_K = (0, 2)
EDGE_SPECS = ((0.5, 0.03), (0.35, 0.03))


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse_multi(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse_multi")
    kernels = open(os.path.join(ROOT, "plinking_duck_amd", "csrc", "glm.hpp")).read()
    assert f"kGlmScoreSparsePb = {PHENO_BLOCK};" in kernels and f"kGlmSparseLong = {LONG};" in kernels


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_sparse_multi_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_sparse_multi(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse_multi(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def test_a_null_dataset_is_refused_with_out_untouched(lib):
    out = np.full(32 * 4, 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    rc = lib.raw().pgh_glm_score_sparse_multi(None, None, 0, 4, 1, y.ctypes.data_as(C.c_void_p), 0, None,
                                              out.ctypes.data_as(C.c_void_p), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and (out == 0xAB).all()


# ---- helpers -----------------------------------------------------------------------------------------------------

def _values(geno):
    """test_glm_score_sparse._values"""
    return np.where(geno == 3, -9.0, geno.astype(np.float64))


def _covariates(rng, k, n):
    """test_glm_score_sparse._covariates"""
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def _phenotypes(rng, n, Z, specs=PHENO_SPECS):
    """test_glm_score_multi._phenotypes"""
    ys = [O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in specs]
    shared = O.pheno(rng, n, Z, case_rate=0.3, missing=0.0)
    shared[np.isnan(ys[0])] = NAN
    return np.stack(ys + [shared])


@functools.lru_cache(maxsize=None)
def _matrix(m, n, seed):
    """test_glm_score_sparse._matrix"""
    rng = np.random.default_rng(seed)
    geno = W.rare_matrix(m, n, rng)
    for v, rate in zip(HET_ROWS, (0.01, 0.3)):
        hit = rng.random(n) < rate
        geno[v] = 1
        geno[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
    return geno, W.choose_kinds(geno, rng)


def _minor(geno):
    return geno.shape[1] - np.array([np.bincount(r, minlength=4).max() for r in geno])


@functools.lru_cache(maxsize=None)
def parity_inputs(n, k):
    """(Z, Y, nulls): test_glm_score_multi.test_parity_with_the_oracle's draw, and the oracle's null fits."""
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    Y = _phenotypes(rng, n, Z)
    return Z, Y, [O.Null(y, Z) for y in Y]


@functools.lru_cache(maxsize=None)
def edge_inputs(n, k):
    """test_glm_score_multi.edge_inputs"""
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    return Z, np.stack([O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in EDGE_SPECS])


@functools.lru_cache(maxsize=None)
def offset_inputs():
    """(Z, Y): n = 4099, k = 3, covariate 0 moved up by 50 of its standard deviations and covariate 2 down by 50.  The
    two shifts cancel in O.pheno's linear predictor, the NaN rates go up to 30 %, so the patterns' means differ."""
    n = 4099
    rng = np.random.default_rng(4242)
    Z = _covariates(rng, 3, n)
    Z[0] += 50.0 * Z[0].std()
    Z[2] -= 50.0 * Z[2].std()
    return Z, np.stack([O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in PHENO_SPECS])


def _col(out, p, rows=slice(None)):
    return {key: v[rows, p] for key, v in out.items()}


def _rows(out, rows):
    return {key: v[rows] for key, v in out.items()}


def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _close(a, b, rel, ctx=None):
    """test_glm_score_sparse._close; returns the worst relative difference."""
    worst = 0.0
    for key in ("obs_ct", "errcode", "firth"):
        assert list(a[key]) == list(b[key]), (key, ctx)
    assert np.array_equal(a["a1_freq"], b["a1_freq"], equal_nan=True), ("a1_freq", ctx)
    se = np.nan_to_num(b["se"], nan=0.0)
    for key in ("beta", "se", "stat", "p"):
        g, e = a[key], b[key]
        assert np.array_equal(np.isnan(g), np.isnan(e)), (key, ctx)
        scale = np.abs(e) + (se if key == "beta" else 1.0 if key == "stat" else 0.0)
        ok = np.isnan(e) | (np.abs(g - e) <= rel * scale + 1e-300)
        bad = np.flatnonzero(~ok)
        assert not len(bad), (key, ctx, bad[:5], g[bad[:5]], e[bad[:5]])
        with np.errstate(all="ignore"):
            d = np.abs(g - e) / scale
        worst = max(worst, float(np.nanmax(np.where(np.isfinite(d), d, 0.0), initial=0.0)))
    return worst


def _counts_equal_the_dense_logistic_fit(got, want, ctx=None):
    """test_glm_score_sparse._counts_equal_the_dense_logistic_fit"""
    assert got["obs_ct"].tolist() == want["obs_ct"].tolist(), ctx
    assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True), ctx
    for code in ("TOO_FEW_SAMPLES", "CONST_ALLELE"):
        assert (got["errcode"] == code).tolist() == (want["errcode"] == code).tolist(), (code, ctx)
    assert not got["firth"].any(), ctx


# ---- no device: conditions on the inputs ------------------------------------------------------------------------

@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_have_fitted_null_models_and_fitted_rows(n, k):
    """So that a GPU case cannot pass on rows that are not fitted: every null model converges, and the oracle fits more
    than half of the compared rows of every phenotype."""
    x = _values(_matrix(M_R, n, n)[0])
    Z, Y, nulls = parity_inputs(n, k)
    assert len(set(y.tobytes() for y in Y)) == 6
    for p, nul in enumerate(nulls):
        assert nul.status is None, (n, k, p, nul.status)
        fitted = sum(O.oracle_row(x[i], nul)["errcode"] is None for i in PARITY_ROWS)
        assert fitted > len(PARITY_ROWS) // 2, (n, k, p, fitted)


def test_the_offset_inputs_have_fitted_null_models():
    Z, Y = offset_inputs()
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None and 2 <= nul.steps <= 25, (p, nul.status, nul.steps)
    means = [Z[:, ~np.isnan(y)].mean(axis=1) for y in Y]
    assert not np.array_equal(means[0], means[4])


# ---- on the GPU --------------------------------------------------------------------------------------------------

class _File:
    """test_glm_score_sparse._File: a .pgen of every record type, its dense dataset and its calls."""

    def __init__(self, L, tmp, m, n, seed, codes=None, name="rare"):
        self.L, self.m, self.n = L, m, n
        if codes is None:
            self.geno, self.kinds = _matrix(m, n, seed)
        else:
            self.geno, self.kinds = codes, W.choose_kinds(codes, np.random.default_rng(seed))
        self.path = str(tmp / f"{name}_{n}.pgen")
        W.write_pgen(self.path, self.geno, self.kinds)
        self.dense = L.Dataset.open(self.path)
        self.x = _values(self.geno)

    def sparse(self, **kw):
        # several windows per open, so that parts are concatenated and windows start after LD bases
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * self.dense.info.pitch_bytes))
            return self.L.Dataset.open(self.path, sparse=True, **kw)


@pytest.fixture(scope="module")
def rare_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_multi")
    return {n: _File(gpu_lib, tmp, M_R, n, n) for n in PARITY_N}


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle_for_every_base_code(gpu_lib, rare_files, n, k):
    f = rare_files[n]
    Z, Y, nulls = parity_inputs(n, k)
    zc = Z if k else None
    want = [f.dense.glm(y, zc, model="logistic", firth=False) for y in Y]
    dense_multi = f.dense.glm_score_multi(Y, zc)
    minor = _minor(f.geno)
    for max_minor in (0, 1, n):
        sp = f.sparse(max_minor=max_minor)
        info = sp.sparse_info()
        got = sp.glm_score_sparse_multi(Y, zc)
        assert got["beta"].shape == (M_R, len(Y))
        for p, y in enumerate(Y):
            col = _col(got, p)
            fitted, worst = O.check_rows(_rows(col, PARITY_ROWS), f.x[PARITY_ROWS], nulls[p], rel=REL)
            assert fitted > len(PARITY_ROWS) // 2
            _counts_equal_the_dense_logistic_fit(col, want[p], ctx=(n, k, max_minor, p))
            single = _close(col, sp.glm_score_sparse(y, zc), 2 * REL, ctx=("single", n, k, max_minor, p))
            dense = _close(col, _col(dense_multi, p), 2 * REL, ctx=("dense", n, k, max_minor, p))
            print(f"n={n} k={k} max_minor={max_minor} phenotype {p}: {fitted} fitted of {len(PARITY_ROWS)}, worst "
                  f"{worst:.3g}; against the single route {single:.3g}, the dense route {dense:.3g}")
        if max_minor == n:
            # het-, hom-alt- and missing-majority rows all run from their entries
            assert info.dense_variant_ct == 0 and all(info.base_hist[b] > 0 for b in (1, 2, 3))
            if n == 4099:  # both sides of the group / workgroup threshold
                assert (minor > LONG).any() and ((minor > 0) & (minor <= LONG)).any()
        if max_minor == 1:
            assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
            assert int((minor > 1).sum()) == info.dense_variant_ct
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_minor", [0, 4099])
def test_a_row_does_not_depend_on_anything_but_its_own_inputs(gpu_lib, rare_files, max_minor):
    """Bit for bit: the other phenotypes, the place, n_pheno, the block edge, the range, the window, the chunk and the
    scratch budget.  max_minor = 0: every row with a carrier is walked from its pool row."""
    f = rare_files[4099]
    Z, Y, _ = parity_inputs(4099, 3)
    sp = f.sparse(max_minor=max_minor)
    whole = sp.glm_score_sparse_multi(Y, Z)
    assert (whole["errcode"] == None).sum() > M_R * len(Y) // 3  # noqa: E711
    _same(sp.glm_score_sparse_multi(Y, Z), whole, ctx="again")
    for p in range(len(Y)):
        _same(_col(sp.glm_score_sparse_multi(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))
    perm = np.random.default_rng(5).permutation(len(Y))
    assert perm.tolist() != list(range(len(Y)))
    shuffled = sp.glm_score_sparse_multi(Y[perm], Z)
    for at, p in enumerate(perm):
        _same(_col(shuffled, at), _col(whole, p), ctx=("shuffled", p))
    _same(sp.glm_score_sparse_multi(Y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx="range")
    # a window that starts after an LD base
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))
    v1 = min(M_R, v0 + 150)
    part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
    _same(part.glm_score_sparse_multi(Y, Z), _rows(whole, slice(v0, v1)), ctx=("window", v0))
    part.close()
    # the block edge 64 | 1: the six cycled, and at position 64 a phenotype of its own
    own = O.pheno(np.random.default_rng(17_003), f.n, Z, case_rate=0.25, missing=0.05)
    many = np.stack([Y[i % len(Y)] for i in range(PHENO_BLOCK)] + [own])
    wide = sp.glm_score_sparse_multi(many, Z)
    alone = sp.glm_score_sparse_multi(own[None, :], Z)
    assert (alone["errcode"] == None).sum() > M_R // 3  # noqa: E711
    _same(_col(wide, PHENO_BLOCK), _col(alone, 0), ctx="65th")
    for i in (0, 7, PHENO_BLOCK - 1):
        _same(_col(wide, i), _col(whole, i % len(Y)), ctx=("block", i))
    # The pair block takes 16 bytes x 4099 samples per phenotype, a chunk variant 228 bytes per phenotype (k = 3: 10
    # sums, 14 entries of {H_N, g_N}, a count and a 32-byte row).  1 byte: one phenotype per block, a chunk of one
    # variant.  134,460 bytes: two phenotypes (131,168 + 456 fit, three do not), and the 3,292 bytes left are seven
    # variants.
    five = Y[:5]
    for budget in (1, 32 * 4099 + 7 * 456 + 100):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(sp.glm_score_sparse_multi(five, Z, v_begin=200, v_end=240),
                  {key: v[200:240, :5] for key, v in whole.items()}, ctx=budget)
    empty = sp.glm_score_sparse_multi(Y, Z, v_begin=77, v_end=77)
    assert empty["beta"].shape == (0, len(Y)) and empty["errcode"].shape == (0, len(Y))
    sp.close()


@pytest.mark.gpu
def test_long_rows_and_long_missing_lists(gpu_lib, tmp_path):
    n, m, k = 70_000, 120, 20
    f = _File(gpu_lib, tmp_path, m, n, 70)
    entries = _minor(f.geno)
    in_missing_list = np.array([(r == 3).sum() if np.bincount(r, minlength=4).argmax() != 3 else 0 for r in f.geno])
    assert entries.max() > 10_000 and in_missing_list.max() > 1_000
    rng = np.random.default_rng(71)
    Z = _covariates(rng, k, n)
    Y = np.stack([O.pheno(rng, n, Z, case_rate=c, missing=mi) for c, mi in ((0.2, 0.03), (0.5, 0.0), (0.35, 0.3))])
    sp = f.sparse(max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_score_sparse_multi(Y, Z)
    # the longest entry lists, the longest missing lists, the het-majority rows and a spread: 16 rows
    idx = list(dict.fromkeys(np.argsort(entries)[-5:].tolist() + np.argsort(in_missing_list)[-3:].tolist()
                             + list(HET_ROWS) + list(range(3, m, 9))))[:16]
    assert len(idx) == 16
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None
        fitted, worst = O.check_rows(_rows(_col(got, p), idx), f.x[idx], nul, rel=REL)
        print(f"long rows, phenotype {p}: {fitted} fitted of 16, worst {worst:.3g}")
        assert fitted >= 8
    _counts_equal_the_dense_logistic_fit(_col(got, 2), f.dense.glm(Y[2], Z, model="logistic", firth=False))
    sp.close()
    f.dense.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kp", WIDTHS)
def test_every_instantiated_width(gpu_lib, rare_files, kp):
    """k = kp and kp - 1 for every width GlmPadCovar returns (kp = 1 covers the width 0), two phenotypes of different
    patterns."""
    f = rare_files[4099]
    idx = sorted(set(range(5, M_R, 55)) | set(HET_ROWS))[:12]
    assert len(idx) == 12
    sp = f.sparse(max_minor=f.n)
    for k in (kp, kp - 1):
        rng = np.random.default_rng(3000 + k)
        Z = _covariates(rng, k, f.n)
        Y = np.stack([O.pheno(rng, f.n, Z), O.pheno(rng, f.n, Z, case_rate=0.35, missing=0.1)])
        got = sp.glm_score_sparse_multi(Y, Z if k else None, v_begin=0, v_end=max(idx) + 1)
        for p, y in enumerate(Y):
            nul = O.Null(y, Z)
            assert nul.status is None
            fitted, worst = O.check_rows(_col(got, p), f.x, nul, rel=REL, idx=idx)
            print(f"k={k} phenotype {p}: {fitted} fitted of 12, worst {worst:.3g}")
            assert fitted >= 4
        # the same two among 33: lanes across 64 phenotypes, where the covariate rows are scalar loads
        wide = sp.glm_score_sparse_multi(np.stack([Y[i % 2] for i in range(33)]), Z if k else None, v_begin=0,
                                         v_end=max(idx) + 1)
        for at in (0, 1, 32):
            _same(_col(wide, at), _col(got, at % 2), ctx=(k, at))
    sp.close()


@pytest.mark.gpu
def test_pattern_centring_under_offset_covariates(gpu_lib, rare_files):
    """Sums of raw, uncentred covariates lose about four digits here, and sums centred on another pattern's means lose
    some.  The single route's worst difference from the oracle is printed beside each column's."""
    f = rare_files[4099]
    Z, Y = offset_inputs()
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi(Y, Z)
        for p, y in enumerate(Y):
            nul = O.Null(y, Z)
            assert nul.status is None
            _, single = O.check_rows(_rows(sp.glm_score_sparse(y, Z), PARITY_ROWS), f.x[PARITY_ROWS], nul, rel=1.0)
            print(f"offset max_minor={max_minor} phenotype {p}: the single route's worst {single:.3g}")
            fitted, worst = O.check_rows(_rows(_col(got, p), PARITY_ROWS), f.x[PARITY_ROWS], nul, rel=REL)
            print(f"offset max_minor={max_minor} phenotype {p}: {fitted} fitted of {len(PARITY_ROWS)}, worst {worst:.3g}")
            assert fitted > len(PARITY_ROWS) // 3
        sp.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, rare_files):
    f = rare_files[4099]
    rng = np.random.default_rng(12)
    keep = rng.random(f.n) < 0.5
    n = int(keep.sum())
    Z = _covariates(rng, 3, n)
    Y = _phenotypes(rng, n, Z)[:3]
    nulls = [O.Null(y, Z) for y in Y]
    assert all(nul.status is None for nul in nulls)
    ss_d = f.dense.subset(keep)
    idx = sorted(set(range(0, M_R, 29)) | set(HET_ROWS))
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        ss = sp.subset(keep)
        got = sp.glm_score_sparse_multi(Y, Z, subset=ss)
        for p, y in enumerate(Y):
            col = _col(got, p)
            _counts_equal_the_dense_logistic_fit(col, f.dense.glm(y, Z, model="logistic", firth=False, subset=ss_d),
                                                 ctx=(max_minor, p))
            fitted, worst = O.check_rows(_rows(col, idx), f.x[idx][:, keep], nulls[p], rel=REL)
            print(f"subset max_minor={max_minor} phenotype {p}: {fitted} fitted of {len(idx)}, worst {worst:.3g}")
            assert fitted > len(idx) // 3
        with pytest.raises(ValueError, match="different dataset"):
            sp.glm_score_sparse_multi(Y, Z, subset=ss_d)
        ss.close()
        sp.close()
    ss_d.close()


@pytest.fixture(scope="module")
def hard_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_multi_hard")
    return {n: _File(gpu_lib, tmp, SS.M, n, n, codes=SS.hard_codes(n), name="hard") for n in EDGE_N + (SS.N_SMALL,)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("n", EDGE_N)
def test_sample_counts_at_a_64_sample_edge(gpu_lib, hard_files, n, k):
    """Every row of both phenotypes against the oracle, and the counts against pgh_glm's logistic fit."""
    f = hard_files[n]
    Z, Y = edge_inputs(n, k)
    zc = Z if k else None
    for max_minor in (0, n):
        sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=max_minor)
        got = sp.glm_score_sparse_multi(Y, zc)
        assert got["beta"].shape == (SS.M, len(Y))
        for p, y in enumerate(Y):
            nul = O.Null(y, Z)
            assert nul.status is None
            fitted, worst = O.check_rows(_col(got, p), f.x, nul, rel=REL)
            print(f"n={n} k={k} max_minor={max_minor} phenotype {p}: {fitted} fitted of {SS.M}, worst {worst:.3g}")
            assert fitted >= 120, (n, k, p, fitted)
            _counts_equal_the_dense_logistic_fit(_col(got, p), f.dense.glm(y, zc, model="logistic", firth=False),
                                                 ctx=(n, k, p))
        assert got["errcode"][SS.ROW_ALL_MISSING].tolist() == ["TOO_FEW_SAMPLES"] * len(Y)
        assert got["errcode"][SS.ROW_MONO].tolist() == ["CONST_ALLELE"] * len(Y)
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["all_but_one", "last_word", "word_block", "tile_plus_one", "stride4"])
def test_structured_sample_subsets(gpu_lib, hard_files, shape):
    """Against the oracle on the physically subsetted matrix (test_glm_score_multi.test_sample_subsets' inputs)."""
    f = hard_files[SS.N_SMALL]
    mask = SS.shapes(f.n)[shape]
    n_out = int(mask.sum())
    rng = np.random.default_rng(7)
    Zr = _covariates(rng, 2, f.n)
    Yr = _phenotypes(rng, f.n, Zr, specs=((0.35, 0.03), (0.5, 0.0), (0.3, 0.1)))
    Z, Y = np.ascontiguousarray(Zr[:, mask]), np.ascontiguousarray(Yr[:, mask])
    sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=f.n)
    ss, ss_d = sp.subset(mask), f.dense.subset(mask)
    got = sp.glm_score_sparse_multi(Y, Z, subset=ss)
    x = f.x[:, mask]
    total = 0
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None, (shape, p, nul.status)
        fitted, worst = O.check_rows(_col(got, p), x, nul, rel=REL)
        print(f"{shape} ({n_out} samples) phenotype {p}: {fitted} fitted, worst {worst:.3g}")
        assert fitted >= 120, (shape, p, fitted)  # of SS.M = 130 rows, three of them made undecidable
        total += fitted
        _counts_equal_the_dense_logistic_fit(_col(got, p), f.dense.glm(y, Z, model="logistic", firth=False, subset=ss_d),
                                             ctx=(shape, p))
    assert total > 0
    ss.close()
    ss_d.close()
    sp.close()


def _decision_file(tmp_path):
    """test_glm_score_sparse._decision_file, with a second phenotype of another pattern."""
    n = 64
    rng = np.random.default_rng(5)
    y = (rng.random(n) < 0.35).astype(np.float64)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    y[[1, 2, 5, 9]] = [0.0, 0.0, 1.0, 1.0]       # cases and controls among the few used samples of rows 3 and 4
    geno = np.zeros((8, n), dtype=np.uint8)
    geno[0, no_pheno] = 1                        # every sample with a phenotype is hom-ref
    geno[1, 17] = 2                              # a singleton whose carrier has no phenotype
    geno[2] = 2
    geno[2, no_pheno[:2]] = [0, 1]               # the same under a hom-alt base
    geno[3] = 3
    geno[3, [1, 2, 5]] = [0, 1, 2]               # k + 2 = 3 used samples
    geno[4] = 3
    geno[4, [1, 2, 5, 9]] = [0, 1, 2, 1]         # k + 3: enough to fit
    geno[5] = rng.binomial(2, 0.2, n)            # the covariate
    geno[6] = rng.binomial(2, 0.3, n)
    geno[6, rng.random(n) < 0.1] = 3
    geno[7] = 1
    geno[7, rng.random(n) < 0.2] = 3             # het base: constant among the called
    y2 = y.copy()
    y2[no_pheno] = [0.0, 1.0, 0.0]               # the carriers of rows 0 and 1 have this phenotype
    y2[[20, 33]] = NAN
    path = str(tmp_path / "decisions.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    return path, geno, np.stack([y, y2])


@pytest.mark.gpu
def test_decisions(gpu_lib, tmp_path):
    L = gpu_lib
    path, geno, Y = _decision_file(tmp_path)
    n = geno.shape[1]
    Z = geno[5].astype(np.float64)[None, :]
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True, max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_score_sparse_multi(Y, Z)
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None
        exp = [O.oracle_row(x, nul) for x in _values(geno)]
        if p == 0:
            assert [e["errcode"] for e in exp] == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES",
                                                   None, "SINGULAR_MATRIX", None, "CONST_ALLELE"]
        else:
            assert [e["errcode"] for e in exp][:2] == [None, None]
        col = _col(got, p)
        assert list(col["errcode"]) == [e["errcode"] for e in exp]
        assert col["obs_ct"].tolist() == [e["obs_ct"] for e in exp]
        O.check_rows(col, _values(geno), nul, rel=REL)
        _counts_equal_the_dense_logistic_fit(col, dense.glm(y, Z, model="logistic", firth=False))
    sp.close()
    dense.close()


@pytest.mark.gpu
def test_a_failed_null_model_decides_its_own_phenotype_only(gpu_lib, rare_files):
    f = rare_files[257]
    rng = np.random.default_rng(77)
    z, z2 = rng.normal(size=(2, f.n))
    ya = O.pheno(rng, f.n, z[None, :], missing=0.1)
    yb = O.pheno(rng, f.n, z[None, :], case_rate=0.4, missing=0.0)
    # a covariate that duplicates another over the samples of phenotype a alone
    dup = np.where(np.isnan(ya), z2, z)
    sp = f.sparse(max_minor=f.n)
    for bad, good, code in ((np.stack([z, dup]), np.stack([z, z2]), "SINGULAR_MATRIX"),
                            (np.nan_to_num(ya, nan=0.0)[None, :], z[None, :], "NO_CONVERGENCE")):  # one equal to a
        assert O.Null(ya, bad).status == code and O.Null(yb, bad).status is None and O.Null(ya, good).status is None
        base = sp.glm_score_sparse_multi(ya[None, :], good)
        assert (base["errcode"] == None).sum() > M_R // 3  # noqa: E711
        decided = np.isin(base["errcode"][:, 0], ["TOO_FEW_SAMPLES", "CONST_ALLELE"])
        assert (base["errcode"] == "CONST_ALLELE").any() and not decided.all()
        got = sp.glm_score_sparse_multi(np.stack([ya, yb]), bad)
        a = _col(got, 0)
        assert a["errcode"][decided].tolist() == base["errcode"][decided, 0].tolist()
        assert set(a["errcode"][~decided]) == {code}
        assert a["obs_ct"].tolist() == base["obs_ct"][:, 0].tolist()
        assert np.array_equal(a["a1_freq"], base["a1_freq"][:, 0], equal_nan=True)
        for key in ("beta", "se", "stat", "p"):
            assert np.isnan(a[key]).all(), key
        # the other phenotype: fitted, against the oracle, and bit for bit what it is without the failing one
        b = _col(got, 1)
        fitted, worst = O.check_rows(_rows(b, PARITY_ROWS), f.x[PARITY_ROWS], O.Null(yb, bad), rel=REL)
        print(f"{code}: the other phenotype, {fitted} fitted of {len(PARITY_ROWS)}, worst {worst:.3g}")
        assert fitted > len(PARITY_ROWS) // 3
        _same(b, _col(sp.glm_score_sparse_multi(yb[None, :], bad), 0), ctx=code)
    sp.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    """Every PGH_ERR_ARG of the contract through the raw call, with its text and `out` untouched; then the binding."""
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    group = L.Dataset.open_sharded(path, [0, 0])
    n, m = sp.n_samples, sp.v_end - sp.v_begin
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    assert sp.glm_score_sparse_multi(Y, v_begin=0, v_end=8)["errcode"].shape == (8, 2)

    def raw(ds, phen, n_pheno=None, z=None, n_covar=0, v0=0, v1=8, subset=None):
        out = np.full(32 * max(1, v1 - v0) * max(1, len(phen)), 0xAB, dtype=np.uint8)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        rc = L.raw().pgh_glm_score_sparse_multi(ds._h, subset, v0, v1, len(phen) if n_pheno is None else n_pheno,
                                                p(phen), n_covar, p(z), p(out), eb)
        return rc, eb.value.decode(), bool((out == 0xAB).all())

    y_two = Y.copy()
    y_two[1, 4] = 2.0
    y_one = Y.copy()
    y_one[1] = 1.0
    y_one[1, ::5] = NAN
    y_zero = Y.copy()
    y_zero[1] = 0.0
    y_zero[1, ::5] = NAN
    inf = np.zeros((2, n))
    inf[1, 5] = np.inf
    other = dense.subset(np.arange(n) % 2 == 0)
    cases = [
        ("at least one phenotype", (sp, Y, 0)),
        ("phenotype must be 0 or 1", (sp, y_two)),
        ("no cases or no controls", (sp, y_one)),
        ("no cases or no controls", (sp, y_zero)),
        ("needs a sparse-resident dataset", (dense, Y)),
        ("one device's dataset", (group, Y)),
        ("at most 20 covariates", (sp, Y, None, np.zeros((21, n)), 21)),
        ("covariate 1 is not finite at sample 5", (sp, Y, None, inf, 2)),
        ("outside the resident range", (sp, Y, None, None, 0, 0, m + 1)),
        ("outside the resident range", (sp, Y, None, None, 0, 9, 8)),
        ("different dataset", (sp, Y[:, ::2], None, None, 0, 0, 8, other._h)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    # the phenotype messages name the phenotype
    for bad in (y_two, y_one, y_zero):
        assert "(phenotype 1)" in raw(sp, bad)[1]
    with pytest.raises(ValueError, match=r"phenotype must be 0 or 1.*\(phenotype 1\)"):
        sp.glm_score_sparse_multi(y_two)
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse_multi(Y, v_begin=0, v_end=8)
    # an empty range is fine
    rc, msg, untouched = raw(sp, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched
    assert sp.glm_score_sparse_multi(Y, v_begin=3, v_end=3)["errcode"].shape == (0, 2)
    other.close()
    for ds in (group, sp, dense):
        ds.close()
