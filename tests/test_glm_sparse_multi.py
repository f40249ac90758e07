"""pgh_glm_sparse_multi / Dataset.glm_sparse_multi: pgh_glm_sparse for many quantitative phenotypes, each with its own
missing-value pattern, in one walk of the entries.  Column p of a call is the row pgh_glm_sparse returns for phenotype
p alone: errcode, obs_ct, firth and a1_freq equal, the estimates within 1e-9 on check_rows' scale (the linear contract,
_close of tests/test_glm_sparse.py), and within 1e-9 of the FP64 oracle (tests/glm_oracle.py).  A row does not depend on
the other phenotypes, its place among them, the block, the range, the window, the chunk or the scratch budget: bit for
bit."""

import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W
import subset_shapes as SS

NAN = float("nan")
REL = 1e-9
NEW_SYMBOLS = ["pgh_glm_sparse_multi"]
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
WINDOW_ENV = "PGH_SPARSE_WINDOW_BYTES"
PHENO_BLOCK = 64  # kGlmSparseMultiPb
M_R = 600
HET_ROWS = (7, 8)  # rare_matrix draws no het-majority rows: these two are made so
PARITY_N, PARITY_K = (257, 4099), (0, 1, 3)
PARITY_ROWS = sorted(set(range(0, M_R, 23)) | set(HET_ROWS))
EDGE_N, EDGE_K = (63, 64, 65, 128), (0, 2)
WIDTHS = (1, 2, 4, 8, 12, 16, 20)
GROUP_P = (1, 2, 3, 5, 9, 17, 33, 64, 65, 70)


def _oracle():
    # glm_oracle needs scipy: only the tests that compare against it skip without it
    return pytest.importorskip("glm_oracle")


def _values(geno):
    """Codes (3 = missing) as the oracle's values (-9 = missing)."""
    return np.where(geno == 3, -9.0, geno.astype(np.float64))


def _covariates(rng, k, n):
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def _matrix(m, n, seed):
    """tests/test_glm_sparse.py's matrix: rare_matrix plus the two het-majority rows."""
    rng = np.random.default_rng(seed)
    geno = W.rare_matrix(m, n, rng)
    for v, rate in zip(HET_ROWS, (0.01, 0.3)):
        hit = rng.random(n) < rate
        geno[v] = 1
        geno[v, hit] = rng.integers(0, 4, hit.sum(), dtype=np.uint8)
    return geno, W.choose_kinds(geno, rng)


RSS_FLOOR = 1e-3
SMALL_ROW = 100


@functools.lru_cache(maxsize=None)
def _geno(m, n, seed):
    return _matrix(m, n, seed)


def _well_conditioned(y, Z, x_small):
    """No fitted row of x_small is a nearly exact fit of y.  The solve takes the Gram of a row's n_obs samples as the
    whole-call Gram minus a correction (every route, pgh_glm's included), which costs a factor n_S / n_obs of the
    doubles' 1.1e-16 -- about 7e-14 for 6 of 3,800 samples -- and the residual sum of squares is what is left of the
    total after the fit, so its relative error is that over rss / tss.  Above RSS_FLOOR the contract's 1e-9 has a
    margin of ten; a fit with one or two degrees of freedom falls below it by chance (rss / tss = 4e-8 was drawn, and
    there pgh_glm and pgh_glm_sparse themselves differ by 1.6e-6), so such a draw is not an input for a 1e-9 check."""
    O = _oracle()
    for x in x_small:
        row = O.oracle_row(x, y, Z, "linear")
        if row["errcode"] is None and row["rss"] < RSS_FLOOR * row["tss"]:
            return False
    return True


def _phenotype(rng, n, Z, gain, pattern, x=None):
    """One quantitative phenotype with a signal from the covariates, NaN at `pattern`; drawn again until it is well
    conditioned on the rows of x (values, -9 = missing) with at most SMALL_ROW called samples, the only ones with few
    degrees of freedom."""
    x_small = [] if x is None else x[(x != -9.0).sum(axis=1) <= SMALL_ROW]
    for _ in range(200):
        y = gain * 0.3 * (Z.sum(axis=0) if Z.shape[0] else np.zeros(n)) + rng.normal(size=n)
        y[pattern] = NAN
        if _well_conditioned(y, Z, x_small):
            return y
    raise AssertionError("no well-conditioned phenotype in 200 draws")


def _phenotypes(rng, n, Z, count, missing=0.03, x=None):
    """count phenotypes, each with its own missing pattern."""
    return np.stack([_phenotype(rng, n, Z, gain, rng.random(n) < missing, x) for gain in np.linspace(0.5, 1.5, count)])


@functools.lru_cache(maxsize=None)
def parity_inputs(n, k):
    """Z and five phenotypes: 0 and 1 share a missing pattern, 2 and 3 have their own, 4 has no missing value."""
    rng = np.random.default_rng(100 * n + k + 7)
    x = _values(_geno(M_R, n, n)[0])
    Z = _covariates(rng, k, n)
    pat_a, pat_b, pat_c = (rng.random(n) < rate for rate in (0.03, 0.08, 0.2))
    none = np.zeros(n, dtype=bool)
    Y = np.stack([_phenotype(rng, n, Z, gain, pat, x)
                  for gain, pat in zip(np.linspace(0.5, 1.5, 5), (pat_a, pat_a, pat_b, pat_c, none))])
    Y.setflags(write=False)
    Z.setflags(write=False)
    return Z, Y


@functools.lru_cache(maxsize=None)
def wide_inputs():
    """n = 257, k = 2 and 70 phenotypes with 5 % missing each: more than a block of 64."""
    n = 257
    rng = np.random.default_rng(2570)
    x = _values(_geno(M_R, n, n)[0])
    Z = _covariates(rng, 2, n)
    Y = _phenotypes(rng, n, Z, 70, missing=0.05, x=x)
    Y.setflags(write=False)
    Z.setflags(write=False)
    return Z, Y


def _decision_inputs():
    """n = 64, eight rows (tests/test_glm_sparse.py's decision rows) and five phenotypes, one per decision:
    0: its carriers of rows 0..2 have no value (CONST_ALLELE, with and without covariates), row 3 has k + 2 = 3 used
       samples (TOO_FEW_SAMPLES), row 5 is the covariate itself (SINGULAR_MATRIX);
    1: values at those carriers, so rows 0 and 1 are fitted for it;
    2: three values in all: TOO_FEW_SAMPLES with a covariate wherever its neighbours are fitted;
    3: exactly linear in x and z with a residual that is exactly zero in floating point -- a constant, slope 0 -- so
       every row that reaches the fit is ZERO_VARIANCE with beta filled;
    4: no value at the called samples of rows 3 and 4: all missing within S_p (TOO_FEW_SAMPLES, obs_ct 0)."""
    n = 64
    rng = np.random.default_rng(5)
    y = rng.normal(size=n)
    no_pheno = np.array([3, 17, 40])
    y[no_pheno] = NAN
    geno = np.zeros((8, n), dtype=np.uint8)
    geno[0, no_pheno] = 1                        # every sample with phenotype 0 is hom-ref
    geno[1, 17] = 2                              # a singleton whose carrier has no phenotype 0
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
    y1 = rng.normal(size=n)
    y1[[20, 33]] = NAN
    y2 = np.full(n, NAN)
    y2[[1, 2, 5]] = [0.5, -1.0, 2.0]
    y3 = np.full(n, 2.0)
    y3[[4, 30, 41]] = NAN
    y4 = rng.normal(size=n)
    y4[[1, 2, 5, 9]] = NAN
    return geno, np.stack([y, y1, y2, y3, y4]), geno[5].astype(np.float64)[None, :]


DECISION_CLAIMS = {  # (k, phenotype) -> the errcodes of the eight rows
    (1, 0): ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None, "SINGULAR_MATRIX", None,
             "CONST_ALLELE"],
    (1, 2): ["TOO_FEW_SAMPLES"] * 8,
    (0, 0): ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", None, None, None, None, "CONST_ALLELE"],
}


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_sparse_multi(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_sparse_multi")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_sparse_multi_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape check runs before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_sparse_multi(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_sparse_multi(fake, np.zeros((2, 5)), np.zeros((2, 4)))


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_have_fitted_rows_and_distinct_patterns(n, k):
    O = _oracle()
    Z, Y = parity_inputs(n, k)
    x = _values(_geno(M_R, n, n)[0])
    pats = [np.isnan(y) for y in Y]
    assert np.array_equal(pats[0], pats[1]) and pats[0].any()
    assert len({p.tobytes() for p in pats}) >= 4 and not pats[4].any()
    for p, y in enumerate(Y):
        fitted = sum(O.oracle_row(x[i], y, Z, "linear")["errcode"] is None for i in PARITY_ROWS)
        assert 2 * fitted >= len(PARITY_ROWS), (n, k, p, fitted)


def test_the_decision_file_reaches_every_errcode_it_claims():
    O = _oracle()
    geno, Y, Z = _decision_inputs()
    x = _values(geno)
    codes = {(k, p): [O.oracle_row(r, Y[p], Z[:k], "linear")["errcode"] for r in x] for k in (0, 1) for p in range(len(Y))}
    for key, claim in DECISION_CLAIMS.items():
        assert codes[key] == claim, key
    assert codes[(1, 1)][:2] == [None, None]                         # fitted where phenotype 0 is constant
    assert codes[(1, 2)][6] == "TOO_FEW_SAMPLES" and codes[(1, 1)][6] is None   # three values beside a fitted neighbour
    zero = codes[(1, 3)]
    assert zero[6] == "ZERO_VARIANCE" and zero[4] == "ZERO_VARIANCE"
    assert np.isfinite(O.oracle_row(x[6], Y[3], Z, "linear")["beta"])
    rows34 = [O.oracle_row(x[i], Y[4], Z, "linear") for i in (3, 4)]
    assert [r["errcode"] for r in rows34] == ["TOO_FEW_SAMPLES"] * 2 and [r["obs_ct"] for r in rows34] == [0, 0]
    assert codes[(1, 4)][6] is None


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _same(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _close(a, b, rel=REL, ctx=None):
    """The linear contract (tests/test_glm_sparse.py): errcode, obs_ct, firth and a1_freq equal; the estimates within
    rel, on check_rows' scale (beta relative to |beta| + SE, the statistic to |t| + 1)."""
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


def _col(out, p, rows=slice(None)):
    return {key: v[rows, p] for key, v in out.items()}


def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


def _minor(geno):
    return geno.shape[1] - np.array([np.bincount(r, minlength=4).max() for r in geno])


class _File:
    """test_glm_sparse._File: a .pgen of every record type, its dense dataset and its calls."""

    def __init__(self, L, tmp, m, n, seed, codes=None, name="rare"):
        self.L, self.m, self.n = L, m, n
        if codes is None:
            self.geno, self.kinds = _geno(m, n, seed)
        else:
            self.geno, self.kinds = codes, W.choose_kinds(codes, np.random.default_rng(seed))
        self.path = str(tmp / f"{name}_{n}.pgen")
        W.write_pgen(self.path, self.geno, self.kinds)
        self.dense = L.Dataset.open(self.path)
        self.x = _values(self.geno)

    def sparse(self, window_rows=97, **kw):
        # several windows per open, so that parts are concatenated and windows start after LD bases
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(WINDOW_ENV, str(window_rows * self.dense.info.pitch_bytes))
            return self.L.Dataset.open(self.path, sparse=True, **kw)


@pytest.fixture(scope="module")
def rare_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_sparse_multi")
    return {n: _File(gpu_lib, tmp, M_R, n, n) for n in PARITY_N}


@pytest.fixture(scope="module")
def hard_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_sparse_multi_hard")
    return {n: _File(gpu_lib, tmp, SS.M, n, n, codes=SS.hard_codes(n), name="hard") for n in EDGE_N + (SS.N_SMALL,)}


def _against_the_singles(sp, Y, zc, got, subset=None, ctx=None):
    for p, y in enumerate(Y):
        _close(_col(got, p), sp.glm_sparse(y, zc, subset=subset), ctx=(ctx, "single", p))


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_singles_the_dense_form_and_the_oracle(gpu_lib, rare_files, n, k):
    f = rare_files[n]
    Z, Y = parity_inputs(n, k)
    zc = Z if k else None
    want = [f.dense.glm(y, zc, model="linear") for y in Y]
    minor = _minor(f.geno)
    for max_minor in (0, 1, n):
        sp = f.sparse(max_minor=max_minor)
        info = sp.sparse_info()
        got = sp.glm_sparse_multi(Y, zc)
        assert got["beta"].shape == (M_R, len(Y))
        _against_the_singles(sp, Y, zc, got, ctx=(n, k, max_minor))
        for p, y in enumerate(Y):
            _close(_col(got, p), want[p], ctx=(n, k, max_minor, "dense", p))
            fitted = _oracle().check_rows(_col(got, p, PARITY_ROWS), f.x[PARITY_ROWS], y, Z, "linear", rel=REL)
            assert 2 * fitted >= len(PARITY_ROWS)
        if max_minor == n:
            # het-, hom-alt- and missing-majority rows all run from their entries
            assert info.dense_variant_ct == 0 and all(info.base_hist[b] > 0 for b in (1, 2, 3))
            if n == 4099:  # both sides of the group / workgroup threshold
                assert (minor > 1024).any() and ((minor > 0) & (minor <= 1024)).any()
        if max_minor == 1:
            assert info.dense_variant_ct > 0 and info.sparse_variant_ct > 0
        sp.close()


@pytest.mark.gpu
def test_every_group_width_and_the_block_edge(gpu_lib, rare_files):
    f = rare_files[257]
    Z, Y70 = wide_inputs()
    sp = f.sparse(max_minor=f.n)
    singles = [sp.glm_sparse(y, Z) for y in Y70]
    assert all((s["errcode"] == None).sum() > M_R // 3 for s in singles)  # noqa: E711
    wide = None
    for P in GROUP_P:
        got = sp.glm_sparse_multi(Y70[:P], Z)
        assert got["beta"].shape == (M_R, P)
        for p in range(P):
            _close(_col(got, p), singles[p], ctx=(P, p))
        wide = got
    reverse = sp.glm_sparse_multi(Y70[::-1], Z)
    for p in range(70):
        _same(_col(sp.glm_sparse_multi(Y70[p:p + 1], Z), 0), _col(wide, p), ctx=("alone", p))
        _same(_col(reverse, 69 - p), _col(wide, p), ctx=("reversed", p))
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kp", WIDTHS)
def test_every_instantiated_width(gpu_lib, rare_files, kp):
    """k = kp and kp - 1 for every width GlmPadCovar returns (kp = 1 covers the width 0).  With 20 covariates most of
    the file's small rows have a handful of degrees of freedom, so the phenotypes are conditioned on the rows that go
    to the oracle; the singles share the call's parameterisation and differ from it in the order of the sums only."""
    f = rare_files[4099]
    idx = sorted(set(range(5, M_R, 55)) | set(HET_ROWS))[:12]
    sp = f.sparse(max_minor=f.n)
    assert sp.sparse_info().dense_variant_ct == 0
    for k in (kp, kp - 1):
        rng = np.random.default_rng(3100 + k)
        Z = _covariates(rng, k, f.n)
        Y = _phenotypes(rng, f.n, Z, 3, x=f.x[idx])
        zc = Z if k else None
        got = sp.glm_sparse_multi(Y, zc)
        _against_the_singles(sp, Y, zc, got, ctx=k)
        for p, y in enumerate(Y):
            _oracle().check_rows(_col(got, p, idx), f.x[idx], y, Z, "linear", rel=REL)
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_minor", [0, 257])
def test_a_row_does_not_depend_on_anything_but_its_own_inputs(gpu_lib, rare_files, max_minor):
    """Bit for bit: the range, the window the dataset was opened with, the scratch budget (several chunks, and blocks
    smaller than 64 at P = 70) and a repeat.  max_minor = 0: every row with a carrier is walked from its pool row."""
    f = rare_files[257]
    Z, Y = wide_inputs()
    sp = f.sparse(max_minor=max_minor)
    whole = sp.glm_sparse_multi(Y, Z)
    assert (whole["errcode"] == None).sum() > M_R * len(Y) // 3  # noqa: E711
    again = sp.glm_sparse_multi(Y, Z)
    _same(again, whole, ctx="again")
    assert again["beta"].tobytes() == whole["beta"].tobytes()
    _same(sp.glm_sparse_multi(Y, Z, v_begin=37), _rows(whole, slice(37, M_R)), ctx="v_begin = 37")
    _same(sp.glm_sparse_multi(Y, Z, v_begin=37, v_end=333), _rows(whole, slice(37, 333)), ctx="range")
    # another window size, and a window that starts after an LD base
    other = f.sparse(window_rows=41, max_minor=max_minor)
    _same(other.glm_sparse_multi(Y, Z), whole, ctx="window bytes")
    other.close()
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))
    v1 = min(M_R, v0 + 150)
    part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
    _same(part.glm_sparse_multi(Y, Z), _rows(whole, slice(v0, v1)), ctx=("window", v0))
    part.close()
    # A block phenotype takes 8 bytes x (257 raw + 257 subset) samples = 4,112 bytes, a chunk variant 160 bytes per
    # phenotype (k = 2: 6 sums, 10 entries of the correction Gram and a 32-byte row) and a 4-byte count.  1 byte: one
    # phenotype per block, chunks of one variant.  240,000 bytes: fewer than 64 phenotypes fit beside one variant
    # (64 x 4,272 = 273,408), so 70 phenotypes take blocks smaller than 64, and what is left holds a few variants.
    for budget in (1, 240_000):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(sp.glm_sparse_multi(Y, Z, v_begin=200, v_end=230), _rows(whole, slice(200, 230)), ctx=budget)
    empty = sp.glm_sparse_multi(Y, Z, v_begin=77, v_end=77)
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
    Y = _phenotypes(rng, n, Z, 3, x=f.x)
    assert len({np.isnan(y).tobytes() for y in Y}) == 3
    sp = f.sparse(max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    got = sp.glm_sparse_multi(Y, Z)
    _against_the_singles(sp, Y, Z, got)
    # the longest entry lists, the longest missing lists, the het-majority rows and a spread: 16 rows
    idx = list(dict.fromkeys(np.argsort(entries)[-5:].tolist() + np.argsort(in_missing_list)[-3:].tolist()
                             + list(HET_ROWS) + list(range(3, m, 9))))[:16]
    assert len(idx) == 16
    for p, y in enumerate(Y):
        _oracle().check_rows(_col(got, p, idx), f.x[idx], y, Z, "linear", rel=REL)
    sp.close()
    f.dense.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("n", EDGE_N)
def test_sample_counts_at_a_64_sample_edge(gpu_lib, hard_files, n, k):
    f = hard_files[n]
    rng = np.random.default_rng(900 + 10 * n + k)
    Z = _covariates(rng, k, n)
    Y = _phenotypes(rng, n, Z, 3, missing=0.06, x=f.x)
    zc = Z if k else None
    for max_minor in (0, n):
        sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=max_minor)
        got = sp.glm_sparse_multi(Y, zc)
        assert got["beta"].shape == (SS.M, len(Y))
        _against_the_singles(sp, Y, zc, got, ctx=(n, k, max_minor))
        for p, y in enumerate(Y):
            _close(_col(got, p), f.dense.glm(y, zc, model="linear"), ctx=(n, k, max_minor, "dense", p))
            fitted = _oracle().check_rows(_col(got, p), f.x, y, Z, "linear", rel=REL, idx=range(0, SS.M, 5))
            assert fitted >= 20
        assert got["errcode"][SS.ROW_ALL_MISSING].tolist() == ["TOO_FEW_SAMPLES"] * len(Y)
        assert got["errcode"][SS.ROW_MONO].tolist() == ["CONST_ALLELE"] * len(Y)
        sp.close()


def _subset_case(sp, dense, x, mask, ctx):
    n_out = int(mask.sum())
    rng = np.random.default_rng(7 + n_out)
    k = 2
    Z = _covariates(rng, k, n_out)
    Y = _phenotypes(rng, n_out, Z, 3, missing=0.04, x=x[:, mask])
    assert len({np.isnan(y).tobytes() for y in Y}) == 3
    ss, ss_d = sp.subset(mask), dense.subset(mask)
    got = sp.glm_sparse_multi(Y, Z, subset=ss)
    _against_the_singles(sp, Y, Z, got, subset=ss, ctx=ctx)
    idx = range(0, x.shape[0], 7)
    total = 0
    for p, y in enumerate(Y):
        _close(_col(got, p), dense.glm(y, Z, model="linear", subset=ss_d), ctx=(ctx, "dense", p))
        total += _oracle().check_rows(_col(got, p), x[:, mask], y, Z, "linear", rel=REL, idx=idx)
    assert total > len(idx)
    ss.close()
    ss_d.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, rare_files):
    f = rare_files[4099]
    keep = np.random.default_rng(12).random(f.n) < 0.5
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        _subset_case(sp, f.dense, f.x, keep, ("plain", max_minor))
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["all_but_one", "last_word", "word_block", "tile_plus_one", "stride4"])
def test_structured_sample_subsets(gpu_lib, hard_files, shape):
    f = hard_files[SS.N_SMALL]
    sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=f.n)
    _subset_case(sp, f.dense, f.x, SS.shapes(f.n)[shape], shape)
    sp.close()


@pytest.mark.gpu
def test_decisions(gpu_lib, tmp_path):
    L = gpu_lib
    O = _oracle()
    geno, Y, Z = _decision_inputs()
    n = geno.shape[1]
    path = str(tmp_path / "decisions.pgen")
    W.write_pgen(path, geno, [0] * len(geno))
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True, max_minor=n)
    assert sp.sparse_info().dense_variant_ct == 0
    x = _values(geno)
    for k in (1, 0):
        zc = Z[:k] if k else None
        got = sp.glm_sparse_multi(Y, zc)
        for p, y in enumerate(Y):
            col = _col(got, p)
            want = dense.glm(y, zc, model="linear")
            exp = [O.oracle_row(r, y, Z[:k], "linear") for r in x]
            assert list(col["errcode"]) == list(want["errcode"]) == [e["errcode"] for e in exp], (k, p)
            assert col["obs_ct"].tolist() == want["obs_ct"].tolist() == [e["obs_ct"] for e in exp], (k, p)
            assert np.array_equal(col["a1_freq"], want["a1_freq"], equal_nan=True), (k, p)
            if (k, p) in DECISION_CLAIMS:
                assert list(col["errcode"]) == DECISION_CLAIMS[(k, p)], (k, p)
            _close(col, sp.glm_sparse(y, zc), ctx=(k, p))
            if p != 3:
                O.check_rows(col, x, y, Z[:k], "linear", rel=REL)
        zero = _col(got, 3)
        assert zero["errcode"][6] == "ZERO_VARIANCE" and np.isfinite(zero["beta"][6]) and np.isnan(zero["se"][6])
    # a covariate that duplicates another over the samples of phenotype 0 alone
    rng = np.random.default_rng(6)
    z2 = rng.normal(size=n)
    dup = np.where(np.isnan(Y[0]), z2, Z[0])
    bad = np.stack([Z[0], dup])
    got = sp.glm_sparse_multi(Y[:2], bad)
    for p in range(2):
        want = dense.glm(Y[p], bad, model="linear")
        assert list(got["errcode"][:, p]) == list(want["errcode"]), p
        assert got["obs_ct"][:, p].tolist() == want["obs_ct"].tolist()
        assert np.array_equal(got["a1_freq"][:, p], want["a1_freq"], equal_nan=True)
    # (row 4 has four used samples: too few beside two covariates)
    assert list(got["errcode"][[4, 6], 0]) == ["TOO_FEW_SAMPLES", "SINGULAR_MATRIX"]
    assert list(got["errcode"][[0, 6], 1]) == [None, None]
    sp.close()
    dense.close()


@pytest.mark.gpu
def test_a_phenotype_that_is_all_nan_decides_only_its_own_column(gpu_lib, rare_files):
    f = rare_files[257]
    Z, Y = parity_inputs(257, 3)
    sp = f.sparse(max_minor=f.n)
    three = np.stack([Y[0], np.full(f.n, NAN), Y[2]])
    got = sp.glm_sparse_multi(three, Z)
    assert set(got["errcode"][:, 1]) == {"TOO_FEW_SAMPLES"} and not got["obs_ct"][:, 1].any()
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.isnan(got[key][:, 1]).all(), key
    _same(_col(got, 1), sp.glm_sparse(three[1], Z))
    pair = sp.glm_sparse_multi(three[[0, 2]], Z)
    _same(_col(got, 0), _col(pair, 0))
    _same(_col(got, 2), _col(pair, 1))
    assert (got["errcode"][:, 0] == None).sum() > M_R // 3  # noqa: E711
    alone = sp.glm_sparse_multi(three[1:2], Z)
    assert set(alone["errcode"][:, 0]) == {"TOO_FEW_SAMPLES"}
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
    y = np.arange(n, dtype=np.float64) % 3
    Y = np.stack([y, np.sqrt(np.arange(n, dtype=np.float64))])
    assert sp.glm_sparse_multi(Y, v_begin=0, v_end=8)["errcode"].shape == (8, 2)

    def raw(ds, phen, n_pheno=None, z=None, n_covar=0, v0=0, v1=8, subset=None, null_out=False):
        out = np.full(32 * max(1, v1 - v0) * max(1, len(phen)), 0xAB, dtype=np.uint8)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        rc = L.raw().pgh_glm_sparse_multi(ds._h, subset, v0, v1, len(phen) if n_pheno is None else n_pheno, p(phen),
                                          n_covar, p(z), None if null_out else p(out), eb)
        return rc, eb.value.decode(), bool((out == 0xAB).all())

    inf = np.zeros((2, n))
    inf[1, 5] = np.inf
    other = dense.subset(np.arange(n) % 2 == 0)
    cases = [
        ("at least one phenotype", (sp, Y, 0)),
        ("needs a sparse-resident dataset", (dense, Y)),
        ("one device's dataset", (group, Y)),
        ("at most 20 covariates", (sp, Y, None, np.zeros((21, n)), 21)),
        ("covariate 1 is not finite at sample 5", (sp, Y, None, inf, 2)),
        ("null argument", (sp, Y, None, None, 2)),
        ("null argument", (sp, Y, None, None, 0, 0, 8, None, True)),
        ("outside the resident range", (sp, Y, None, None, 0, 0, m + 1)),
        ("outside the resident range", (sp, Y, None, None, 0, 9, 8)),
        ("different dataset", (sp, Y[:, ::2], None, None, 0, 0, 8, other._h)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_sparse_multi(Y, v_begin=0, v_end=8)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.glm_multi(Y, v_begin=0, v_end=8)
    # an empty range is fine
    rc, msg, untouched = raw(sp, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched
    assert sp.glm_sparse_multi(Y, v_begin=3, v_end=3)["errcode"].shape == (0, 2)
    other.close()
    for ds in (group, sp, dense):
        ds.close()
