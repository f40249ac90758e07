"""pgh_glm_score_multi / Dataset.glm_score_multi: the logistic score test over a dense-resident dataset for many
phenotypes in one call, on the FP64 matrix cores.  Every column is checked against the FP64 oracle of the sparse route
(tests/glm_score_oracle.py) within test_glm_score_sparse's 1e-9 on check_rows' scale; obs_ct, a1_freq and the count
decisions equal pgh_glm's logistic fit bit for bit; the sparse route over the same file agrees within 2e-9 (two
results, each within 1e-9 of the oracle); and a row does not depend on the other phenotypes, its place among them,
the range, the window, the phenotype block, the variant chunk or the scratch budget: bit for bit."""

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
import variant_shapes as VS

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_multi"]
REL = 1e-9          # test_glm_score_sparse.REL
M = 323
PHENO_BLOCK = 64    # kGlmScoreDensePb: the phenotypes of one column block at most
VARIANT_TILE = 128  # kGlmScoreDenseTileV: the variants of one workgroup of the contraction
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
# (case rate, NaN rate) of the five phenotypes; a sixth shares the first one's NaN pattern
PHENO_SPECS = ((0.2, 0.03), (0.5, 0.0), (0.05, 0.1), (0.35, 0.03), (0.1, 0.3))
STRIDE7 = list(range(0, M, 7))
MADE = [SS.ROW_ALL_MISSING, SS.ROW_MONO, SS.ROW_BLOCK]
# every padded covariate width of kGlmWidths at its exact value and one above the bucket below it
# (test_glm_widths_chunks.WIDTHS without the k = 1 of test_parity_with_the_oracle)
WIDTHS = [2, 4, 5, 8, 9, 12, 13, 16, 17, 20]
WIDTHS_N = 4099
WIDTHS_ROWS = MADE + list(range(0, M, 23))
# (k, what 17 phenotypes of k + 2 x-columns each do to the 16-column blocks)
LAYOUTS = [(14, "a phenotype is one block"), (13, "every phenotype after the first straddles a block edge")]
LAYOUT_PHENOTYPES = 17  # one more than the 16 squared-weight columns of a block: two such blocks
# sample counts at and next to a 64-sample edge (words16 = ceil(n / 64), B padded to 64, the mask zero past n)
EDGE_N = (63, 64, 65, 128)
EDGE_K = (0, 2)
EDGE_M = SS.M
EDGE_SPECS = ((0.5, 0.03), (0.35, 0.03))


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_multi(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_multi")
    assert SCRATCH_ENV in header
    kernels = open(os.path.join(ROOT, "plinking_duck_amd", "csrc", "glm.hpp")).read()
    assert f"kGlmScoreDensePb = {PHENO_BLOCK};" in kernels and f"kGlmScoreDenseTileV = {VARIANT_TILE};" in kernels


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_multi_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def test_a_null_dataset_is_refused_with_out_untouched(lib):
    out = np.full(32 * 4, 0xAB, dtype=np.uint8)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    rc = lib.raw().pgh_glm_score_multi(None, None, 0, 4, 1, y.ctypes.data_as(C.c_void_p), 0, None,
                                       out.ctypes.data_as(C.c_void_p), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and (out == 0xAB).all()


# ---- helpers -----------------------------------------------------------------------------------------------------

def _covariates(rng, k, n):
    """test_glm_score_sparse._covariates"""
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def _phenotypes(rng, n, Z, specs=PHENO_SPECS):
    ys = [O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in specs]
    shared = O.pheno(rng, n, Z, case_rate=0.3, missing=0.0)
    shared[np.isnan(ys[0])] = NAN
    return np.stack(ys + [shared])


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
    """test_glm_score_sparse._close"""
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


def _counts_equal_the_dense_logistic_fit(got, want, ctx=None):
    """test_glm_score_sparse._counts_equal_the_dense_logistic_fit"""
    assert got["obs_ct"].tolist() == want["obs_ct"].tolist(), ctx
    assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True), ctx
    for code in ("TOO_FEW_SAMPLES", "CONST_ALLELE"):
        assert (got["errcode"] == code).tolist() == (want["errcode"] == code).tolist(), (code, ctx)
    assert not got["firth"].any(), ctx


@functools.lru_cache(maxsize=None)
def _hard_codes(n, m):
    return SS.hard_codes(n, m=m)


@functools.lru_cache(maxsize=None)
def width_inputs(k):
    """(Z, Y) of the width cases: test_parity_with_the_oracle's draw at n = 4099, the six phenotypes."""
    rng = np.random.default_rng(100 * WIDTHS_N + k)
    Z = _covariates(rng, k, WIDTHS_N)
    return Z, _phenotypes(rng, WIDTHS_N, Z)


@functools.lru_cache(maxsize=None)
def layout_inputs(k):
    """(Z, Y): the six phenotypes of width_inputs in turn at positions 0..15, and at 16 one of its own."""
    Z, six = width_inputs(k)
    own = O.pheno(np.random.default_rng(17_000 + k), WIDTHS_N, Z, case_rate=0.25, missing=0.05)
    Y = np.stack([six[i % len(six)] for i in range(LAYOUT_PHENOTYPES - 1)] + [own])
    return Z, Y


@functools.lru_cache(maxsize=None)
def edge_inputs(n, k):
    """(Z, Y) of the sample-count edges: case rates 0.5 and 0.35, 3 % NaN."""
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    return Z, np.stack([O.pheno(rng, n, Z, case_rate=c, missing=m) for c, m in EDGE_SPECS])


# ---- no device: conditions on the inputs ------------------------------------------------------------------------

@pytest.mark.parametrize("k", WIDTHS + [k for k, _ in LAYOUTS])
def test_the_width_inputs_have_fitted_null_models_and_fitted_rows(k):
    """So that a GPU case cannot pass on rows that are not fitted: every null model converges, and the oracle fits
    more than half of the chosen rows of every phenotype that is compared with it."""
    x = SS.values(_hard_codes(WIDTHS_N, M))
    Z, Y = layout_inputs(k) if k in dict(LAYOUTS) else width_inputs(k)
    assert len(set(y.tobytes() for y in Y)) == (7 if k in dict(LAYOUTS) else 6)
    for p, y in enumerate(Y):
        if p >= 6 and p != LAYOUT_PHENOTYPES - 1:
            continue  # a copy
        nul = O.Null(y, Z)
        assert nul.status is None, (k, p, nul.status)
        fitted = sum(O.oracle_row(x[i], nul)["errcode"] is None for i in WIDTHS_ROWS)
        assert fitted > len(WIDTHS_ROWS) // 2, (k, p, fitted)


@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("n", EDGE_N)
def test_the_sample_count_edges_have_fitted_null_models_and_fitted_rows(n, k):
    x = SS.values(_hard_codes(n, EDGE_M))
    Z, Y = edge_inputs(n, k)
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None, (n, k, p, nul.status)
        fitted = sum(O.oracle_row(x[i], nul)["errcode"] is None for i in range(EDGE_M))
        assert fitted >= 120, (n, k, p, fitted)


class _File:
    def __init__(self, L, tmp, name, codes, seed):
        self.codes, self.n = codes, codes.shape[1]
        self.x = SS.values(codes)
        self.path = str(tmp / f"{name}_{self.n}.pgen")
        W.write_pgen(self.path, codes, W.choose_kinds(codes, np.random.default_rng(seed)))
        self.ds = L.Dataset.open(self.path)


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi")
    out = {}
    for n in (257, 1003, 4099):
        out["hard", n] = _File(gpu_lib, tmp, "hard", SS.hard_codes(n, m=M), n)
        out["rare", n] = _File(gpu_lib, tmp, "rare", W.rare_matrix(M, n, np.random.default_rng(n)), n)
    return out


@pytest.fixture(scope="module")
def case_1003(files):
    """The file, covariates, phenotypes and whole-range result that the bit-for-bit tests share."""
    f = files["hard", 1003]
    rng = np.random.default_rng(1003)
    Z = _covariates(rng, 3, f.n)
    Y = _phenotypes(rng, f.n, Z)
    return types.SimpleNamespace(f=f, Z=Z, Y=Y, whole=f.ds.glm_score_multi(Y, Z))


# ---- on the GPU --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 3, 20])
@pytest.mark.parametrize("n", [257, 1003, 4099])
@pytest.mark.parametrize("kind", ["hard", "rare"])
def test_parity_with_the_oracle(gpu_lib, files, kind, n, k):
    """Rows 3, 4, 5 and every 7th row, per phenotype.  Also items 2 and 3 of the same call: the counts equal pgh_glm's
    logistic fit, and (k = 3) the sparse route over the same file agrees within 2 REL."""
    f = files[kind, n]
    rng = np.random.default_rng(100 * n + k)
    Z = _covariates(rng, k, n)
    Y = _phenotypes(rng, n, Z)
    zc = Z if k else None
    got = f.ds.glm_score_multi(Y, zc)
    assert got["beta"].shape == (M, len(Y))
    worst_all = 0.0
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        col = _col(got, p)
        fitted, worst = O.check_rows(col, f.x, nul, rel=REL, idx=STRIDE7)
        _, worst_made = O.check_rows(col, f.x, nul, rel=REL, idx=MADE)
        worst_all = max(worst_all, worst, worst_made)
        print(f"{kind} n={n} k={k} phenotype {p}: {fitted} fitted of {len(STRIDE7)}, worst {max(worst, worst_made):.3g}")
        if kind == "hard":
            assert fitted >= 40, (p, fitted, nul.status)
        else:
            assert fitted > len(STRIDE7) // 3, (p, fitted, nul.status)
        _counts_equal_the_dense_logistic_fit(col, f.ds.glm(y, zc, model="logistic", firth=False), ctx=(kind, n, k, p))
    if kind == "hard":
        assert got["errcode"][SS.ROW_ALL_MISSING].tolist() == ["TOO_FEW_SAMPLES"] * len(Y)
        assert got["errcode"][SS.ROW_MONO].tolist() == ["CONST_ALLELE"] * len(Y)
    print(f"{kind} n={n} k={k}: worst difference {worst_all:.3g}")
    if k == 3:
        for max_minor in (0, n):
            sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=max_minor)
            for p, y in enumerate(Y):
                _close(_col(got, p), sp.glm_score_sparse(y, zc), 2 * REL, ctx=(kind, n, max_minor, p))
            sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """The column layout p (k + 2), the epilogue's column -> (phenotype, slot) map and GlmScoreDenseCorrKernel's rows of
    k + 3 for every width GlmPadCovar returns, at k = KP and one above the width below: the made rows and every 23rd
    row of every phenotype against the oracle, and the counts of one phenotype against pgh_glm's logistic fit."""
    f = files["hard", WIDTHS_N]
    Z, Y = width_inputs(k)
    got = f.ds.glm_score_multi(Y, Z)
    assert got["beta"].shape == (M, len(Y))
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        fitted, worst = O.check_rows(_col(got, p), f.x, nul, rel=REL, idx=WIDTHS_ROWS)
        print(f"k={k} phenotype {p}: {fitted} fitted of {len(WIDTHS_ROWS)}, worst {worst:.3g}")
        assert fitted > len(WIDTHS_ROWS) // 2, (k, p, fitted, nul.status)
    p = k % len(Y)
    _counts_equal_the_dense_logistic_fit(_col(got, p), f.ds.glm(Y[p], Z, model="logistic", firth=False), ctx=(k, p))


@pytest.mark.gpu
@pytest.mark.parametrize("k,what", LAYOUTS)
def test_phenotypes_at_and_across_the_column_blocks(gpu_lib, files, k, what):
    """17 phenotypes, two blocks of squared-weight columns.  k = 14: the k + 2 x-columns of a phenotype are exactly one
    16-column block; k = 13: 15 columns, so every phenotype after the first straddles a block edge.  The last
    phenotype, which is no copy of another, and the first and the sixteenth against the oracle; every copy equals
    its original bit for bit."""
    f = files["hard", WIDTHS_N]
    Z, Y = layout_inputs(k)
    assert len(Y) == LAYOUT_PHENOTYPES and (len(Y) * (k + 2) + 15) // 16 >= 16
    got = f.ds.glm_score_multi(Y, Z)
    for p in (0, LAYOUT_PHENOTYPES - 2, LAYOUT_PHENOTYPES - 1):
        nul = O.Null(Y[p], Z)
        fitted, worst = O.check_rows(_col(got, p), f.x, nul, rel=REL, idx=WIDTHS_ROWS)
        print(f"k={k} phenotype {p}: {fitted} fitted of {len(WIDTHS_ROWS)}, worst {worst:.3g}")
        assert fitted > len(WIDTHS_ROWS) // 2, (k, p, fitted, nul.status)
    for p in range(6, LAYOUT_PHENOTYPES - 1):
        _same(_col(got, p), _col(got, p % 6), ctx=(k, p))
    assert not np.array_equal(got["beta"][:, LAYOUT_PHENOTYPES - 1], got["beta"][:, 0], equal_nan=True)


@pytest.fixture(scope="module")
def edge_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_edges")
    return {n: _File(gpu_lib, tmp, "edge", _hard_codes(n, EDGE_M), n) for n in EDGE_N}


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
@pytest.mark.parametrize("n", EDGE_N)
def test_sample_counts_at_a_64_sample_edge(gpu_lib, edge_files, n, k):
    """words16 = ceil(n / 64), B padded to 64-sample steps and a mask that is zero past the last sample: every row of
    both phenotypes against the oracle, and the counts against pgh_glm's logistic fit."""
    f = edge_files[n]
    Z, Y = edge_inputs(n, k)
    zc = Z if k else None
    got = f.ds.glm_score_multi(Y, zc)
    assert got["beta"].shape == (EDGE_M, len(Y))
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        fitted, worst = O.check_rows(_col(got, p), f.x, nul, rel=REL)
        print(f"n={n} k={k} phenotype {p}: {fitted} fitted of {EDGE_M}, worst {worst:.3g}")
        assert fitted >= 120, (n, k, p, fitted, nul.status)
        want = f.ds.glm(y, zc, model="logistic", firth=False)
        _counts_equal_the_dense_logistic_fit(_col(got, p), want, ctx=(n, k, p))
    assert got["errcode"][SS.ROW_ALL_MISSING].tolist() == ["TOO_FEW_SAMPLES"] * len(Y)
    assert got["errcode"][SS.ROW_MONO].tolist() == ["CONST_ALLELE"] * len(Y)


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_other_phenotypes_or_its_place(gpu_lib, case_1003):
    c = case_1003
    ds, Y, Z, whole = c.f.ds, c.Y, c.Z, c.whole
    assert (whole["errcode"] == None).sum() > M * len(Y) // 2  # noqa: E711
    _same(ds.glm_score_multi(Y, Z), whole, ctx="again")
    for p in range(len(Y)):
        _same(_col(ds.glm_score_multi(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))
    rev = ds.glm_score_multi(Y[::-1], Z)
    for p in range(len(Y)):
        _same(_col(rev, len(Y) - 1 - p), _col(whole, p), ctx=("reversed", p))
    # at position 23 of 40, among copies of the others
    filler = np.stack([Y[(i * 5 + 1) % len(Y)] for i in range(40)])
    for p in (0, 2):
        many = filler.copy()
        many[23] = Y[p]
        _same(_col(ds.glm_score_multi(many, Z), 23), _col(whole, p), ctx=("23 of 40", p))


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_or_the_window(gpu_lib, case_1003):
    c = case_1003
    lo, hi = VS.WINDOW
    _same(c.f.ds.glm_score_multi(c.Y, c.Z, v_begin=lo, v_end=hi), _rows(c.whole, slice(lo, hi)), ctx="range")
    part = gpu_lib.Dataset.open(c.f.path, variant_begin=lo, variant_end=hi)
    _same(part.glm_score_multi(c.Y, c.Z), _rows(c.whole, slice(lo, hi)), ctx="window")
    part.close()
    # one variant more than a full variant tile
    _same(c.f.ds.glm_score_multi(c.Y, c.Z, v_begin=11, v_end=11 + VARIANT_TILE + 1),
          _rows(c.whole, slice(11, 11 + VARIANT_TILE + 1)), ctx="tile + 1")
    empty = c.f.ds.glm_score_multi(c.Y, c.Z, v_begin=77, v_end=77)
    assert empty["beta"].shape == (0, len(c.Y)) and empty["errcode"].shape == (0, len(c.Y))


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_blocks_the_chunks_or_the_scratch_budget(gpu_lib, case_1003):
    c = case_1003
    ds, Y, Z, whole = c.f.ds, c.Y, c.Z, c.whole
    # one phenotype more than a full phenotype block: two blocks under the default budget
    many = np.stack([Y[i % len(Y)] for i in range(PHENO_BLOCK + 1)])
    wide = ds.glm_score_multi(many, Z)
    for i in (0, 1, PHENO_BLOCK - 1, PHENO_BLOCK):
        _same(_col(wide, i), _col(whole, i % len(Y)), ctx=("block + 1", i))
    # The smallest column block is 1024 sample rows x 64 columns x 8 bytes = 524,288 bytes, and a phenotype's mask is
    # 256 bytes.  Any budget of which three quarters are less than that leaves one phenotype per block; what is left
    # of the budget after the block bounds the chunk at 228 bytes per variant and phenotype (k = 3):
    # 1 byte: a chunk of one variant; 526,200 bytes: seven variants.
    for budget in (1, 526_200):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(ds.glm_score_multi(Y, Z, v_begin=200, v_end=260), _rows(whole, slice(200, 260)), ctx=budget)
    # 1.5 MB: the largest block within 1.125 MB has 128 columns (1 MiB), which hold 19 phenotypes, so the 65 run as
    # blocks of 19, 19, 19 and 8, in chunks of 103 variants
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(SCRATCH_ENV, str(1_500_000))
        _same(ds.glm_score_multi(many, Z), wide, ctx="1.5 MB")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["all_but_one", "last_word", "word_block", "tile_plus_one", "stride4"])
def test_sample_subsets(gpu_lib, files, shape):
    """Against the oracle on the physically subsetted matrix."""
    f = files["hard", 1003]
    mask = SS.shapes(f.n)[shape]
    n_out = int(mask.sum())
    rng = np.random.default_rng(7)
    Zr = _covariates(rng, 2, f.n)
    Yr = _phenotypes(rng, f.n, Zr, specs=((0.35, 0.03), (0.5, 0.0), (0.3, 0.1)))
    Z, Y = np.ascontiguousarray(Zr[:, mask]), np.ascontiguousarray(Yr[:, mask])
    ss = f.ds.subset(mask)
    got = f.ds.glm_score_multi(Y, Z, subset=ss)
    x = f.x[:, mask]
    total = 0
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        fitted, worst = O.check_rows(_col(got, p), x, nul, rel=REL, idx=MADE + STRIDE7)
        print(f"{shape} ({n_out} samples) phenotype {p}: {fitted} fitted, worst {worst:.3g}")
        total += fitted
        _counts_equal_the_dense_logistic_fit(_col(got, p), f.ds.glm(y, Z, model="logistic", firth=False, subset=ss),
                                             ctx=(shape, p))
    assert total > len(Y) * len(STRIDE7) // 3
    if shape == "word_block":
        assert got["errcode"][SS.ROW_BLOCK].tolist() == ["CONST_ALLELE"] * len(Y)
    ss.close()


@pytest.mark.gpu
def test_empty_and_tiny_subsets(gpu_lib, files):
    """As glm_score_sparse handles them in tests/test_subset_shapes.py: an empty subset is refused as empty, a single
    sample has one class, two samples of both classes give TOO_FEW_SAMPLES rows."""
    L = gpu_lib
    f = files["hard", 1003]
    masks = SS.shapes(f.n)
    ss = f.ds.subset(masks["empty"])
    with pytest.raises(L.PghArgError, match="sample subset is empty"):
        f.ds.glm_score_multi(np.zeros((2, 0)), None, subset=ss)
    ss.close()
    for name in ("first", "last"):
        ss = f.ds.subset(masks[name])
        with pytest.raises(L.PghArgError, match="no cases or no controls"):
            f.ds.glm_score_multi(np.array([[1.0], [0.0]]), None, subset=ss)
        ss.close()
    ss = f.ds.subset(masks["ends"])
    got = f.ds.glm_score_multi(np.array([[1.0, 0.0], [0.0, 1.0]]), None, subset=ss)
    assert set(got["errcode"].ravel()) == {"TOO_FEW_SAMPLES"} and np.isnan(got["beta"]).all()
    assert got["obs_ct"].max() <= 2
    ss.close()


@pytest.mark.gpu
def test_long_rows(gpu_lib, tmp_path):
    """The shape of test_glm_score_sparse.test_long_rows_and_long_missing_lists."""
    n, m, k = 70_000, 120, 20
    codes = SS.hard_codes(n, m=m)
    path = str(tmp_path / "long.pgen")
    W.write_pgen(path, codes, [0] * m)
    ds = gpu_lib.Dataset.open(path)
    rng = np.random.default_rng(71)
    Z = _covariates(rng, k, n)
    Y = _phenotypes(rng, n, Z, specs=((0.2, 0.03), (0.05, 0.3)))
    got = ds.glm_score_multi(Y, Z)
    x = SS.values(codes)
    idx = MADE + list(range(0, m, 9))[:13]
    assert len(idx) == 16
    for p, y in enumerate(Y):
        nul = O.Null(y, Z)
        assert nul.status is None
        fitted, worst = O.check_rows(_col(got, p), x, nul, rel=REL, idx=idx)
        print(f"long rows phenotype {p}: {fitted} fitted of 16, worst {worst:.3g}")
        assert fitted >= 12
    ds.close()


@pytest.mark.gpu
def test_null_model_outcomes(gpu_lib, files):
    f = files["hard", 257]
    ds = f.ds
    rng = np.random.default_rng(77)
    z, z2 = rng.normal(size=(2, f.n))
    Y = _phenotypes(rng, f.n, z[None, :], specs=((0.3, 0.03), (0.5, 0.0)))
    # collinear covariates: every otherwise undecided row of every phenotype
    good = ds.glm_score_multi(Y, np.stack([z, z2]))
    assert all(O.Null(y, np.stack([z, z])).status == "SINGULAR_MATRIX" for y in Y)
    got = ds.glm_score_multi(Y, np.stack([z, z]))
    decided = np.isin(good["errcode"], ["TOO_FEW_SAMPLES", "CONST_ALLELE"])
    assert decided.any() and not decided.all()
    assert got["errcode"][decided].tolist() == good["errcode"][decided].tolist()
    assert set(got["errcode"][~decided]) == {"SINGULAR_MATRIX"}
    assert got["obs_ct"].tolist() == good["obs_ct"].tolist()
    assert np.array_equal(got["a1_freq"], good["a1_freq"], equal_nan=True)
    for key in ("beta", "se", "stat", "p"):
        assert np.isnan(got[key]).all(), key
    # a phenotype separated by a covariate: NO_CONVERGENCE for its own column only
    sep = (z > 0.1).astype(np.float64)
    assert O.Null(sep, z[None, :]).status == "NO_CONVERGENCE"
    base = ds.glm_score_multi(Y, z[None, :])
    assert (base["errcode"] == None).sum() > M  # noqa: E711
    with_sep = ds.glm_score_multi(np.stack([Y[0], sep, Y[1]]), z[None, :])
    _same(_col(with_sep, 0), _col(base, 0), ctx="before the separated phenotype")
    _same(_col(with_sep, 2), _col(base, 1), ctx="after the separated phenotype")
    sep_decided = np.isin(with_sep["errcode"][:, 1], ["TOO_FEW_SAMPLES", "CONST_ALLELE"])
    assert not sep_decided.all() and set(with_sep["errcode"][~sep_decided, 1]) == {"NO_CONVERGENCE"}
    _counts_equal_the_dense_logistic_fit(_col(with_sep, 1), ds.glm(sep, z[None, :], model="logistic", firth=False))


@pytest.mark.gpu
def test_refusals(gpu_lib, tmp_path):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    group = L.Dataset.open_sharded(path, [0, 0])
    n, m = dense.n_samples, dense.v_end - dense.v_begin
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    assert dense.glm_score_multi(Y, v_begin=0, v_end=8)["errcode"].shape == (8, 2)

    from test_dosage_tracks import make_dosage_file

    dose_path = str(tmp_path / "dose.pgen")
    make_dosage_file(dose_path, 20, 100, 300, True)
    dose = L.Dataset.open(dose_path)
    assert dose.info.dosage_variant_ct > 0
    y_dose = (np.arange(100) % 3 == 0).astype(np.float64)[None, :]

    def raw(ds, phen, n_pheno=None, z=None, n_covar=0, v0=0, v1=8, subset=None):
        out = np.full(32 * max(1, v1 - v0) * max(1, len(phen)), 0xAB, dtype=np.uint8)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        rc = L.raw().pgh_glm_score_multi(ds._h, subset, v0, v1, len(phen) if n_pheno is None else n_pheno, p(phen),
                                         n_covar, p(z), p(out), eb)
        return rc, eb.value.decode(), bool((out == 0xAB).all())

    y_two = Y.copy()
    y_two[1, 4] = 2.0
    y_one = Y.copy()
    y_one[1] = 1.0
    y_one[1, ::5] = NAN
    inf = np.zeros((2, n))
    inf[1, 5] = np.inf
    cases = [
        ("at least one phenotype", (dense, Y, 0)),
        ("phenotype must be 0 or 1", (dense, y_two)),
        ("no cases or no controls", (dense, y_one)),
        ("needs a dense-resident dataset", (sp, Y)),
        ("one device's dataset", (group, Y)),
        ("hardcalls only", (dose, y_dose)),
        ("at most 20 covariates", (dense, Y, None, np.zeros((21, n)), 21)),
        ("covariate 1 is not finite at sample 5", (dense, Y, None, inf, 2)),
        ("outside the resident range", (dense, Y, None, None, 0, 0, m + 1)),
        ("outside the resident range", (dense, Y, None, None, 0, 9, 8)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    # the two phenotype messages name the phenotype
    assert "(phenotype 1)" in raw(dense, y_two)[1] and "(phenotype 1)" in raw(dense, y_one)[1]
    with pytest.raises(ValueError, match="phenotype must be 0 or 1"):
        dense.glm_score_multi(y_two)
    # an empty range is fine
    rc, msg, untouched = raw(dense, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched
    assert dense.glm_score_multi(Y, v_begin=3, v_end=3)["errcode"].shape == (0, 2)
    for ds in (dose, group, sp, dense):
        ds.close()
