"""pgh_glm_score_multi_firth / Dataset.glm_score_multi_firth: the approximate Firth estimate (covariate effects fixed
at the null fit) of the dense route's rows beyond a cutoff.  Against the FP64 oracle (tests/glm_firth_oracle.py) the
errcodes and states are equal, the rows that are not applied carry NaN or `out`'s beta, se and p bit for bit, and the
applied rows are within TOL on |delta beta| / se, |delta se| / se and |delta p| / p; `out` is pgh_glm_score_multi's bit
for bit with its firth byte 0; and a row does not depend on the other phenotypes, its place among them, the range, the
phenotype block, the variant chunk or the scratch budget.

TOL is 100 x the worst difference between the numpy model of the kernel's accumulation order
(tools/glm_score_dense_firth_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is
test_glm_score_sparse_spa's, for device exp / log1p and fma contraction.  The cases at every covariate width and at
the sample-count edges are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_dense_firth_model.py --widths` prints."""

import ctypes as C
import functools
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_firth_oracle as F
import glm_score_oracle as O
import pgen_writer as W
import subset_shapes as SS
import test_glm_score_multi_spa as MS
from test_glm_score_multi_spa import phenotypes
from test_glm_score_sparse_spa import ParityInputs

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_multi_firth"]
MODEL_WORST = 1.21e-12  # printed by tools/glm_score_dense_firth_model.py
TOL = 100 * MODEL_WORST
# printed by tools/glm_score_dense_firth_model.py --widths: the width and sample-count cases below, on the rows they
# check
MODEL_WORST_WIDTHS = 4.93e-12
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
PARITY_N = (257, 4099)
PARITY_K = (0, 1, 3)
WIDTHS, WIDTHS_N, WIDTHS_STRIDE, EDGES, EDGE_K = MS.WIDTHS, MS.WIDTHS_N, MS.WIDTHS_STRIDE, MS.EDGES, MS.EDGE_K
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
SUBSET_SHAPE = "stride4"  # every 16-code word of the row is cut: four of its samples are kept
FIRTH_KEYS = ("beta_firth", "se_firth", "p_firth")


# ---- inputs and the oracle ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(n):
    return ParityInputs(n)


def oracle_column(x, codes, y, Z, cutoff=CUTOFF, idx=None):
    """Per variant glm_firth_oracle.firth_row's (row, beta, se, p, state, info) of one phenotype; None where idx leaves
    it out."""
    nul = O.Null(y, Z)
    assert nul.status is None
    out = [None] * len(x)
    for i in (range(len(x)) if idx is None else idx):
        out[i] = F.firth_row(x[i], codes[i], nul, cutoff)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(n, k):
    """The oracle's columns of the three phenotypes of ParityInputs(n) with k covariates (computed once)."""
    case = inputs(n)
    Z = case.covariates(k)
    return [oracle_column(case.x, case.geno, y, Z) for y in phenotypes(case)]


@functools.lru_cache(maxsize=None)
def oracle_thinned(n, k, stride):
    """oracle_case on every stride-th row: the width and sample-count cases (computed once)."""
    case = inputs(n)
    Z = case.covariates(k)
    return [oracle_column(case.x, case.geno, y, Z, idx=range(0, case.m, stride)) for y in phenotypes(case)]


def applied_rows(col):
    return [w for w in col if w is not None and w[4] == 1]


def check_column(got, p, want, tol=None, ctx=None):
    """Column p of Dataset.glm_score_multi_firth's dict against oracle_column's rows.  Returns (applied, worst)."""
    tol = TOL if tol is None else tol
    applied, worst = 0, 0.0
    for i, w in enumerate(want):
        if w is None:
            continue
        row, beta, se, pv, state, _ = w
        g = [got[key][i, p] for key in FIRTH_KEYS]
        at = (ctx, i, p, row, beta, se, pv, state, g, got["firth_state"][i, p], got["errcode"][i, p])
        assert got["errcode"][i, p] == row["errcode"], at
        assert got["firth_state"][i, p] == state, at
        if row["errcode"] is not None:
            assert all(math.isnan(v) for v in g), at
        elif state != 1:
            assert g == [got[key][i, p] for key in ("beta", "se", "p")], at
        else:
            diffs = (abs(g[0] - beta) / se, abs(g[1] - se) / se, abs(g[2] - pv) / pv)
            worst = max(worst, *diffs)
            assert max(diffs) <= tol, (diffs, at)
            applied += 1
    return applied, worst


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_multi_firth(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "} pgh_glm_firth_row;" in header
    assert lib.GLM_FIRTH_ROW_DTYPE.itemsize == 32
    assert hasattr(lib.Dataset, "glm_score_multi_firth")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_multi_firth_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi_firth(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi_firth(fake, np.zeros((2, 5)), np.zeros((2, 4)))


@pytest.mark.parametrize("cutoff", [0.05, NAN, -math.inf])
def test_glm_score_multi_firth_rejects_a_cutoff_below_a_tenth(lib, cutoff):
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        lib.Dataset.glm_score_multi_firth(fake, np.zeros((2, 5)), firth_cutoff=cutoff)


def _fill(L, n_rows):
    return (np.full(n_rows * L.GLM_ROW_DTYPE.itemsize, 0xAB, dtype=np.uint8),
            np.full(n_rows * L.GLM_FIRTH_ROW_DTYPE.itemsize, 0xCD, dtype=np.uint8))


def _untouched(out, firth):
    return bool((out == 0xAB).all() and (firth == 0xCD).all())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_a_null_dataset_is_refused_with_the_outputs_untouched(lib):
    out, firth = _fill(lib, 4)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    rc = lib.raw().pgh_glm_score_multi_firth(None, None, 0, 4, 1, _ptr(y), 0, None, C.c_double(CUTOFF), _ptr(out),
                                             _ptr(firth), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and _untouched(out, firth)


@functools.lru_cache(maxsize=None)
def small_case():
    """n = 257, k = 1, the inputs' own phenotype: (case, Null, the oracle's column)."""
    case = inputs(257)
    col = oracle_case(257, 1)[0]
    return case, O.Null(phenotypes(case)[0], case.covariates(1)), col


def test_the_oracle_F_and_H_are_the_derivatives_of_l_star():
    """Central differences with h = 1e-4 / sqrt(K''(0)), a ten-thousandth of the null standard error of beta.  On the
    scale beta / se0 the derivatives of l* are O(1) multiples of each other, so the truncation error h^2 f''' / 6 is
    about 1e-8 of the derivative's scale and the rounding error eps |f| / h about 1e-12 |f|: 1e-6 of the scale
    (sqrt(K''(0)) + |G| for F, K''(0) for H) bounds both with room."""
    case, nul, col = small_case()
    checked = replaced = 0
    for i, (row, beta, se, pv, state, info) in enumerate(col):
        if state != 1:
            continue
        cgf, _ = F.cgf_of(case.x[i], case.geno[i], nul)
        k2_0 = cgf.k(0.0)[2]
        h = 1e-4 / math.sqrt(k2_0)
        for b in (0.0, 0.5 * beta, beta, 2.0 * beta):
            ls, f, hh, k2, was_replaced = cgf.at(b)
            d1 = (cgf.lstar(b + h) - cgf.lstar(b - h)) / (2 * h)
            assert abs(d1 - f) <= 1e-6 * (math.sqrt(k2_0) + abs(cgf.g)), (i, b, d1, f)
            replaced += was_replaced
            if not was_replaced:
                d2 = (cgf.at(b + h)[1] - cgf.at(b - h)[1]) / (2 * h)
                assert abs(-d2 - hh) <= 1e-6 * k2_0, (i, b, d2, hh)
                checked += 1
    print(f"{checked} points with H checked, {replaced} with H replaced by K''")
    assert checked >= 40


def test_the_oracle_root_is_a_local_maximum_of_l_star():
    """A thousandth of the row's se to either side: l* falls by about H h^2 / 2 = 5e-7 K''-units, far above the
    rounding of l*."""
    case, nul, col = small_case()
    seen = 0
    for i, (row, beta, se, pv, state, info) in enumerate(col):
        if state != 1:
            continue
        cgf, _ = F.cgf_of(case.x[i], case.geno[i], nul)
        top = cgf.lstar(beta)
        assert cgf.lstar(beta + 1e-3 * se) <= top and cgf.lstar(beta - 1e-3 * se) <= top, (i, beta, se)
        assert 0.0 <= pv <= 1.0 and se > 0
        seen += 1
    assert seen >= 10


def test_the_oracle_leaves_every_row_alone_under_a_cutoff_above_every_stat():
    case, nul, col = small_case()
    top = max(abs(w[0]["stat"]) for w in col if w[0]["errcode"] is None)
    fitted = 0
    for i in range(case.m):
        row, beta, se, pv, state, info = F.firth_row(case.x[i], case.geno[i], nul, top + 1.0)
        assert state == 0 and info["evals"] == 0
        if row["errcode"] is None:
            assert (beta, se, pv) == (row["beta"], row["se"], row["p"])
            fitted += 1
        else:
            assert math.isnan(beta) and math.isnan(se) and math.isnan(pv)
    assert 0 < fitted < case.m


def test_the_oracle_gives_a_separated_row_a_finite_estimate():
    case, nul, col = small_case()
    separated = [w for w in col if w[4] == 1 and w[5]["separated"]]
    assert separated
    for row, beta, se, pv, state, info in separated:
        assert math.isfinite(beta) and math.isfinite(se) and se > 0 and 0.0 < pv <= 1.0


def test_the_parity_inputs_reach_the_cases_of_the_contract():
    """Conditions on the inputs, not on the device."""
    flipped_all = 0
    for n in PARITY_N:
        for k in PARITY_K:
            for p, col in enumerate(oracle_case(n, k)):
                applied = [w for w in col if w[4] == 1]
                failed = sum(w[4] == 2 for w in col)
                evals = max(w[5]["evals"] for w in applied)
                separated = sum(w[5]["separated"] for w in applied)
                flipped = sum(w[1] * w[0]["beta"] < 0 for w in applied)
                print(f"n={n} k={k} phenotype {p}: {len(applied)} applied, {failed} failed, at most {evals} evaluations, "
                      f"{separated} separated, {flipped} of the other sign")
                assert len(applied) >= 10, (n, k, p)
                assert failed == 0, (n, k, p)
                assert evals <= 16, (n, k, p)
                if p == 0:
                    assert separated >= 4, (n, k)
                flipped_all += flipped
    assert flipped_all >= 1


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_at_every_width(k):
    """Conditions on the inputs, not on the device, so that a width cannot pass on rows that are left alone: on the
    rows test_every_instantiated_width checks the oracle decides every row (it asserts that every null model is
    fitted), no row fails, each phenotype has 3 applied rows and the three have 15."""
    cols = oracle_thinned(WIDTHS_N, k, WIDTHS_STRIDE)
    applied = [len(applied_rows(col)) for col in cols]
    print(f"k={k}: {applied} applied")
    assert not any(w is not None and w[4] == 2 for col in cols for w in col), k
    assert min(applied) >= 3 and sum(applied) >= 15, k


@pytest.mark.parametrize("n,stride", EDGES)
def test_the_sample_count_edges_have_applied_rows(n, stride):
    applied = [len(applied_rows(col)) for col in oracle_thinned(n, EDGE_K, stride)]
    print(f"n={n}: {applied} applied")
    assert min(applied) >= (15 if n == 4096 else 5), n


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _col(out, p, rows=slice(None)):
    return {key: v[rows, p] for key, v in out.items()}


def _rows(out, rows):
    return {key: v[rows] for key, v in out.items()}


def _same_rows(a, b, ctx=None):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    for key in ("obs_ct", "errcode", "firth"):
        assert np.asarray(a[key]).tolist() == np.asarray(b[key]).tolist(), (key, ctx)


def _same(a, b, ctx=None):
    _same_rows(a, b, ctx)
    for key in FIRTH_KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    assert a["firth_state"].tolist() == b["firth_state"].tolist(), ctx


class _File:
    """The parity inputs as a .pgen of every record type, opened dense."""

    def __init__(self, L, tmp, n):
        self.case = inputs(n)
        self.n, self.m = n, self.case.m
        self.Y = phenotypes(self.case)
        self.path = str(tmp / f"multi_firth_{n}.pgen")
        W.write_pgen(self.path, self.case.geno, self.case.kinds)
        self.ds = L.Dataset.open(self.path)


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_firth")
    return {n: _File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.fixture(scope="module")
def case_4099(files):
    """n = 4099, k = 3: the covariates and the whole-range result that the bit-for-bit tests share."""
    f = files[4099]
    Z = f.case.covariates(3)
    return types.SimpleNamespace(f=f, Z=Z, whole=f.ds.glm_score_multi_firth(f.Y, Z, firth_cutoff=CUTOFF))


def _raw(L, ds, Y, Z, cutoff, v0, v1):
    """The C call on prefilled buffers: (rc, rows, firth rows) as structured arrays."""
    out, firth = _fill(L, (v1 - v0) * len(Y))
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = L.raw().pgh_glm_score_multi_firth(ds._h, None, v0, v1, len(Y), _ptr(Y), len(Z), _ptr(Z), C.c_double(cutoff),
                                           _ptr(out), _ptr(firth), eb)
    return rc, out.view(L.GLM_ROW_DTYPE), firth.view(L.GLM_FIRTH_ROW_DTYPE)


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle(gpu_lib, files, n, k):
    f = files[n]
    zc = f.case.covariates(k) if k else None
    got = f.ds.glm_score_multi_firth(f.Y, zc, firth_cutoff=CUTOFF)
    for key in FIRTH_KEYS:
        assert got[key].shape == (f.m, len(f.Y)) and got[key].dtype == np.float64
    assert got["firth_state"].shape == (f.m, len(f.Y)) and got["firth_state"].dtype == np.uint8
    _same_rows(got, f.ds.glm_score_multi(f.Y, zc), ctx=(n, k))
    assert not got["firth"].any()
    for p, col in enumerate(oracle_case(n, k)):
        applied, worst = check_column(got, p, col, ctx=(n, k))
        print(f"n={n} k={k} phenotype {p}: {applied} applied, worst {worst:.3g} (TOL {TOL:.3g})")
        assert applied == sum(w[4] == 1 for w in col) >= 10


@pytest.fixture(scope="module")
def edge_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_firth_edges")
    return {n: _File(gpu_lib, tmp, n) for n, _ in EDGES}


def _thinned_parity(f, k, stride):
    """The thinned rows of file f at k covariates against the oracle at TOL_WIDTHS; `out` is glm_score_multi's bit for
    bit.  Returns the applied rows per phenotype."""
    Z = f.case.covariates(k)
    got = f.ds.glm_score_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
    _same_rows(got, f.ds.glm_score_multi(f.Y, Z), ctx=(f.n, k))
    assert not got["firth"].any()
    counts = []
    for p, col in enumerate(oracle_thinned(f.n, k, stride)):
        applied, worst = check_column(got, p, col, tol=TOL_WIDTHS, ctx=(f.n, k))
        print(f"n={f.n} k={k} phenotype {p}: {applied} applied, worst {worst:.3g} (TOL {TOL_WIDTHS:.3g})")
        assert applied == len(applied_rows(col))
        counts.append(applied)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """Column p (k + 2) of a block whose leading dimension is GlmScoreDenseLayout(pb, k).ld, for every width
    GlmPadCovar returns at k = KP and one above the width below."""
    counts = _thinned_parity(files[WIDTHS_N], k, WIDTHS_STRIDE)
    assert min(counts) >= 3 and sum(counts) >= 15


@pytest.mark.gpu
@pytest.mark.parametrize("n,stride", EDGES)
def test_sample_count_edges(gpu_lib, edge_files, n, stride):
    """n = 4096: the mask's words fill exactly one 4,096-sample step of the walk; n = 8209: a third step."""
    counts = _thinned_parity(edge_files[n], EDGE_K, stride)
    assert min(counts) >= (15 if n == 4096 else 5)


@pytest.mark.gpu
def test_the_same_bytes(gpu_lib, files):
    L = gpu_lib
    f = files[257]
    Z = f.case.covariates(1)
    base = f.ds.glm_score_multi(f.Y, Z)
    got = f.ds.glm_score_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
    _same_rows(got, base, ctx="out")
    assert (got["firth_state"] == 1).any()
    _same(f.ds.glm_score_multi_firth(f.Y, Z, firth_cutoff=CUTOFF), got, ctx="again")
    rc_a, out_a, firth_a = _raw(L, f.ds, f.Y, Z, CUTOFF, 0, f.m)
    rc_b, out_b, firth_b = _raw(L, f.ds, f.Y, Z, CUTOFF, 0, f.m)
    assert rc_a == rc_b == L.PGH_OK
    assert out_a.tobytes() == out_b.tobytes() and firth_a.tobytes() == firth_b.tobytes()
    assert not firth_a["pad"].any() and not out_a["firth"].any()
    assert firth_a["state"].reshape(f.m, len(f.Y)).tolist() == got["firth_state"].tolist()
    never = f.ds.glm_score_multi_firth(f.Y, Z, firth_cutoff=math.inf)
    _same_rows(never, base, ctx="inf")
    assert not never["firth_state"].any()
    for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
        assert np.array_equal(never[key], base[of], equal_nan=True), key
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
    empty = f.ds.glm_score_multi_firth(f.Y, Z, v_begin=77, v_end=77)
    assert all(empty[key].shape == (0, len(f.Y)) for key in FIRTH_KEYS + ("firth_state", "beta"))


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_other_phenotypes_or_its_place(gpu_lib, case_4099):
    c = case_4099
    ds, Y, Z, whole = c.f.ds, c.f.Y, c.Z, c.whole
    assert all((whole["firth_state"][:, p] == 1).sum() >= 10 for p in range(len(Y)))
    perm = [2, 0, 1]
    moved = ds.glm_score_multi_firth(Y[perm], Z)
    for to, p in enumerate(perm):
        _same(_col(moved, to), _col(whole, p), ctx=("permuted", p))
    for p in range(len(Y)):
        _same(_col(ds.glm_score_multi_firth(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_the_block_the_chunk_or_the_scratch_budget(gpu_lib, case_4099):
    c = case_4099
    ds, Y, Z, whole = c.f.ds, c.f.Y, c.Z, c.whole
    _same(ds.glm_score_multi_firth(Y, Z, v_begin=37), _rows(whole, slice(37, None)), ctx="v_begin = 37")
    _same(ds.glm_score_multi_firth(Y, Z, v_begin=37, v_end=333), _rows(whole, slice(37, 333)), ctx="37 .. 333")
    # test_glm_score_multi_spa's budgets.  The smallest column block is 4,160 sample rows x 64 columns x 8 bytes =
    # 2,129,920 bytes and a phenotype's mask 1,040 bytes: any budget of which three quarters are less leaves one
    # phenotype per block.  What the budget leaves after the block goes to one workgroup's stash first (16 bytes x
    # 4,099 samples = 65,584; never less than one) and then bounds the chunk.  1 byte: a chunk of one variant (a part
    # of the range); 2,200,960 bytes = block + 70,000: 4,416 bytes are left, at 276 bytes per variant and phenotype
    # (k = 3) a chunk of 16 variants.
    # 2,430,960 bytes = block_bytes + 300,000 (block_bytes = the block and the mask, 2,130,960; three quarters of the
    # budget are still less, so pb_max = 1): n_groups = 300,000 / 4 * 3 / per_group = 225,000 / 65,584 = 3 workgroups,
    # and the 300,000 - 3 x 65,584 = 103,248 bytes left bound the chunk at per_variant = 228 + 32 = 260 (k = 3): 397
    # variants, so each workgroup walks its chunk's rows at a stride of 3.
    before = os.environ.get(SCRATCH_ENV)
    for budget, lo, hi in ((1, 200, 260), (2_200_960, 0, c.f.m), (2_430_960, 0, c.f.m)):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(ds.glm_score_multi_firth(Y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx=budget)
    assert os.environ.get(SCRATCH_ENV) == before


@pytest.mark.gpu
def test_a_sample_subset_that_cuts_the_words(gpu_lib, files):
    """Against the oracle on the subset's samples."""
    f = files[4099]
    mask = SS.shapes(f.n)[SUBSET_SHAPE]
    assert mask[:16].sum() not in (0, 16)
    k = 3
    Z = np.ascontiguousarray(f.case.covariates(k)[:, mask])
    Y = np.ascontiguousarray(f.Y[:, mask])
    x, codes = f.case.x[:, mask], f.case.geno[:, mask]
    ss = f.ds.subset(mask)
    got = f.ds.glm_score_multi_firth(Y, Z, firth_cutoff=CUTOFF, subset=ss)
    _same_rows(got, f.ds.glm_score_multi(Y, Z, subset=ss), ctx=SUBSET_SHAPE)
    total = 0
    for p, y in enumerate(Y):
        applied, worst = check_column(got, p, oracle_column(x, codes, y, Z), ctx=(SUBSET_SHAPE, p))
        print(f"{SUBSET_SHAPE} ({int(mask.sum())} samples) phenotype {p}: {applied} applied, worst {worst:.3g}")
        total += applied
    assert total >= 7
    ss.close()


@pytest.mark.gpu
def test_refusals(gpu_lib, tmp_path):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = dense.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    ok = dense.glm_score_multi_firth(Y, v_begin=0, v_end=8)
    assert ok["beta_firth"].shape == (8, 2) and ok["firth_state"].dtype == np.uint8

    from test_dosage_tracks import make_dosage_file

    dose_path = str(tmp_path / "dose.pgen")
    make_dosage_file(dose_path, 20, 100, 300, True)
    dose = L.Dataset.open(dose_path)
    assert dose.info.dosage_variant_ct > 0
    y_dose = (np.arange(100) % 3 == 0).astype(np.float64)[None, :]

    def raw(ds, phen, cutoff=CUTOFF, null_firth=False):
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        out, firth = _fill(L, 8 * len(phen))
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        rc = L.raw().pgh_glm_score_multi_firth(ds._h, None, 0, 8, len(phen), _ptr(phen), 0, None, C.c_double(cutoff),
                                               _ptr(out), None if null_firth else _ptr(firth), eb)
        return rc, eb.value.decode(), _untouched(out, firth)

    cases = [
        ("firth_cutoff must be at least 0.1", (dense, Y, 0.05)),
        ("firth_cutoff must be at least 0.1", (dense, Y, NAN)),
        ("null firth", (dense, Y, CUTOFF, True)),
        ("needs a dense-resident dataset", (sp, Y)),
        ("hardcalls only", (dose, y_dose)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        dense.glm_score_multi_firth(Y, firth_cutoff=0.05)
    for ds in (dose, sp, dense):
        ds.close()
