"""pgh_glm_score_multi_spa / Dataset.glm_score_multi_spa: the saddlepoint p-value of the logistic score test on the
dense route.  Against the FP64 oracle (tests/glm_spa_oracle.py) under the dense rule (b = 2 when the hom-alt calls among
N outnumber the hom-ref ones, otherwise 0; E = the samples of N with x != b) the errcodes and states are equal and p_spa
is within TOL in state 1; `out` is pgh_glm_score_multi's bit for bit; a row's triple does not depend on the other
phenotypes, its place among them, the range, the phenotype block, the variant chunk or the scratch budget; and the
sparse route agrees on the rows whose base code is the dense b.

TOL is 100 x the worst relative difference between the numpy model of the kernel's accumulation order
(tools/glm_score_dense_spa_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is
test_glm_score_sparse_spa's, for device exp / log1p and fma contraction.  The cases at every covariate width and at
the sample-count edges are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_dense_spa_model.py --widths` prints."""

import ctypes as C
import functools
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_score_oracle as O
import glm_spa_oracle as S
import pgen_writer as W
import subset_shapes as SS
import test_glm_score_sparse_spa as SP
from test_glm_score_sparse_spa import ParityInputs

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_multi_spa"]
MODEL_WORST = 1.41e-11  # printed by tools/glm_score_dense_spa_model.py
TOL = 100 * MODEL_WORST
# printed by tools/glm_score_dense_spa_model.py --widths: the width and sample-count cases below, on the rows they check
MODEL_WORST_WIDTHS = 9.76e-12
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
PARITY_N = (257, 4099)
PARITY_K = (0, 1, 3)
WIDTHS, WIDTHS_N, WIDTHS_STRIDE = SP.WIDTHS, SP.WIDTHS_N, SP.WIDTHS_STRIDE
# (n, row stride) at k = EDGE_K: exactly one 4,096-sample step of the walk, and a third step
EDGES = ((4096, 1), (8209, 3))
EDGE_K = 3
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
SUBSET_SHAPE = "stride4"  # every 16-code word of the row is cut: four of its samples are kept


# ---- inputs and the oracle ----------------------------------------------------------------------------------------

def phenotypes(case):
    """The inputs' own y, a 2 % phenotype without NaN, a 30 % phenotype with a tenth of it NaN."""
    rng = np.random.default_rng(9000 + case.n)
    rare = (rng.random(case.n) < 0.02).astype(np.float64)
    common = (rng.random(case.n) < 0.3).astype(np.float64)
    common[rng.random(case.n) < 0.1] = NAN
    return np.stack([case.y, rare, common])


@functools.lru_cache(maxsize=None)
def inputs(n):
    return ParityInputs(n)


def dense_base(codes, in_s):
    c = np.bincount(codes[in_s], minlength=4)
    return (2 if c[2] > c[0] else 0), int(c[0]), int(c[2])


def oracle_column(x, codes, y, Z, cutoff=CUTOFF, idx=None):
    """Per variant (row, p_spa, state, b, n0, n2) of one phenotype under the dense rule; None where idx leaves it out."""
    nul = O.Null(y, Z)
    assert nul.status is None
    out = [None] * len(x)
    for i in (range(len(x)) if idx is None else idx):
        b, n0, n2 = dense_base(codes[i], nul.in_s)
        out[i] = S.spa_row(x[i], codes[i], nul, b, False, cutoff) + (b, n0, n2)
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
    return [w for w in col if w is not None and w[2] == 1]


def check_column(got, p, want, tol=None, ctx=None):
    """Column p of Dataset.glm_score_multi_spa's dict against oracle_column's rows.  Returns (applied, worst)."""
    tol = TOL if tol is None else tol
    applied, worst = 0, 0.0
    for i, w in enumerate(want):
        if w is None:
            continue
        row, p_spa, state = w[:3]
        g_p, g_spa, g_state = got["p"][i, p], got["p_spa"][i, p], got["spa_state"][i, p]
        at = (ctx, i, p, w, g_p, g_spa, g_state, got["errcode"][i, p])
        assert got["errcode"][i, p] == row["errcode"], at
        assert g_state == state, at
        if row["errcode"] is not None:
            assert math.isnan(g_spa), at
        elif state != 1:
            assert g_spa == g_p, at
        else:
            diff = abs(g_spa - p_spa) / p_spa
            worst = max(worst, diff)
            assert diff <= tol, (diff, at)
            applied += 1
    return applied, worst


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_multi_spa(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_multi_spa")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_multi_spa_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi_spa(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi_spa(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def _fill(n_rows, itemsize):
    return (np.full(n_rows * itemsize, 0xAB, dtype=np.uint8), np.full(n_rows, 123.0), np.full(n_rows, 77, dtype=np.uint8))


def _untouched(out, p_spa, state):
    return bool((out == 0xAB).all() and (p_spa == 123.0).all() and (state == 77).all())


def test_a_null_dataset_is_refused_with_the_outputs_untouched(lib):
    out, p_spa, state = _fill(4, 32)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.raw().pgh_glm_score_multi_spa(None, None, 0, 4, 1, p(y), 0, None, C.c_double(CUTOFF), p(out), p(p_spa),
                                           p(state), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and _untouched(out, p_spa, state)


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_reach_every_case_of_the_dense_rule(n, k):
    """Conditions on the inputs, not on the device: the oracle decides every row (it asserts where the contract does
    not), and each phenotype has applied rows of both base codes."""
    for p, col in enumerate(oracle_case(n, k)):
        applied = [w for w in col if w[2] == 1]
        b2 = [w for w in applied if w[3] == 2]
        tie = [w for w in applied if w[4] == w[5]]
        differ = [w for w in applied if not 0.5 <= w[1] / w[0]["p"] <= 2.0]
        failed = sum(w[2] == 2 for w in col)
        print(f"n={n} k={k} phenotype {p}: {len(applied)} applied, {len(b2)} with b = 2, {len(tie)} with n0 == n2, "
              f"{len(differ)} beyond 2x, {failed} failed")
        assert len(applied) >= 7 and len(b2) >= 2, (n, k, p)
        if n == 257 and p == 1:
            assert len(tie) >= 1, (n, k)
        if n == 4099 and p == 0:
            assert len(differ) >= 30, (n, k)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_at_every_width(k):
    """Conditions on the inputs, not on the device, so that a width cannot pass on rows that are left alone: on the
    rows test_every_instantiated_width checks the oracle decides every row (it asserts where the contract does not,
    and that every null model is fitted), each phenotype has 3 applied rows, the three have 15, and 4 have b = 2."""
    applied = [applied_rows(col) for col in oracle_thinned(WIDTHS_N, k, WIDTHS_STRIDE)]
    b2 = sum(w[3] == 2 for a in applied for w in a)
    print(f"k={k}: {[len(a) for a in applied]} applied, {b2} with b = 2")
    assert min(len(a) for a in applied) >= 3 and sum(len(a) for a in applied) >= 15 and b2 >= 4, k


@pytest.mark.parametrize("n,stride", EDGES)
def test_the_sample_count_edges_have_applied_rows(n, stride):
    applied = [applied_rows(col) for col in oracle_thinned(n, EDGE_K, stride)]
    b2 = sum(w[3] == 2 for a in applied for w in a)
    print(f"n={n}: {[len(a) for a in applied]} applied, {b2} with b = 2")
    assert min(len(a) for a in applied) >= (15 if n == 4096 else 5) and b2 >= 1, n


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
    assert np.array_equal(a["p_spa"], b["p_spa"], equal_nan=True), ctx
    assert a["spa_state"].tolist() == b["spa_state"].tolist(), ctx


class _File:
    """The parity inputs as a .pgen of every record type, opened dense."""

    def __init__(self, L, tmp, n):
        self.case = inputs(n)
        self.n, self.m = n, self.case.m
        self.Y = phenotypes(self.case)
        self.path = str(tmp / f"multi_spa_{n}.pgen")
        W.write_pgen(self.path, self.case.geno, self.case.kinds)
        self.ds = L.Dataset.open(self.path)


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_spa")
    return {n: _File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.fixture(scope="module")
def case_4099(files):
    """n = 4099, k = 3: the covariates and the whole-range result that the bit-for-bit tests share."""
    f = files[4099]
    Z = f.case.covariates(3)
    return types.SimpleNamespace(f=f, Z=Z, whole=f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF))


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle(gpu_lib, files, n, k):
    f = files[n]
    zc = f.case.covariates(k) if k else None
    got = f.ds.glm_score_multi_spa(f.Y, zc, spa_cutoff=CUTOFF)
    assert got["p_spa"].shape == (f.m, len(f.Y)) and got["spa_state"].shape == (f.m, len(f.Y))
    assert got["p_spa"].dtype == np.float64 and got["spa_state"].dtype == np.uint8
    _same_rows(got, f.ds.glm_score_multi(f.Y, zc), ctx=(n, k))
    for p, col in enumerate(oracle_case(n, k)):
        applied, worst = check_column(got, p, col, ctx=(n, k))
        print(f"n={n} k={k} phenotype {p}: {applied} applied, worst {worst:.3g} (TOL {TOL:.3g})")
        assert applied == sum(w[2] == 1 for w in col) >= 7


@pytest.fixture(scope="module")
def edge_files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_spa_edges")
    return {n: _File(gpu_lib, tmp, n) for n, _ in EDGES}


def _thinned_parity(f, k, stride):
    """The thinned rows of file f at k covariates against the oracle at TOL_WIDTHS; `out` is glm_score_multi's bit for
    bit.  Returns the applied rows per phenotype."""
    Z = f.case.covariates(k)
    got = f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    _same_rows(got, f.ds.glm_score_multi(f.Y, Z), ctx=(f.n, k))
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
    """GlmScoreDenseSpaKernel<KP> for every width GlmPadCovar returns, at k = KP and one above the width below."""
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
    f = files[257]
    Z = f.case.covariates(1)
    base = f.ds.glm_score_multi(f.Y, Z)
    got = f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    _same_rows(got, base, ctx="out")
    assert (got["spa_state"] == 1).any()
    _same(f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF), got, ctx="again")
    never = f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=math.inf)
    _same_rows(never, base, ctx="inf")
    assert not never["spa_state"].any()
    assert np.array_equal(never["p_spa"], base["p"], equal_nan=True)
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
    empty = f.ds.glm_score_multi_spa(f.Y, Z, v_begin=77, v_end=77)
    assert empty["p_spa"].shape == (0, len(f.Y)) and empty["spa_state"].shape == (0, len(f.Y))


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_other_phenotypes_or_its_place(gpu_lib, case_4099):
    c = case_4099
    ds, Y, Z, whole = c.f.ds, c.f.Y, c.Z, c.whole
    assert all((whole["spa_state"][:, p] == 1).sum() >= 7 for p in range(len(Y)))
    _same(ds.glm_score_multi_spa(Y, Z), whole, ctx="again")
    perm = [2, 0, 1]
    moved = ds.glm_score_multi_spa(Y[perm], Z)
    for to, p in enumerate(perm):
        _same(_col(moved, to), _col(whole, p), ctx=("permuted", p))
    for p in range(len(Y)):
        _same(_col(ds.glm_score_multi_spa(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_range_the_block_the_chunk_or_the_scratch_budget(gpu_lib, case_4099):
    c = case_4099
    ds, Y, Z, whole = c.f.ds, c.f.Y, c.Z, c.whole
    _same(ds.glm_score_multi_spa(Y, Z, v_begin=37), _rows(whole, slice(37, None)), ctx="v_begin = 37")
    _same(ds.glm_score_multi_spa(Y, Z, v_begin=37, v_end=333), _rows(whole, slice(37, 333)), ctx="37 .. 333")
    # The smallest column block is 4,160 sample rows x 64 columns x 8 bytes = 2,129,920 bytes and a phenotype's mask
    # 1,040 bytes: any budget of which three quarters are less leaves one phenotype per block.  What the budget leaves
    # after the block goes to one workgroup's stash first (16 bytes x 4,099 samples = 65,584; never less than one) and
    # then bounds the chunk at 293 bytes per variant and phenotype (k = 3).  1 byte: a chunk of one variant (a part
    # of the range); 2,200,960 bytes = block + 70,000: (70,000 - 65,584) / 293 = a chunk of 15 variants.
    # 2,430,960 bytes = block_bytes + 300,000 (block_bytes = the block and the mask, 2,130,960; three quarters of the
    # budget are still less, so pb_max = 1): n_groups = 300,000 / 4 * 3 / per_group = 225,000 / 65,584 = 3 workgroups,
    # and the 300,000 - 3 x 65,584 = 103,248 bytes left bound the chunk at per_variant = 293: 352 variants, so each
    # workgroup walks its chunk's rows at a stride of 3.
    before = os.environ.get(SCRATCH_ENV)
    for budget, lo, hi in ((1, 200, 260), (2_200_960, 0, c.f.m), (2_430_960, 0, c.f.m)):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(ds.glm_score_multi_spa(Y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx=budget)
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
    got = f.ds.glm_score_multi_spa(Y, Z, spa_cutoff=CUTOFF, subset=ss)
    _same_rows(got, f.ds.glm_score_multi(Y, Z, subset=ss), ctx=SUBSET_SHAPE)
    total = 0
    for p, y in enumerate(Y):
        applied, worst = check_column(got, p, oracle_column(x, codes, y, Z), ctx=(SUBSET_SHAPE, p))
        print(f"{SUBSET_SHAPE} ({int(mask.sum())} samples) phenotype {p}: {applied} applied, worst {worst:.3g}")
        total += applied
    assert total >= 7
    ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_the_sparse_route_agrees_where_its_base_code_is_the_dense_b(gpu_lib, files, n):
    """Phenotype 0, k = 3, every row held sparse (max_minor = n): a row whose base code is the dense b has the same
    E on both routes, and each route is within its own tolerance of the same oracle value."""
    f = files[n]
    Z = f.case.covariates(3)
    y = f.Y[0]
    got = f.ds.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    sp = gpu_lib.Dataset.open(f.path, sparse=True, max_minor=n)
    other = sp.glm_score_sparse_spa(y, Z, cutoff=CUTOFF)
    sp.close()
    in_s = ~np.isnan(y)
    applied, worst = 0, 0.0
    for i in range(f.m):
        base, dense_form = S.row_form(f.case.geno[i], n)
        assert not dense_form
        if base == 3 or base != dense_base(f.case.geno[i], in_s)[0]:
            continue
        ctx = (n, i, base, got["spa_state"][i, 0], other["spa_state"][i], got["p_spa"][i, 0], other["p_spa"][i])
        assert got["errcode"][i, 0] == other["errcode"][i], ctx
        assert got["spa_state"][i, 0] == other["spa_state"][i], ctx
        if got["spa_state"][i, 0] == 1:
            diff = abs(got["p_spa"][i, 0] - other["p_spa"][i]) / other["p_spa"][i]
            worst = max(worst, diff)
            assert diff <= TOL + SP.TOL, (diff, ctx)
            applied += 1
    print(f"n={n}: {applied} applied rows with the same E on both routes, worst {worst:.3g}")
    if n == 4099:
        assert applied >= 20


@pytest.mark.gpu
def test_refusals(gpu_lib, tmp_path):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = dense.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    ok = dense.glm_score_multi_spa(Y, v_begin=0, v_end=8)
    assert ok["p_spa"].shape == (8, 2) and ok["spa_state"].dtype == np.uint8

    from test_dosage_tracks import make_dosage_file

    dose_path = str(tmp_path / "dose.pgen")
    make_dosage_file(dose_path, 20, 100, 300, True)
    dose = L.Dataset.open(dose_path)
    assert dose.info.dosage_variant_ct > 0
    y_dose = (np.arange(100) % 3 == 0).astype(np.float64)[None, :]

    def raw(ds, phen, cutoff=CUTOFF, null_p_spa=False):
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        out, p_spa, state = _fill(8 * len(phen), L.GLM_ROW_DTYPE.itemsize)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.raw().pgh_glm_score_multi_spa(ds._h, None, 0, 8, len(phen), p(phen), 0, None, C.c_double(cutoff), p(out),
                                             None if null_p_spa else p(p_spa), p(state), eb)
        return rc, eb.value.decode(), _untouched(out, p_spa, state)

    cases = [
        ("spa_cutoff must be at least 0.1", (dense, Y, 0.05)),
        ("spa_cutoff must be at least 0.1", (dense, Y, NAN)),
        ("null p_spa or spa_state", (dense, Y, CUTOFF, True)),
        ("needs a dense-resident dataset", (sp, Y)),
        ("hardcalls only", (dose, y_dose)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    with pytest.raises(ValueError, match="spa_cutoff must be at least 0.1"):
        dense.glm_score_multi_spa(Y, spa_cutoff=0.05)
    for ds in (dose, sp, dense):
        ds.close()
