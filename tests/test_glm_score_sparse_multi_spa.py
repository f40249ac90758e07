"""pgh_glm_score_sparse_multi_spa / Dataset.glm_score_sparse_multi_spa: the saddlepoint p-value of the logistic score
test over a sparse-resident dataset for many phenotypes in one call.  Against the FP64 oracle (tests/glm_spa_oracle.py,
one null fit per phenotype) the errcodes and states are equal and p_spa is within TOL in state 1, for every form the
file can be opened in; `out` is pgh_glm_score_sparse_multi's bit for bit; the one-phenotype route and the dense route
agree where their contracts say so; and a row's triple does not depend on the other phenotypes, its place among them,
n_pheno, the phenotype block, the range, the window, the variant chunk or the scratch budget.

TOL is 100 x the worst relative difference between the numpy model of the route's accumulation order
(tools/glm_score_sparse_multi_spa_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is
test_glm_score_sparse_spa's, for device exp / log1p and fma contraction.  The cases at every covariate width are held to
TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_sparse_multi_spa_model.py --widths` prints."""

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
import test_glm_score_multi_spa as MS
import test_glm_score_sparse_multi as SM
import test_glm_score_sparse_spa as SP

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse_multi_spa"]
MODEL_WORST = 2.06e-10  # printed by tools/glm_score_sparse_multi_spa_model.py
TOL = 100 * MODEL_WORST
MODEL_WORST_WIDTHS = 1.88e-11  # printed by tools/glm_score_sparse_multi_spa_model.py --widths
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
PARITY_N = SP.PARITY_N        # 257 and 4099: the 600-variant rare_matrix files of test_glm_score_sparse_spa
PARITY_K = (0, 1, 3)
# seeds whose matrices hold no row that the contract leaves undecided for any of the four phenotypes, any k of PARITY_K
# or WIDTHS and any form (the oracle asserts it: test_the_parity_inputs_reach_every_case), found by a search on the CPU
SEEDS = {257: 258, 4099: 4102}
WIDTHS, WIDTHS_N, WIDTHS_ROWS = SP.WIDTHS, SP.WIDTHS_N, SP.WIDTHS_ROWS
PHENO_BLOCK = SM.PHENO_BLOCK  # kGlmScoreSparsePb
LONG = SM.LONG                # kGlmSparseLong
SCRATCH_ENV = SM.SCRATCH_ENV
SUBSET_SHAPES = ["all_but_one", "last_word", "word_block", "tile_plus_one", "stride4"]  # test_glm_score_sparse_multi's
SUBSET_CUTOFF = 1.0           # 130 rows and a few hundred samples: more rows beyond it than beyond 2


# ---- inputs and the oracle ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(n):
    return SP.ParityInputs(n, seed=SEEDS[n])


def max_minors(n, thinned=False):
    """The forms the single-phenotype test opens its files in: the default rule, dense beyond one entry, all sparse.
    The width cases take the last two: every row from its entries (the wave form, and the long row in the workgroup
    form), and every row of more than one entry from its pool row (the workgroup form)."""
    return (n, 1) if thinned else (0, 1, n)


@functools.lru_cache(maxsize=None)
def phenotypes(n):
    """test_glm_score_multi_spa's three (the inputs' own y, a 2 % one without NaN, a 30 % one with a tenth NaN) and a
    15 % phenotype that shares the first one's NaN pattern."""
    case = inputs(n)
    rng = np.random.default_rng(9100 + n)
    shared = (rng.random(n) < 0.15).astype(np.float64)
    shared[np.isnan(case.y)] = NAN
    return np.vstack([MS.phenotypes(case), shared[None, :]])


@functools.lru_cache(maxsize=None)
def null_of(n, k, p):
    nul = O.Null(phenotypes(n)[p], inputs(n).covariates(k))
    assert nul.status is None, (n, k, p, nul.status)
    return nul


@functools.lru_cache(maxsize=None)
def oracle_rows(n, k, p, thinned=False):
    """Per variant {(base, dense_form): (row, p_spa, state)} of phenotype p for every form of max_minors(n); None where
    `thinned` leaves the variant out.  The oracle asserts that it decides every row."""
    case = inputs(n)
    nul = null_of(n, k, p)
    out = [None] * case.m
    for i in (WIDTHS_ROWS if thinned else range(case.m)):
        out[i] = {}
        for mm in max_minors(n, thinned):
            form = S.row_form(case.geno[i], mm)
            if form not in out[i]:
                out[i][form] = S.spa_row(case.x[i], case.geno[i], nul, form[0], form[1], CUTOFF)
    return out


def entries_of(codes, form):
    """How many entries the row holds: what decides the wave or the workgroup form (a dense-form row: the latter)."""
    return int((codes != form[0]).sum())


def is_group_form(codes, form):
    return form[1] or entries_of(codes, form) > LONG


def check_column(got, p, want, codes, max_minor, tol, ctx=None):
    """Column p of the dict against oracle_rows' rows under max_minor.  Returns (applied, failed, worst)."""
    applied, failed, worst = 0, 0, 0.0
    for i, forms in enumerate(want):
        if forms is None:
            continue
        row, p_spa, state = forms[S.row_form(codes[i], max_minor)]
        g_p, g_spa, g_state = got["p"][i, p], got["p_spa"][i, p], got["spa_state"][i, p]
        at = (ctx, i, p, row, p_spa, state, g_p, g_spa, g_state, got["errcode"][i, p])
        assert got["errcode"][i, p] == row["errcode"], at
        assert g_state == state, at
        if row["errcode"] is not None:
            assert math.isnan(g_spa), at
        elif state != 1:
            assert g_spa == g_p, at
            failed += state == 2
        else:
            diff = abs(g_spa - p_spa) / p_spa
            worst = max(worst, diff)
            assert diff <= tol, (diff, at)
            applied += 1
    return applied, failed, worst


def input_conditions(n, k, thinned):
    """The issue's conditions on the inputs of one (n, k), from the oracle alone."""
    case = inputs(n)
    cols = [oracle_rows(n, k, p, thinned) for p in range(len(phenotypes(n)))]
    rows = [i for i in range(case.m) if cols[0][i] is not None]
    dense_applied = base3_applied = False
    per_variant = {}
    for p, col in enumerate(cols):
        wave = group = 0
        for i in rows:
            for form, (row, p_spa, state) in col[i].items():
                if state != 1:
                    continue
                if is_group_form(case.geno[i], form):
                    group += 1
                else:
                    wave += 1
                dense_applied |= form[1]
                base3_applied |= form[0] == 3 and not form[1]
        print(f"n={n} k={k} phenotype {p}: applied in the wave form {wave}, in the workgroup form {group}")
        assert wave >= 1 and group >= 1, (n, k, p, wave, group)
    for mm in max_minors(n, thinned):
        counts = [sum(col[i][S.row_form(case.geno[i], mm)][2] == 1 for col in cols) for i in rows]
        per_variant[mm] = counts
        print(f"n={n} k={k} max_minor={mm}: variants with 0 / 1 / 2+ applied phenotypes: "
              f"{counts.count(0)} / {counts.count(1)} / {sum(c >= 2 for c in counts)}")
        assert counts.count(0) and counts.count(1) and any(c >= 2 for c in counts), (n, k, mm)
    assert dense_applied and base3_applied, (n, k, dense_applied, base3_applied)


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse_multi_spa(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse_multi_spa")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_sparse_multi_spa_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_sparse_multi_spa(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse_multi_spa(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def test_a_null_dataset_is_refused_with_the_outputs_untouched(lib):
    out, p_spa, state = MS._fill(4, 32)
    eb = C.create_string_buffer(lib.ERRBUF_LEN)
    y = np.array([[0.0, 1.0]])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.raw().pgh_glm_score_sparse_multi_spa(None, None, 0, 4, 1, p(y), 0, None, C.c_double(CUTOFF), p(out),
                                                  p(p_spa), p(state), eb)
    assert rc == lib.PGH_ERR_ARG and eb.value and MS._untouched(out, p_spa, state)


def test_the_fourth_phenotype_shares_the_first_ones_pattern():
    for n in PARITY_N:
        Y = phenotypes(n)
        assert len(Y) == 4 and len(set(y.tobytes() for y in Y)) == 4
        assert np.array_equal(np.isnan(Y[3]), np.isnan(Y[0])) and np.isnan(Y[0]).any()
        assert not np.isnan(Y[1]).any() and not np.array_equal(np.isnan(Y[2]), np.isnan(Y[0]))


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_reach_every_case(n, k):
    """Conditions on the inputs, not on the device, so that no device test can pass on rows that are left alone: the
    oracle decides every row of every phenotype under every form (it asserts where the contract does not, so no row is
    left out of the comparison); every phenotype has applied rows in the wave form and in the workgroup form; some
    variant has at least two applied phenotypes, some exactly one, some none; a dense-form row and a base-3 row are
    applied."""
    input_conditions(n, k, thinned=False)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_reach_every_case(k):
    """The same conditions on the rows test_every_instantiated_width checks, at every width."""
    input_conditions(WIDTHS_N, k, thinned=True)


@functools.lru_cache(maxsize=None)
def subset_inputs():
    """(codes, Z, Y) over the raw samples of the structured-subset cases: subset_shapes' rare matrix and its phenotype,
    a 30 % phenotype with NaN of its own and one more that shares the first one's pattern (it has none)."""
    n = SS.N_SMALL
    codes, y = SS.rare_codes(n)
    rng = np.random.default_rng(31 + n)
    other = (rng.random(n) < 0.3).astype(np.float64)
    other[rng.random(n) < 0.1] = NAN
    shared = (rng.random(n) < 0.2).astype(np.float64)
    return codes, SS.covariates(n), np.stack([y, other, shared])


@functools.lru_cache(maxsize=None)
def subset_oracle(shape):
    """Per phenotype the oracle's rows on the subset's samples, every row held sparse (the form comes from all raw
    samples)."""
    codes, Z, Y = subset_inputs()
    mask = SS.shapes(SS.N_SMALL)[shape]
    x = SS.values(codes)[:, mask]
    cols = []
    for y in Y[:, mask]:
        nul = O.Null(y, Z[:, mask])
        assert nul.status is None, (shape, nul.status)
        cols.append([{S.row_form(codes[i], SS.N_SMALL): S.spa_row(x[i], codes[i][mask], nul,
                                                                 *S.row_form(codes[i], SS.N_SMALL), SUBSET_CUTOFF)}
                     for i in range(len(codes))])
    return cols


@pytest.mark.parametrize("shape", SUBSET_SHAPES)
def test_the_subset_inputs_have_applied_rows(shape):
    cols = subset_oracle(shape)
    applied = [sum(w[2] == 1 for forms in col for w in forms.values()) for col in cols]
    print(f"{shape}: {applied} applied")
    assert min(applied) >= 3, (shape, applied)


# ---- on the GPU --------------------------------------------------------------------------------------------------

_col, _rows, _same_rows, _same = MS._col, MS._rows, MS._same_rows, MS._same


class _File:
    """The parity inputs as a .pgen of every record type, with the four phenotypes."""

    def __init__(self, L, tmp, n):
        self.L, self.case = L, inputs(n)
        self.n, self.m = n, self.case.m
        self.Y = phenotypes(n)
        self.path = str(tmp / f"sparse_multi_spa_{n}.pgen")
        W.write_pgen(self.path, self.case.geno, self.case.kinds)

    def sparse(self, **kw):
        # several windows per open, so that parts are concatenated and windows start after LD bases
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("PGH_SPARSE_WINDOW_BYTES", str(97 * ((self.n + 3) // 4 + 15) // 16 * 16))
            return self.L.Dataset.open(self.path, sparse=True, **kw)


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_multi_spa")
    return {n: _File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.fixture(scope="module")
def case_4099(files):
    """n = 4099, k = 3, every row held sparse: the dataset, the covariates and the whole-range result that the
    bit-for-bit tests share."""
    f = files[4099]
    Z = f.case.covariates(3)
    sp = f.sparse(max_minor=f.n)
    yield types.SimpleNamespace(f=f, sp=sp, Z=Z, whole=sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=CUTOFF))
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle_for_every_form(gpu_lib, files, n, k):
    f = files[n]
    zc = f.case.covariates(k) if k else None
    for max_minor in max_minors(n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_spa(f.Y, zc, spa_cutoff=CUTOFF)
        assert got["p_spa"].shape == (f.m, len(f.Y)) and got["spa_state"].shape == (f.m, len(f.Y))
        assert got["p_spa"].dtype == np.float64 and got["spa_state"].dtype == np.uint8
        _same_rows(got, sp.glm_score_sparse_multi(f.Y, zc), ctx=(n, k, max_minor))
        for p in range(len(f.Y)):
            want = oracle_rows(n, k, p)
            applied, failed, worst = check_column(got, p, want, f.case.geno, max_minor, TOL, ctx=(n, k, max_minor))
            print(f"n={n} k={k} max_minor={max_minor} phenotype {p}: {applied} applied, {failed} failed, worst "
                  f"{worst:.3g} (TOL {TOL:.3g})")
            # (how many rows of which kind the oracle applies: test_the_parity_inputs_reach_every_case)
            assert applied == sum(w[S.row_form(f.case.geno[i], max_minor)][2] == 1 for i, w in enumerate(want)) >= 1
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_the_one_phenotype_route_agrees(gpu_lib, files, n):
    """Column p against glm_score_sparse_spa() of phenotype p alone, k = 3, every form: E is the same set, the states
    are equal, and p_spa is within 2 x TOL (both are within TOL of the oracle)."""
    f = files[n]
    Z = f.case.covariates(3)
    for max_minor in max_minors(n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
        for p, y in enumerate(f.Y):
            one = sp.glm_score_sparse_spa(y, Z, cutoff=CUTOFF)
            assert got["errcode"][:, p].tolist() == list(one["errcode"]), (n, max_minor, p)
            assert got["spa_state"][:, p].tolist() == one["spa_state"].tolist(), (n, max_minor, p)
            at = one["spa_state"] == 1
            diff = np.abs(got["p_spa"][at, p] - one["p_spa"][at]) / one["p_spa"][at]
            print(f"n={n} max_minor={max_minor} phenotype {p}: {int(at.sum())} applied on both routes, worst "
                  f"{diff.max():.3g}")
            assert at.sum() >= 7 and (diff <= 2 * TOL).all(), (n, max_minor, p, diff.max())
            rest = ~at & ~np.isnan(one["p_spa"])
            assert np.array_equal(got["p_spa"][rest, p], got["p"][rest, p])
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_the_dense_route_agrees_where_the_base_code_is_its_b(gpu_lib, files, n):
    """test_glm_score_multi_spa.test_the_sparse_route_agrees_where_its_base_code_is_the_dense_b's rule, for every
    phenotype: k = 3, every row held sparse; a row whose base code is the dense b (and not 3) has the same E on both
    routes, and each route is within its own tolerance of the same oracle value."""
    f = files[n]
    Z = f.case.covariates(3)
    dense = gpu_lib.Dataset.open(f.path)
    other = dense.glm_score_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    dense.close()
    sp = f.sparse(max_minor=n)
    got = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    sp.close()
    total = 0
    for p, y in enumerate(f.Y):
        in_s = ~np.isnan(y)
        applied, worst = 0, 0.0
        for i in range(f.m):
            base, dense_form = S.row_form(f.case.geno[i], n)
            assert not dense_form
            if base == 3 or base != MS.dense_base(f.case.geno[i], in_s)[0]:
                continue
            ctx = (n, i, p, base, got["spa_state"][i, p], other["spa_state"][i, p], got["p_spa"][i, p], other["p_spa"][i, p])
            assert got["errcode"][i, p] == other["errcode"][i, p], ctx
            assert got["spa_state"][i, p] == other["spa_state"][i, p], ctx
            if got["spa_state"][i, p] == 1:
                diff = abs(got["p_spa"][i, p] - other["p_spa"][i, p]) / other["p_spa"][i, p]
                worst = max(worst, diff)
                assert diff <= TOL + MS.TOL, (diff, ctx)
                applied += 1
        print(f"n={n} phenotype {p}: {applied} applied rows with the same E on both routes, worst {worst:.3g}")
        total += applied
    assert total >= (20 if n == 4099 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """GlmScoreSparseMultiSpaKernel<KP, TEAM> for every width GlmPadCovar returns, at k = KP and one above the width
    below: with every row held sparse and with every row of more than one entry in the dense form, on the thinned
    rows."""
    f = files[WIDTHS_N]
    Z = f.case.covariates(k)
    for max_minor in max_minors(f.n, True):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
        _same_rows(got, sp.glm_score_sparse_multi(f.Y, Z), ctx=(k, max_minor))
        total = 0
        for p in range(len(f.Y)):
            want = oracle_rows(WIDTHS_N, k, p, True)
            applied, failed, worst = check_column(got, p, want, f.case.geno, max_minor, TOL_WIDTHS, ctx=(k, max_minor))
            print(f"k={k} max_minor={max_minor} phenotype {p}: {applied} applied, {failed} failed, worst {worst:.3g} "
                  f"(TOL {TOL_WIDTHS:.3g})")
            total += applied
        assert total >= 15
        sp.close()


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_other_phenotypes_their_number_or_its_place(gpu_lib, case_4099):
    c = case_4099
    sp, Y, Z, whole = c.sp, c.f.Y, c.Z, c.whole
    assert all((whole["spa_state"][:, p] == 1).sum() >= 7 for p in range(len(Y)))
    _same(sp.glm_score_sparse_multi_spa(Y, Z), whole, ctx="again")
    for p in range(len(Y)):
        _same(_col(sp.glm_score_sparse_multi_spa(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))
    perm = [2, 0, 3, 1]
    moved = sp.glm_score_sparse_multi_spa(Y[perm], Z)
    for to, p in enumerate(perm):
        _same(_col(moved, to), _col(whole, p), ctx=("permuted", p))
    # n_pheno = 6, and 65, where a second pair block exists: the four cycled, and at position 64 a phenotype of its own
    six = sp.glm_score_sparse_multi_spa(np.stack([Y[i % len(Y)] for i in range(6)]), Z)
    for i in range(6):
        _same(_col(six, i), _col(whole, i % len(Y)), ctx=("six", i))
    own = (np.random.default_rng(17_003).random(c.f.n) < 0.25).astype(np.float64)
    own[::19] = NAN
    many = np.stack([Y[i % len(Y)] for i in range(PHENO_BLOCK)] + [own])
    wide = sp.glm_score_sparse_multi_spa(many, Z)
    alone = sp.glm_score_sparse_multi_spa(own[None, :], Z)
    assert (alone["spa_state"] == 1).sum() >= 7
    _same(_col(wide, PHENO_BLOCK), _col(alone, 0), ctx="65th")
    for i in (0, 7, 30, PHENO_BLOCK - 1):
        _same(_col(wide, i), _col(whole, i % len(Y)), ctx=("block", i))


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_range_the_window_the_chunk_or_the_scratch_budget(gpu_lib, case_4099):
    c = case_4099
    f, sp, Y, Z, whole = c.f, c.sp, c.f.Y, c.Z, c.whole
    _same(sp.glm_score_sparse_multi_spa(Y, Z, v_begin=37), _rows(whole, slice(37, None)), ctx="v_begin = 37")
    _same(sp.glm_score_sparse_multi_spa(Y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx="40 .. 333")
    empty = sp.glm_score_sparse_multi_spa(Y, Z, v_begin=77, v_end=77)
    assert empty["p_spa"].shape == (0, len(Y)) and empty["spa_state"].shape == (0, len(Y))
    # a window that starts after an LD base
    v0 = next(v for v in range(150, f.m) if f.case.kinds[v] in (2, 3))
    v1 = min(f.m, v0 + 150)
    part = f.sparse(max_minor=f.n, variant_begin=v0, variant_end=v1)
    _same(part.glm_score_sparse_multi_spa(Y, Z), _rows(whole, slice(v0, v1)), ctx=("window", v0))
    part.close()
    # The pair block takes 16 bytes x 4,099 samples = 65,584 per phenotype, a workgroup's stash as much, and a chunk
    # variant 317 bytes per phenotype (k = 3: 10 sums, 14 entries of {H_N, g_N}, a count, a 48-byte row, the 7 doubles
    # of [t, U, V], p_spa, the state and two list words) and 16 for the tile counts.  1 byte: one phenotype per block,
    # one stash, a chunk of one variant (a part of the range).  133,168 bytes = 2 x 65,584 + 2,000: one phenotype and
    # one stash fit, two phenotypes do not, and of the 67,584 bytes the block leaves a quarter is less than a stash, so
    # there is the one, and the 2,000 left are a chunk of six variants.  400,000 bytes: four phenotypes, a variant and a
    # stash fit with 4 x 65,584 + 1,284 + 65,584 = 329,204; a quarter of the 137,664 left is less than a stash, so there
    # is one, and the 72,080 after it are a chunk of 56 variants.
    before = os.environ.get(SCRATCH_ENV)
    for budget, lo, hi in ((1, 200, 260), (133_168, 0, f.m), (400_000, 0, f.m)):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(sp.glm_score_sparse_multi_spa(Y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx=budget)
    assert os.environ.get(SCRATCH_ENV) == before
    # under the default rule, where rows are walked from their pool rows
    dflt = f.sparse(max_minor=0)
    whole0 = dflt.glm_score_sparse_multi_spa(Y, Z)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(SCRATCH_ENV, "133168")
        _same(dflt.glm_score_sparse_multi_spa(Y, Z, v_begin=40, v_end=333), _rows(whole0, slice(40, 333)), ctx="default")
    dflt.close()


@pytest.mark.gpu
def test_cutoff(gpu_lib, files):
    f = files[257]
    Z = f.case.covariates(1)
    sp = f.sparse(max_minor=f.n)
    base = sp.glm_score_sparse_multi(f.Y, Z)
    never = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=math.inf)
    _same_rows(never, base, ctx="inf")
    assert not never["spa_state"].any()
    assert np.array_equal(never["p_spa"], base["p"], equal_nan=True)
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
    low = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=0.1)
    at2 = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=CUTOFF)
    at3 = sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=3.0)
    for got in (low, at2, at3):
        _same_rows(got, base)
    assert (low["spa_state"] == 1).sum() > (at2["spa_state"] == 1).sum() >= (at3["spa_state"] == 1).sum()
    # raising the cutoff only moves rows from state 1 to state 0, with p_spa = out.p
    for lo, hi, cut in ((low, at2, CUTOFF), (at2, at3, 3.0)):
        moved = (lo["spa_state"] != 0) & ~(np.abs(base["stat"]) > cut)
        assert moved.any()
        assert not hi["spa_state"][moved].any() and np.array_equal(hi["p_spa"][moved], base["p"][moved])
        assert np.array_equal(hi["spa_state"][~moved], lo["spa_state"][~moved])
        assert np.array_equal(hi["p_spa"][~moved], lo["p_spa"][~moved], equal_nan=True)
    # refused before anything is written
    Y = np.ascontiguousarray(f.Y)
    z = np.ascontiguousarray(Z)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for bad in (0.09, NAN):
        out, p_spa, state = MS._fill(f.m * len(Y), gpu_lib.GLM_ROW_DTYPE.itemsize)
        eb = C.create_string_buffer(gpu_lib.ERRBUF_LEN)
        rc = gpu_lib.raw().pgh_glm_score_sparse_multi_spa(sp._h, None, 0, f.m, len(Y), p(Y), 1, p(z), C.c_double(bad),
                                                          p(out), p(p_spa), p(state), eb)
        assert rc == gpu_lib.PGH_ERR_ARG and b"spa_cutoff must be at least 0.1" in eb.value, (bad, rc, eb.value)
        assert MS._untouched(out, p_spa, state)
        with pytest.raises(ValueError, match="spa_cutoff must be at least 0.1"):
            sp.glm_score_sparse_multi_spa(f.Y, Z, spa_cutoff=bad)
    sp.close()


@pytest.fixture(scope="module")
def subset_file(gpu_lib, tmp_path_factory):
    codes, _, _ = subset_inputs()
    path = str(tmp_path_factory.mktemp("glm_score_sparse_multi_spa_subsets") / "rare.pgen")
    W.write_pgen(path, codes, W.choose_kinds(codes, np.random.default_rng(7 * SS.N_SMALL)))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SUBSET_SHAPES)
def test_structured_sample_subsets(gpu_lib, subset_file, shape):
    """Against the oracle on the subset's samples, every row held sparse."""
    codes, Zr, Yr = subset_inputs()
    mask = SS.shapes(SS.N_SMALL)[shape]
    Z, Y = np.ascontiguousarray(Zr[:, mask]), np.ascontiguousarray(Yr[:, mask])
    sp = gpu_lib.Dataset.open(subset_file, sparse=True, max_minor=SS.N_SMALL)
    ss = sp.subset(mask)
    got = sp.glm_score_sparse_multi_spa(Y, Z, spa_cutoff=SUBSET_CUTOFF, subset=ss)
    _same_rows(got, sp.glm_score_sparse_multi(Y, Z, subset=ss), ctx=shape)
    for p, want in enumerate(subset_oracle(shape)):
        applied, failed, worst = check_column(got, p, want, codes, SS.N_SMALL, TOL, ctx=shape)
        print(f"{shape} ({int(mask.sum())} samples) phenotype {p}: {applied} applied, {failed} failed, worst {worst:.3g}")
        assert applied >= 3
    ss.close()
    sp.close()


@pytest.mark.gpu
def test_undecided_rows_and_a_null_fit_that_fails(gpu_lib, tmp_path):
    """test_glm_score_sparse's decision file (CONST_ALLELE, TOO_FEW_SAMPLES, SINGULAR_MATRIX) with a third phenotype
    that the covariate separates, so that its null fit fails: the undecided rows have NaN and state 0, and the failed
    fit decides only its own column."""
    path, geno, Y2 = SM._decision_file(tmp_path)
    n = geno.shape[1]
    Z = geno[5].astype(np.float64)[None, :]
    separated = (geno[5] > 0).astype(np.float64)
    assert O.Null(separated, Z).status is not None and all(O.Null(y, Z).status is None for y in Y2)
    Y = np.vstack([Y2, separated[None, :]])
    sp = gpu_lib.Dataset.open(path, sparse=True, max_minor=n)
    got = sp.glm_score_sparse_multi_spa(Y, Z, spa_cutoff=0.1)
    _same_rows(got, sp.glm_score_sparse_multi(Y, Z))
    assert list(got["errcode"][:, 0]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                          "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    undecided = got["errcode"] != None  # noqa: E711
    assert np.isnan(got["p_spa"][undecided]).all() and not got["spa_state"][undecided].any()
    assert not np.isnan(got["p_spa"][~undecided]).any() and (got["spa_state"][~undecided] != 0).any()
    assert undecided[:, 2].all() and not undecided[:, 0].all() and not undecided[:, 1].all()
    # the first two columns are what they are without the failing phenotype
    pair = sp.glm_score_sparse_multi_spa(Y2, Z, spa_cutoff=0.1)
    for p in range(2):
        _same(_col(got, p), _col(pair, p), ctx=("without the failing one", p))
        # ... and the one-phenotype route's states
        one = sp.glm_score_sparse_spa(Y2[p], Z, cutoff=0.1)
        assert got["spa_state"][:, p].tolist() == one["spa_state"].tolist()
    sp.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    group = L.Dataset.open_sharded(path, [0, 0])
    n = sp.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    ok = sp.glm_score_sparse_multi_spa(Y, v_begin=0, v_end=8)
    assert ok["p_spa"].shape == (8, 2) and ok["spa_state"].dtype == np.uint8

    def raw(ds, phen, n_pheno=None, cutoff=CUTOFF, null_p_spa=False, null_state=False, v0=0, v1=8):
        phen = np.ascontiguousarray(phen, dtype=np.float64)
        out, p_spa, state = MS._fill(max(1, v1 - v0) * len(phen), L.GLM_ROW_DTYPE.itemsize)
        eb = C.create_string_buffer(L.ERRBUF_LEN)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = L.raw().pgh_glm_score_sparse_multi_spa(ds._h, None, v0, v1, len(phen) if n_pheno is None else n_pheno, p(phen),
                                                    0, None, C.c_double(cutoff), p(out), None if null_p_spa else p(p_spa),
                                                    None if null_state else p(state), eb)
        return rc, eb.value.decode(), MS._untouched(out, p_spa, state)

    y_two = Y.copy()
    y_two[1, 4] = 2.0
    y_one = Y.copy()
    y_one[1] = 1.0
    y_one[1, ::5] = NAN
    cases = [
        ("needs a sparse-resident dataset", (dense, Y)),
        ("one device's dataset", (group, Y)),
        ("null p_spa or spa_state", (sp, Y, None, CUTOFF, True)),
        ("null p_spa or spa_state", (sp, Y, None, CUTOFF, False, True)),
        ("spa_cutoff must be at least 0.1", (sp, Y, None, 0.09)),
        ("spa_cutoff must be at least 0.1", (sp, Y, None, NAN)),
        ("at least one phenotype", (sp, Y, 0)),
        ("phenotype must be 0 or 1", (sp, y_two)),
        ("no cases or no controls", (sp, y_one)),
    ]
    for text, args in cases:
        rc, msg, untouched = raw(*args)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    for bad in (y_two, y_one):
        assert "(phenotype 1)" in raw(sp, bad)[1]
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse_multi_spa(Y, v_begin=0, v_end=8)
    # an empty range is fine
    rc, msg, untouched = raw(sp, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched
    for ds in (group, sp, dense):
        ds.close()
