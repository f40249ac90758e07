"""pgh_glm_score_sparse_multi_firth / Dataset.glm_score_sparse_multi_firth: the approximate Firth estimate (covariate
effects fixed at the null fit, the genotype coded against the row's base code) of the rows of the sparse many-phenotype
route beyond a cutoff, in one call.  Against the FP64 oracle (tests/glm_firth_sparse_oracle.py, one
glm_score_oracle.Null per phenotype) the errcodes and states are equal, the rows that are not applied carry NaN or
`out`'s beta, se and p bit for bit, and the applied rows are within TOL on |delta beta| / se, |delta se| / se and
|delta p| / p, for every form the file can be opened in; `out` is pgh_glm_score_sparse_multi's bit for bit with its
firth byte 0; the one-phenotype route and the dense route agree where the contract says so; and a row does not depend on
the other phenotypes, its place among them, n_pheno, the phenotype block, the range, the window, the variant chunk or
the scratch budget.

TOL is 100 x the worst difference between the numpy model of the route's accumulation order
(tools/glm_score_sparse_multi_firth_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is the
family's, for device exp / log1p and fma contraction.  The rows at the wave / workgroup edge, which are also the cases
at the widest null model (k = 20), are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_sparse_multi_firth_model.py --widths` prints.

State 2 (attempted and failed) is not reached on the GPU by these inputs, as in test_glm_score_multi_firth and
test_glm_score_sparse_firth: the oracle finds an estimate for every applied row
(test_the_parity_inputs_reach_every_case asserts that there is no state-2 row), in at most 10 evaluations."""

import ctypes as C
import functools
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_firth_sparse_oracle as FS
import glm_score_oracle as O
import glm_spa_oracle as S
import pgen_writer as W
import subset_shapes as SS
import test_glm_score_multi_firth as MF
import test_glm_score_sparse_firth as SF
import test_glm_score_sparse_multi as SM
import test_glm_score_sparse_multi_spa as MSPA
import test_glm_score_sparse_spa as SP

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse_multi_firth"]
MODEL_WORST = 1.56e-12  # printed by tools/glm_score_sparse_multi_firth_model.py
TOL = 100 * MODEL_WORST
MODEL_WORST_WIDTHS = 1.07e-13  # printed by tools/glm_score_sparse_multi_firth_model.py --widths
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
PARITY_N = MSPA.PARITY_N  # 257 and 4099: test_glm_score_sparse_multi_spa's 600-variant rare_matrix files (seeds 258, 4102)
PARITY_K = (0, 1, 3)
inputs, phenotypes, max_minors, null_of = MSPA.inputs, MSPA.phenotypes, MSPA.max_minors, MSPA.null_of
is_group_form = MSPA.is_group_form
PHENO_BLOCK = SM.PHENO_BLOCK  # kGlmScoreSparsePb
LONG = SM.LONG                # kGlmSparseLong
SCRATCH_ENV = SM.SCRATCH_ENV
SUBSET_SHAPES = MSPA.SUBSET_SHAPES
SUBSET_CUTOFF = MSPA.SUBSET_CUTOFF
FIRTH_KEYS = MF.FIRTH_KEYS
EDGE_N = 4099
EDGE_ENTRIES = (1023, 1024, 1025, 1026)  # the wave's LDS stash is full at 1,024 pairs; 1,025 is the workgroup list's
EDGE_CASES = 200
EDGE_TARGETS = (0, 2, 0, 2)  # the phenotype whose cases a row's carriers are drawn from, and in whose S all of them are
# found by a search on the CPU with the oracle (test_the_edge_rows_are_applied): at every k of EDGE_K no |stat| of any
# phenotype is within 1e-6 of the cutoff and every row is applied for its target phenotype
EDGE_SEED = 1000
EDGE_K = (0, 3, 20)


# ---- inputs and the oracle ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def score_rows(n, k, p):
    """glm_score_oracle's row of every variant for phenotype p (computed once: it does not depend on the form)."""
    case, nul = inputs(n), null_of(n, k, p)
    return [O.oracle_row(case.x[i], nul) for i in range(case.m)]


@functools.lru_cache(maxsize=None)
def oracle_rows(n, k, p):
    """Per variant {(base, dense_form): firth_row_sparse's tuple} of phenotype p for every form of max_minors(n).  The
    oracle asserts that it decides every row (no |stat| within 1e-6 of the cutoff)."""
    case, nul, rows = inputs(n), null_of(n, k, p), score_rows(n, k, p)
    out = []
    for i in range(case.m):
        forms = {}
        for mm in max_minors(n):
            form = S.row_form(case.geno[i], mm)
            if form not in forms:
                forms[form] = FS.firth_row_sparse(case.x[i], case.geno[i], nul, form[0], form[1], CUTOFF, row=rows[i])
        out.append(forms)
    return out


def want_column(n, k, p, max_minor):
    """firth_row_sparse's tuple per variant as Dataset.open(sparse=True, max_minor=...) holds the rows."""
    case = inputs(n)
    return [forms[S.row_form(case.geno[i], max_minor)] for i, forms in enumerate(oracle_rows(n, k, p))]


def _col(out, p, rows=slice(None)):
    return {key: v[rows, p] for key, v in out.items()}


def check_column(got, p, want, x, codes, max_minor, tol):
    """Column p of the dict against firth_row_sparse's tuples: glm_firth_sparse_oracle.check_firth's assertions."""
    return FS.check_firth(_col(got, p), x, codes, None, max_minor, None, tol, want=want)


@functools.lru_cache(maxsize=None)
def edge_rows():
    """Four hom-ref-majority rows over inputs(EDGE_N)'s samples with exactly EDGE_ENTRIES entries, made the way
    test_glm_score_sparse_firth.edge_rows makes its four: codes 1 and 2, all on samples with the row's target
    phenotype, EDGE_CASES of them its cases.  Each is a wave's row up to 1,024 entries and the workgroup's beyond; for
    the target phenotype E is all of the entries."""
    Y = phenotypes(EDGE_N)
    rng = np.random.default_rng(EDGE_SEED)
    geno = np.zeros((len(EDGE_ENTRIES), EDGE_N), dtype=np.uint8)
    for v, (m, t) in enumerate(zip(EDGE_ENTRIES, EDGE_TARGETS)):
        cases, controls = np.flatnonzero(Y[t] == 1.0), np.flatnonzero(Y[t] == 0.0)
        pick = np.concatenate([rng.choice(cases, EDGE_CASES, replace=False),
                               rng.choice(controls, m - EDGE_CASES, replace=False)])
        geno[v, pick] = rng.integers(1, 3, m, dtype=np.uint8)
        assert int((geno[v] != 0).sum()) == m
    return geno


@functools.lru_cache(maxsize=None)
def edge_oracle(k):
    """(x, per phenotype firth_row_sparse's tuples of the four rows)"""
    case, geno = inputs(EDGE_N), edge_rows()
    x = SP._values(geno)
    cols = []
    for p, y in enumerate(phenotypes(EDGE_N)):
        nul = null_of(EDGE_N, k, p) if k in PARITY_K else O.Null(y, case.covariates(k))
        assert nul.status is None, (k, p, nul.status)
        cols.append([FS.firth_row_sparse(x[v], geno[v], nul, 0, False, CUTOFF) for v in range(len(geno))])
    return x, cols


@functools.lru_cache(maxsize=None)
def subset_oracle(shape):
    """Per phenotype firth_row_sparse's tuples on the subset's samples of test_glm_score_sparse_multi_spa's
    subset_inputs, every row held sparse (the form comes from all raw samples)."""
    codes, Z, Y = MSPA.subset_inputs()
    mask = SS.shapes(SS.N_SMALL)[shape]
    x = SS.values(codes)[:, mask]
    cols = []
    for y in Y[:, mask]:
        nul = O.Null(y, Z[:, mask])
        assert nul.status is None, (shape, nul.status)
        cols.append([FS.firth_row_sparse(x[i], codes[i][mask], nul, *S.row_form(codes[i], SS.N_SMALL), SUBSET_CUTOFF)
                     for i in range(len(codes))])
    return cols


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse_multi_firth(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse_multi_firth")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_glm_score_sparse_multi_firth_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_sparse_multi_firth(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse_multi_firth(fake, np.zeros((2, 5)), np.zeros((2, 4)))


@pytest.mark.parametrize("cutoff", [NAN, 0.0999, -1.0])
def test_glm_score_sparse_multi_firth_rejects_a_cutoff_below_a_tenth(lib, cutoff):
    """... and so does the cutoff check."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        lib.Dataset.glm_score_sparse_multi_firth(fake, np.zeros((2, 5)), firth_cutoff=cutoff)


_fill, _untouched, _ptr = SF._fill, SF._untouched, SF._ptr


def _raw(L, handle, Y, Z, cutoff, v0, v1, n_pheno=None, null_firth=False):
    """The C call on prefilled buffers: (rc, message, out bytes, firth bytes)."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Z = None if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    out, firth = _fill(L, max(1, v1 - v0) * len(Y))
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = L.raw().pgh_glm_score_sparse_multi_firth(handle, None, v0, v1, len(Y) if n_pheno is None else n_pheno, _ptr(Y),
                                                  0 if Z is None else len(Z), None if Z is None else _ptr(Z),
                                                  C.c_double(cutoff), _ptr(out), None if null_firth else _ptr(firth), eb)
    return rc, eb.value.decode(), out, firth


def test_a_null_dataset_a_null_firth_and_a_bad_cutoff_are_refused_with_the_outputs_untouched(lib):
    Y = np.array([[0.0, 1.0]])
    rc, msg, out, firth = _raw(lib, None, Y, None, CUTOFF, 0, 4)
    assert rc == lib.PGH_ERR_ARG and msg and _untouched(out, firth)
    rc, msg, out, firth = _raw(lib, None, Y, None, CUTOFF, 0, 4, null_firth=True)
    assert rc == lib.PGH_ERR_ARG and "null firth" in msg and _untouched(out, firth)
    for cutoff in (NAN, 0.0999, -1.0):  # the cutoff is checked before the dataset is looked at
        rc, msg, out, firth = _raw(lib, None, Y, None, cutoff, 0, 4)
        assert rc == lib.PGH_ERR_ARG and "firth_cutoff must be at least 0.1" in msg and _untouched(out, firth), cutoff


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_reach_every_case(n, k):
    """Conditions on the inputs, not on the device, so that no device test can pass on rows that are left alone: the
    oracle decides every row of every phenotype under every form (it asserts where the contract does not); nothing
    fails (no state 2); every phenotype has applied rows in the wave form and in the workgroup form; under every form
    some variant has at least two applied phenotypes, some exactly one, some none; a dense-form row and a base-3 row
    are applied; no row takes more than 10 evaluations."""
    case = inputs(n)
    cols = [oracle_rows(n, k, p) for p in range(len(phenotypes(n)))]
    dense_applied = base3_applied = False
    evals = 0
    for p, col in enumerate(cols):
        wave = group = 0
        for i, forms in enumerate(col):
            for form, w in forms.items():
                assert w[4] != 2, (n, k, p, i, form)
                if w[4] != 1:
                    continue
                evals = max(evals, w[5]["evals"])
                if is_group_form(case.geno[i], form):
                    group += 1
                else:
                    wave += 1
                dense_applied |= form[1]
                base3_applied |= form[0] == 3 and not form[1]
        print(f"n={n} k={k} phenotype {p}: applied in the wave form {wave}, in the workgroup form {group}")
        assert wave >= 1 and group >= 1, (n, k, p, wave, group)
    for mm in max_minors(n):
        counts = [sum(col[i][S.row_form(case.geno[i], mm)][4] == 1 for col in cols) for i in range(case.m)]
        print(f"n={n} k={k} max_minor={mm}: variants with 0 / 1 / 2+ applied phenotypes: "
              f"{counts.count(0)} / {counts.count(1)} / {sum(c >= 2 for c in counts)}")
        assert counts.count(0) and counts.count(1) and any(c >= 2 for c in counts), (n, k, mm)
    print(f"n={n} k={k}: at most {evals} evaluations")
    assert dense_applied and base3_applied and evals <= 10, (n, k, dense_applied, base3_applied, evals)


@pytest.mark.parametrize("k", EDGE_K)
def test_the_edge_rows_are_applied(k):
    """Every row is applied for its target phenotype, where E is all of its entries, so the four rows together are
    applied for two different phenotypes; nothing fails."""
    x, cols = edge_oracle(k)
    states = [[w[4] for w in col] for col in cols]
    print(f"k={k}: states per phenotype {states}, |stat| "
          f"{[[round(abs(w[0]['stat']), 2) for w in col] for col in cols]}")
    assert not any(s == 2 for col in states for s in col)
    for v, t in enumerate(EDGE_TARGETS):
        w = cols[t][v]
        assert w[0]["errcode"] is None and w[4] == 1 and w[5]["n_e"] == EDGE_ENTRIES[v], (k, v, t, w)
    assert len(set(EDGE_TARGETS)) >= 2


@pytest.mark.parametrize("shape", SUBSET_SHAPES)
def test_the_subset_inputs_have_applied_rows(shape):
    cols = subset_oracle(shape)
    applied = [sum(w[4] == 1 for w in col) for col in cols]
    print(f"{shape}: {applied} applied")
    assert min(applied) >= 3 and not any(w[4] == 2 for col in cols for w in col), (shape, applied)


# ---- on the GPU --------------------------------------------------------------------------------------------------

_rows, _same_rows, _same = MF._rows, MF._same_rows, MF._same


def _as_score_rows(got, base, ctx=None):
    """`out` is glm_score_sparse_multi's bit for bit, with its firth byte 0."""
    _same_rows(got, base, ctx)
    assert not got["firth"].any(), ctx


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_multi_firth")
    return {n: MSPA._File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.fixture(scope="module")
def case_4099(files):
    """n = 4099, k = 3, every row held sparse: the dataset, the covariates and the whole-range result that the
    bit-for-bit tests share."""
    f = files[4099]
    Z = f.case.covariates(3)
    sp = f.sparse(max_minor=f.n)
    yield types.SimpleNamespace(f=f, sp=sp, Z=Z, whole=sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=CUTOFF))
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle_for_every_form(gpu_lib, files, n, k):
    f = files[n]
    zc = f.case.covariates(k) if k else None
    shape = (f.m, len(f.Y))
    for max_minor in max_minors(n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_firth(f.Y, zc, firth_cutoff=CUTOFF)
        for key in FIRTH_KEYS:
            assert got[key].shape == shape and got[key].dtype == np.float64
        assert got["firth_state"].shape == shape and got["firth_state"].dtype == np.uint8
        _as_score_rows(got, sp.glm_score_sparse_multi(f.Y, zc), ctx=(n, k, max_minor))
        for p in range(len(f.Y)):
            want = want_column(n, k, p, max_minor)
            s = check_column(got, p, want, f.case.x, f.case.geno, max_minor, TOL)
            print(f"n={n} k={k} max_minor={max_minor} phenotype {p}: {s['applied']} applied, {s['failed']} failed, worst "
                  f"{s['worst']:.3g} (TOL {TOL:.3g})")
            # (how many rows of which kind the oracle applies: test_the_parity_inputs_reach_every_case)
            assert s["applied"] == sum(w[4] == 1 for w in want) >= 1 and s["failed"] == 0
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_the_one_phenotype_route_agrees(gpu_lib, files, n):
    """Column p against glm_score_sparse_firth() of phenotype p alone, k = 3, every form: E is the same set, the
    errcodes and states are equal, and the applied rows are within 2 x TOL (both are within TOL of the oracle)."""
    f = files[n]
    Z = f.case.covariates(3)
    for max_minor in max_minors(n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
        for p, y in enumerate(f.Y):
            one = sp.glm_score_sparse_firth(y, Z, firth_cutoff=CUTOFF)
            assert got["errcode"][:, p].tolist() == list(one["errcode"]), (n, max_minor, p)
            assert got["firth_state"][:, p].tolist() == one["firth_state"].tolist(), (n, max_minor, p)
            at = np.flatnonzero(one["firth_state"] == 1)
            worst, equal = 0.0, 0
            for i in at:
                a = [got[key][i, p] for key in FIRTH_KEYS]
                b = [one[key][i] for key in FIRTH_KEYS]
                worst = max(worst, *FS.scales(*a, *b))
                equal += all(FS.same_bits(u, v) for u, v in zip(a, b))
            print(f"n={n} max_minor={max_minor} phenotype {p}: {len(at)} applied on both routes, {equal} of them "
                  f"byte-equal, worst {worst:.3g}")
            assert len(at) >= 7 and worst <= 2 * TOL, (n, max_minor, p, worst)
            rest = (one["firth_state"] != 1) & ~np.isnan(one["p_firth"])
            for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
                assert np.array_equal(got[key][rest, p], got[of][rest, p]), (key, n, max_minor, p)
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_the_dense_route_agrees_where_E_is_its_E(gpu_lib, files, n):
    """Base-0, base-3 and dense-form rows have the dense route's E (test_glm_score_sparse_firth's rule), for every
    phenotype: k = 3, under the default form and with every row held sparse.  The states are equal and each route is
    within its own tolerance of the same oracle value."""
    f = files[n]
    Z = f.case.covariates(3)
    dense = gpu_lib.Dataset.open(f.path)
    ref = dense.glm_score_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
    dense.close()
    for max_minor in (0, n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
        sp.close()
        applied, worst = 0, 0.0
        for i in range(f.m):
            base, dense_form = S.row_form(f.case.geno[i], max_minor)
            if not (dense_form or base in (0, 3)):
                continue
            for p in range(len(f.Y)):
                ctx = (n, max_minor, i, p, base, dense_form)
                assert got["errcode"][i, p] == ref["errcode"][i, p], ctx
                assert got["firth_state"][i, p] == ref["firth_state"][i, p], ctx
                if got["firth_state"][i, p] == 1:
                    a = [got[key][i, p] for key in FIRTH_KEYS]
                    b = [ref[key][i, p] for key in FIRTH_KEYS]
                    diff = max(FS.scales(*a, *b))
                    worst = max(worst, diff)
                    assert diff <= TOL + MF.TOL, (diff, ctx, a, b)
                    applied += 1
        print(f"n={n} max_minor={max_minor}: {applied} applied rows with the dense route's E, worst {worst:.3g}")
        assert applied >= (20 if n == 4099 else 1)


@pytest.fixture(scope="module")
def edge_file(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("glm_score_sparse_multi_firth_edge") / "edge.pgen")
    W.write_pgen(path, edge_rows(), [0] * len(EDGE_ENTRIES))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_the_wave_workgroup_edge(gpu_lib, edge_file, k):
    """1,023 and 1,024 entries are on the wave list, and 1,024 pairs fill a wave's LDS stash; 1,025 and 1,026 are on
    the workgroup list."""
    case, Y = inputs(EDGE_N), phenotypes(EDGE_N)
    x, cols = edge_oracle(k)
    Z = case.covariates(k) if k else None
    sp = gpu_lib.Dataset.open(edge_file, sparse=True, max_minor=EDGE_N)
    info = sp.sparse_info()
    assert info.dense_variant_ct == 0 and info.sparse_variant_ct == len(EDGE_ENTRIES)
    got = sp.glm_score_sparse_multi_firth(Y, Z, firth_cutoff=CUTOFF)
    _as_score_rows(got, sp.glm_score_sparse_multi(Y, Z), ctx=k)
    for p, want in enumerate(cols):
        s = check_column(got, p, want, x, edge_rows(), EDGE_N, TOL_WIDTHS)
        print(f"k={k} phenotype {p}: {s['applied']} applied, worst {s['worst']:.3g} (TOL {TOL_WIDTHS:.3g})")
        assert s["applied"] == sum(w[4] == 1 for w in want) and s["failed"] == 0
        assert [r[4] for r in s["rows"]] == [EDGE_ENTRIES[r[0]] for r in s["rows"]]
    for v, t in enumerate(EDGE_TARGETS):
        assert got["firth_state"][v, t] == 1
    sp.close()


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_other_phenotypes_their_number_or_its_place(gpu_lib, case_4099):
    c = case_4099
    sp, Y, Z, whole = c.sp, c.f.Y, c.Z, c.whole
    assert all((whole["firth_state"][:, p] == 1).sum() >= 7 for p in range(len(Y)))
    _same(sp.glm_score_sparse_multi_firth(Y, Z), whole, ctx="again")
    # the same bytes, the padding included
    rc_a, _, out_a, firth_a = _raw(gpu_lib, sp._h, Y, Z, CUTOFF, 0, c.f.m)
    rc_b, _, out_b, firth_b = _raw(gpu_lib, sp._h, Y, Z, CUTOFF, 0, c.f.m)
    assert rc_a == rc_b == gpu_lib.PGH_OK
    assert out_a.tobytes() == out_b.tobytes() and firth_a.tobytes() == firth_b.tobytes()
    rows = firth_a.view(gpu_lib.GLM_FIRTH_ROW_DTYPE).reshape(c.f.m, len(Y))
    assert not rows["pad"].any() and rows["state"].tolist() == whole["firth_state"].tolist()
    for p in range(len(Y)):
        _same(_col(sp.glm_score_sparse_multi_firth(Y[p:p + 1], Z), 0), _col(whole, p), ctx=("alone", p))
    perm = [2, 0, 3, 1]
    moved = sp.glm_score_sparse_multi_firth(Y[perm], Z)
    for to, p in enumerate(perm):
        _same(_col(moved, to), _col(whole, p), ctx=("permuted", p))
    # n_pheno = 6, and 65, where a second pair block exists: the four cycled, and at position 64 a phenotype of its own
    six = sp.glm_score_sparse_multi_firth(np.stack([Y[i % len(Y)] for i in range(6)]), Z)
    for i in range(6):
        _same(_col(six, i), _col(whole, i % len(Y)), ctx=("six", i))
    own = (np.random.default_rng(17_003).random(c.f.n) < 0.25).astype(np.float64)
    own[::19] = NAN
    many = np.stack([Y[i % len(Y)] for i in range(PHENO_BLOCK)] + [own])
    wide = sp.glm_score_sparse_multi_firth(many, Z)
    alone = sp.glm_score_sparse_multi_firth(own[None, :], Z)
    assert (alone["firth_state"] == 1).sum() >= 7
    _same(_col(wide, PHENO_BLOCK), _col(alone, 0), ctx="65th")
    for i in (0, 7, 30, PHENO_BLOCK - 1):
        _same(_col(wide, i), _col(whole, i % len(Y)), ctx=("block", i))


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_the_window_the_chunk_or_the_scratch_budget(gpu_lib, case_4099):
    c = case_4099
    f, sp, Y, Z, whole = c.f, c.sp, c.f.Y, c.Z, c.whole
    _same(sp.glm_score_sparse_multi_firth(Y, Z, v_begin=37), _rows(whole, slice(37, None)), ctx="v_begin = 37")
    _same(sp.glm_score_sparse_multi_firth(Y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx="40 .. 333")
    empty = sp.glm_score_sparse_multi_firth(Y, Z, v_begin=77, v_end=77)
    assert all(empty[key].shape == (0, len(Y)) for key in FIRTH_KEYS + ("firth_state", "beta"))
    # a window that starts after an LD base
    v0 = next(v for v in range(150, f.m) if f.case.kinds[v] in (2, 3))
    v1 = min(f.m, v0 + 150)
    part = f.sparse(max_minor=f.n, variant_begin=v0, variant_end=v1)
    _same(part.glm_score_sparse_multi_firth(Y, Z), _rows(whole, slice(v0, v1)), ctx=("window", v0))
    part.close()
    # The pair block takes 16 bytes x 4,099 samples = 65,584 per phenotype, a workgroup's stash as much, and a chunk
    # variant 284 bytes per phenotype (k = 3: 10 sums, 14 entries of {H_N, g_N}, a count, a 48-byte row, the 32-byte
    # pgh_glm_firth_row where the saddlepoint call has 7 + 1 doubles and a state byte, and two list words) and 16 for
    # the tile counts.  1 byte: one phenotype per block, one stash, a chunk of one variant (a part of the range).
    # 133,168 bytes = 2 x 65,584 + 2,000: one phenotype, a variant and one stash fit (131,468), two phenotypes do not
    # (3 x 65,584 + 584 = 197,336), and of the 67,584 bytes the block leaves a quarter is less than a stash, so there
    # is the one, and the 2,000 left are a chunk of six variants at 300 bytes.  400,000 bytes: four phenotypes, a
    # variant and a stash fit with 4 x 65,584 + 1,152 + 65,584 = 329,072; a quarter of the 137,664 left is less than a
    # stash, so there is one, and the 72,080 after it are a chunk of 62 variants at 1,152 bytes.
    before = os.environ.get(SCRATCH_ENV)
    for budget, lo, hi in ((1, 200, 260), (133_168, 0, f.m), (400_000, 0, f.m)):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(sp.glm_score_sparse_multi_firth(Y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo, hi)), ctx=budget)
    assert os.environ.get(SCRATCH_ENV) == before
    # under the default rule, where rows are walked from their pool rows
    dflt = f.sparse(max_minor=0)
    whole0 = dflt.glm_score_sparse_multi_firth(Y, Z)
    assert (whole0["firth_state"] == 1).any()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv(SCRATCH_ENV, "133168")
        _same(dflt.glm_score_sparse_multi_firth(Y, Z, v_begin=40, v_end=333), _rows(whole0, slice(40, 333)), ctx="default")
    dflt.close()


@pytest.mark.gpu
def test_cutoff(gpu_lib, files):
    f = files[257]
    Z = f.case.covariates(1)
    sp = f.sparse(max_minor=f.n)
    base = sp.glm_score_sparse_multi(f.Y, Z)
    fitted = base["errcode"] == None  # noqa: E711
    assert fitted.any() and not fitted.all()
    never = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=math.inf)
    _as_score_rows(never, base, ctx="inf")
    assert not never["firth_state"].any()
    for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
        assert np.array_equal(never[key], base[of], equal_nan=True), key
        assert np.isnan(never[key][~fitted]).all() and not np.isnan(never[key][fitted]).any()
    low = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=0.1)
    at2 = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=CUTOFF)
    at3 = sp.glm_score_sparse_multi_firth(f.Y, Z, firth_cutoff=3.0)
    for got, cut in ((low, 0.1), (at2, CUTOFF), (at3, 3.0)):
        _as_score_rows(got, base, ctx=cut)
        # every fitted row beyond the cutoff is applied (or attempted), and no other
        assert np.array_equal(got["firth_state"] != 0, fitted & (np.abs(base["stat"]) > cut)), cut
    assert (low["firth_state"] == 1).sum() > (at2["firth_state"] == 1).sum() > (at3["firth_state"] == 1).sum() >= 1
    # a larger cutoff's applied set is a subset of a smaller one's, with the same bytes on the rows applied under both
    for lo, hi in ((low, at2), (at2, at3), (low, at3)):
        both = hi["firth_state"] != 0
        assert both.any() and (lo["firth_state"][both] == hi["firth_state"][both]).all()
        rest = ~both
        for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
            assert np.array_equal(hi[key][both], lo[key][both]), key
            assert np.array_equal(hi[key][rest], base[of][rest], equal_nan=True), key
    sp.close()


@pytest.fixture(scope="module")
def subset_file(gpu_lib, tmp_path_factory):
    codes, _, _ = MSPA.subset_inputs()
    path = str(tmp_path_factory.mktemp("glm_score_sparse_multi_firth_subsets") / "rare.pgen")
    W.write_pgen(path, codes, W.choose_kinds(codes, np.random.default_rng(7 * SS.N_SMALL)))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SUBSET_SHAPES)
def test_structured_sample_subsets(gpu_lib, subset_file, shape):
    """Against the oracle on the subset's samples, every row held sparse."""
    codes, Zr, Yr = MSPA.subset_inputs()
    mask = SS.shapes(SS.N_SMALL)[shape]
    Z, Y = np.ascontiguousarray(Zr[:, mask]), np.ascontiguousarray(Yr[:, mask])
    sp = gpu_lib.Dataset.open(subset_file, sparse=True, max_minor=SS.N_SMALL)
    ss = sp.subset(mask)
    got = sp.glm_score_sparse_multi_firth(Y, Z, firth_cutoff=SUBSET_CUTOFF, subset=ss)
    _as_score_rows(got, sp.glm_score_sparse_multi(Y, Z, subset=ss), ctx=shape)
    forms = [S.row_form(codes[i], SS.N_SMALL) for i in range(len(codes))]  # the form comes from all raw samples
    x = SS.values(codes)[:, mask]
    for p, want in enumerate(subset_oracle(shape)):
        s = check_column(got, p, want, x, codes[:, mask], forms, TOL)
        print(f"{shape} ({int(mask.sum())} samples) phenotype {p}: {s['applied']} applied, worst {s['worst']:.3g}")
        assert s["applied"] >= 3 and s["failed"] == 0
    ss.close()
    sp.close()


@pytest.mark.gpu
def test_undecided_rows_and_a_null_fit_that_fails(gpu_lib, tmp_path):
    """test_glm_score_sparse_multi_spa's construction: the decision file (CONST_ALLELE, TOO_FEW_SAMPLES,
    SINGULAR_MATRIX) with a third phenotype that the covariate separates, so that its null fit fails.  The undecided
    rows have NaN and state 0, and the failed fit decides only its own column."""
    path, geno, Y2 = SM._decision_file(tmp_path)
    n = geno.shape[1]
    Z = geno[5].astype(np.float64)[None, :]
    separated = (geno[5] > 0).astype(np.float64)
    assert O.Null(separated, Z).status is not None and all(O.Null(y, Z).status is None for y in Y2)
    Y = np.vstack([Y2, separated[None, :]])
    sp = gpu_lib.Dataset.open(path, sparse=True, max_minor=n)
    got = sp.glm_score_sparse_multi_firth(Y, Z, firth_cutoff=0.1)
    _as_score_rows(got, sp.glm_score_sparse_multi(Y, Z))
    assert list(got["errcode"][:, 0]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                          "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    undecided = got["errcode"] != None  # noqa: E711
    for key in FIRTH_KEYS:
        assert np.isnan(got[key][undecided]).all() and not np.isnan(got[key][~undecided]).any(), key
    assert not got["firth_state"][undecided].any() and (got["firth_state"][~undecided] != 0).any()
    assert undecided[:, 2].all() and not undecided[:, 0].all() and not undecided[:, 1].all()
    # the first two columns are what they are without the failing phenotype, bit for bit
    pair = sp.glm_score_sparse_multi_firth(Y2, Z, firth_cutoff=0.1)
    for p in range(2):
        _same(_col(got, p), _col(pair, p), ctx=("without the failing one", p))
        # ... and the one-phenotype route's states
        one = sp.glm_score_sparse_firth(Y2[p], Z, firth_cutoff=0.1)
        assert got["firth_state"][:, p].tolist() == one["firth_state"].tolist()
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
    ok = sp.glm_score_sparse_multi_firth(Y, v_begin=0, v_end=8)
    assert ok["beta_firth"].shape == (8, 2) and ok["firth_state"].dtype == np.uint8
    y_two = Y.copy()
    y_two[1, 4] = 2.0
    y_one = Y.copy()
    y_one[1] = 1.0
    y_one[1, ::5] = NAN
    cases = [
        ("needs a sparse-resident dataset", dict(handle=dense._h)),
        ("one device's dataset", dict(handle=group._h)),
        ("null firth", dict(null_firth=True)),
        ("firth_cutoff must be at least 0.1", dict(cutoff=0.0999)),
        ("firth_cutoff must be at least 0.1", dict(cutoff=NAN)),
        ("firth_cutoff must be at least 0.1", dict(cutoff=-1.0)),
        ("at least one phenotype", dict(n_pheno=0)),
        ("phenotype must be 0 or 1", dict(Y=y_two)),
        ("no cases or no controls", dict(Y=y_one)),
    ]
    for text, kw in cases:
        args = dict(handle=sp._h, Y=Y, Z=None, cutoff=CUTOFF, v0=0, v1=8)
        args.update(kw)
        rc, msg, out, firth = _raw(L, args.pop("handle"), args.pop("Y"), args.pop("Z"), args.pop("cutoff"),
                                   args.pop("v0"), args.pop("v1"), **args)
        assert rc == L.PGH_ERR_ARG and text in msg and _untouched(out, firth), (text, rc, msg)
        if "Y" in kw:
            assert "(phenotype 1)" in msg
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse_multi_firth(Y, v_begin=0, v_end=8)
    # an empty range is fine, and nothing is written
    rc, msg, out, firth = _raw(L, sp._h, Y, None, CUTOFF, 3, 3)
    assert rc == L.PGH_OK and _untouched(out, firth)
    for ds in (group, sp, dense):
        ds.close()
