"""pgh_glm_score_sparse_firth / Dataset.glm_score_sparse_firth: the approximate Firth estimate (covariate effects fixed
at the null fit, the genotype coded against the row's base code) of the sparse route's rows beyond a cutoff.  Against
the FP64 oracle (tests/glm_firth_sparse_oracle.py) the errcodes and states are equal, the rows that are not applied
carry NaN or `out`'s beta, se and p bit for bit, and the applied rows are within TOL on |delta beta| / se,
|delta se| / se and |delta p| / p; `out` is pgh_glm_score_sparse's bit for bit with its firth byte 0; a row does not
depend on the range, the window or the chunk; and the rows whose E is the dense route's agree with
pgh_glm_score_multi_firth.

TOL is 100 x the worst difference between the numpy model of the kernel's accumulation order
(tools/glm_score_sparse_firth_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is the
family's, for device exp / log1p and fma contraction.  The cases at every covariate width and at the wave / workgroup
edge are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_sparse_firth_model.py --widths` prints."""

import ctypes as C
import functools
import math
import os
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_firth_oracle as F
import glm_firth_sparse_oracle as FS
import glm_score_oracle as O
import glm_spa_oracle as S
import pgen_writer as W
import subset_shapes as SS
import test_glm_score_sparse_spa as T
from test_glm_score_sparse_spa import ParityInputs

NAN = float("nan")
NEW_SYMBOLS = ["pgh_glm_score_sparse_firth"]
MODEL_WORST = 3.47e-13  # printed by tools/glm_score_sparse_firth_model.py
TOL = 100 * MODEL_WORST
# printed by tools/glm_score_sparse_firth_model.py --widths: the width and edge cases below, on the rows they check
MODEL_WORST_WIDTHS = 1.29e-13
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
CUTOFF = 2.0
PARITY_N = (257, 4099)
PARITY_K = (0, 1, 3)
M_R = T.M_R
WIDTHS, WIDTHS_N, WIDTHS_ROWS = T.WIDTHS, T.WIDTHS_N, T.WIDTHS_ROWS
EDGE_N = 4099
EDGE_ENTRIES = (1023, 1024, 1025, 1026)  # the wave's LDS stash is full at 1,024 pairs
EDGE_CASES = 200
# found by a search on the CPU with the oracle: every row's |stat| lies between 8 and 12 at every k of EDGE_K (the
# covariates are shifted among the cases, so 20 of them take up a third of the score)
EDGE_SEED = 1045
EDGE_K = (0, 1, 3, 20)
FIRTH_KEYS = ("beta_firth", "se_firth", "p_firth")


# ---- inputs and the oracle ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(n):
    return ParityInputs(n)


def max_minors(n):
    return (0, 1, n)


@functools.lru_cache(maxsize=None)
def null_of(n, k):
    case = inputs(n)
    nul = O.Null(case.y, case.covariates(k))
    assert nul.status is None
    return nul


@functools.lru_cache(maxsize=None)
def score_rows(n, k):
    """glm_score_oracle's row of every variant of ParityInputs(n) with k covariates (computed once: it does not depend
    on the form)."""
    case, nul = inputs(n), null_of(n, k)
    return [O.oracle_row(case.x[i], nul) for i in range(case.m)]


@functools.lru_cache(maxsize=None)
def oracle_case(n, k, max_minor, cutoff=CUTOFF):
    """firth_row_sparse's tuple of every variant of ParityInputs(n) as Dataset.open(sparse=True, max_minor=...) holds
    it (computed once)."""
    case, nul, rows = inputs(n), null_of(n, k), score_rows(n, k)
    return [FS.firth_row_sparse(case.x[i], case.geno[i], nul, *S.row_form(case.geno[i], max_minor), cutoff, row=rows[i])
            for i in range(case.m)]


def applied_forms(n, k, max_minor):
    """(row, base, dense_form, |E|, entries, hom-ref entries) of the applied rows."""
    case = inputs(n)
    out = []
    for i, w in enumerate(oracle_case(n, k, max_minor)):
        if w[4] == 1:
            base, dense_form = S.row_form(case.geno[i], max_minor)
            entries = case.n if dense_form else int((case.geno[i] != base).sum())
            hom_ref = int((case.geno[i] == 0).sum()) if base == 3 and not dense_form else 0
            out.append((i, base, dense_form, w[5]["n_e"], entries, hom_ref))
    return out


@functools.lru_cache(maxsize=None)
def edge_rows():
    """Four hom-ref-majority rows over ParityInputs(EDGE_N)'s samples with exactly EDGE_ENTRIES entries: codes 1 and 2,
    all on samples with a phenotype, EDGE_CASES of them cases.  Each is a wave's row up to 1,024 entries and the
    workgroup's beyond."""
    case = inputs(EDGE_N)
    rng = np.random.default_rng(EDGE_SEED)
    cases, controls = np.flatnonzero(case.y == 1.0), np.flatnonzero(case.y == 0.0)
    geno = np.zeros((len(EDGE_ENTRIES), case.n), dtype=np.uint8)
    for v, m in enumerate(EDGE_ENTRIES):
        pick = np.concatenate([rng.choice(cases, EDGE_CASES, replace=False),
                               rng.choice(controls, m - EDGE_CASES, replace=False)])
        geno[v, pick] = rng.integers(1, 3, m, dtype=np.uint8)
        assert int((geno[v] != 0).sum()) == m
    return geno


@functools.lru_cache(maxsize=None)
def edge_oracle(k):
    case, geno = inputs(EDGE_N), edge_rows()
    nul = null_of(EDGE_N, k) if k in PARITY_K else O.Null(case.y, case.covariates(k))
    assert nul.status is None
    x = T._values(geno)
    return nul, x, [FS.firth_row_sparse(x[v], geno[v], nul, 0, False, CUTOFF) for v in range(len(geno))]


@functools.lru_cache(maxsize=None)
def widths_oracle(k, max_minor):
    """firth_row_sparse's tuples of WIDTHS_ROWS (None elsewhere) of ParityInputs(WIDTHS_N) with k covariates."""
    case = inputs(WIDTHS_N)
    nul = O.Null(case.y, case.covariates(k))
    assert nul.status is None
    out = [None] * case.m
    for i in WIDTHS_ROWS:
        out[i] = FS.firth_row_sparse(case.x[i], case.geno[i], nul, *S.row_form(case.geno[i], max_minor), CUTOFF)
    return nul, out


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_glm_score_sparse_firth(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert hasattr(lib.Dataset, "glm_score_sparse_firth")


@pytest.mark.parametrize("shape", [(4,), (6,), (1, 5)])
def test_glm_score_sparse_firth_rejects_arrays_of_the_wrong_shape(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotype"):
        lib.Dataset.glm_score_sparse_firth(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_sparse_firth(fake, np.zeros(5), np.zeros((2, 4)))


def _fill(L, n_rows):
    return (np.full(n_rows * L.GLM_ROW_DTYPE.itemsize, 0xAB, dtype=np.uint8),
            np.full(n_rows * L.GLM_FIRTH_ROW_DTYPE.itemsize, 0xCD, dtype=np.uint8))


def _untouched(out, firth):
    return bool((out == 0xAB).all() and (firth == 0xCD).all())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(L, handle, y, Z, cutoff, v0, v1, null_firth=False):
    """The C call on prefilled buffers: (rc, message, out bytes, firth bytes)."""
    out, firth = _fill(L, v1 - v0)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    y = np.ascontiguousarray(y, dtype=np.float64)
    Z = None if Z is None else np.ascontiguousarray(Z, dtype=np.float64)
    rc = L.raw().pgh_glm_score_sparse_firth(handle, None, v0, v1, _ptr(y), 0 if Z is None else len(Z),
                                            None if Z is None else _ptr(Z), C.c_double(cutoff), _ptr(out),
                                            None if null_firth else _ptr(firth), eb)
    return rc, eb.value.decode(), out, firth


@pytest.mark.parametrize("cutoff", [NAN, 0.0999, -1.0])
def test_a_cutoff_below_a_tenth_is_refused_with_the_outputs_untouched(lib, cutoff):
    """The cutoff is checked before the dataset is looked at."""
    rc, msg, out, firth = _raw(lib, None, np.array([0.0, 1.0]), None, cutoff, 0, 4)
    assert rc == lib.PGH_ERR_ARG and "firth_cutoff must be at least 0.1" in msg and _untouched(out, firth)


def test_a_null_dataset_and_a_null_firth_are_refused_with_the_outputs_untouched(lib):
    rc, msg, out, firth = _raw(lib, None, np.array([0.0, 1.0]), None, CUTOFF, 0, 4)
    assert rc == lib.PGH_ERR_ARG and msg and _untouched(out, firth)
    rc, msg, out, firth = _raw(lib, None, np.array([0.0, 1.0]), None, CUTOFF, 0, 4, null_firth=True)
    assert rc == lib.PGH_ERR_ARG and "null firth" in msg and _untouched(out, firth)


def test_the_oracle_F_and_H_are_the_derivatives_of_l_star_under_d_coding():
    """test_glm_score_multi_firth's check on the base-2 rows held sparse, where d is -2 or -1.  Central differences
    with h = 1e-4 / sqrt(K''(0)), a ten-thousandth of the null standard error of beta: the truncation error
    h^2 f''' / 6 is about 1e-8 of the derivative's scale and the rounding error eps |f| / h about 1e-12 |f|, so 1e-6
    of the scale (sqrt(K''(0)) + |G| for F, K''(0) for H) bounds both with room."""
    n, k = 257, 1
    case, nul = inputs(n), null_of(n, k)
    rows = checked = 0
    for i, (row, beta, se, pv, state, info) in enumerate(oracle_case(n, k, n)):
        base, dense_form = S.row_form(case.geno[i], n)
        if state != 1 or base != 2 or dense_form:
            continue
        cgf, n_e = FS.cgf_of(case.x[i], case.geno[i], nul, base, dense_form)
        assert n_e and set(cgf.x.tolist()) <= {-2.0, -1.0}
        k2_0 = cgf.k(0.0)[2]
        h = 1e-4 / math.sqrt(k2_0)
        rows += 1
        for b in (0.0, 0.5 * beta, beta, 2.0 * beta):
            ls, f, hh, k2, was_replaced = cgf.at(b)
            d1 = (cgf.lstar(b + h) - cgf.lstar(b - h)) / (2 * h)
            assert abs(d1 - f) <= 1e-6 * (math.sqrt(k2_0) + abs(cgf.g)), (i, b, d1, f)
            if not was_replaced:
                d2 = (cgf.at(b + h)[1] - cgf.at(b - h)[1]) / (2 * h)
                assert abs(-d2 - hh) <= 1e-6 * k2_0, (i, b, d2, hh)
                checked += 1
    print(f"{rows} base-2 rows, {checked} points with H checked")
    assert rows >= 3 and checked >= 8


def test_the_oracle_is_the_dense_oracle_where_E_is_the_dense_route_s():
    """Base 0, base 3 and dense-form rows: the same E, d = x, so the same numbers."""
    n, k = 257, 1
    case, nul = inputs(n), null_of(n, k)
    applied = {0: 0, 3: 0, "dense": 0}
    for max_minor in max_minors(n):
        for i, w in enumerate(oracle_case(n, k, max_minor)):
            base, dense_form = S.row_form(case.geno[i], max_minor)
            if not (dense_form or base in (0, 3)):
                continue
            row, beta, se, pv, state, info = F.firth_row(case.x[i], case.geno[i], nul, CUTOFF)
            assert w[4] == state and info["evals"] == w[5]["evals"]
            if state == 1:
                assert (w[1], w[2], w[3]) == (beta, se, pv), (i, max_minor)
                applied["dense" if dense_form else base] += 1
    print(applied)
    assert all(applied.values())


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_the_parity_inputs_reach_the_cases_of_the_contract(n, k):
    """Conditions on the inputs, not on the device, so that the GPU tests cannot pass on empty ground."""
    for max_minor in max_minors(n):
        col = oracle_case(n, k, max_minor)  # (the oracle asserts that no |stat| is within 1e-6 of the cutoff)
        forms = applied_forms(n, k, max_minor)
        evals = max(w[5]["evals"] for w in col)
        print(f"n={n} k={k} max_minor={max_minor}: {len(forms)} applied, at most {evals} evaluations, "
              f"bases held sparse {sorted({f[1] for f in forms if not f[2]})}, {sum(f[2] for f in forms)} dense-form")
        assert len(forms) >= 32, (n, k, max_minor)
        assert not any(w[4] == 2 for w in col), (n, k, max_minor)
        assert evals <= 10, (n, k, max_minor)
    forms = applied_forms(n, k, n)
    assert {0, 1, 2, 3} <= {f[1] for f in forms if not f[2]}, (n, k)
    if n == 4099:
        assert any(f[4] > 1024 for f in forms) and any(f[4] <= 1024 for f in forms)
    if k in (0, 3):
        assert any(f[1] == 3 and f[5] > 0 for f in forms), (n, k)


@pytest.mark.parametrize("k", EDGE_K)
def test_the_edge_rows_are_fitted_and_applied(k):
    nul, x, want = edge_oracle(k)
    stats = [abs(w[0]["stat"]) for w in want]
    print(f"k={k}: |stat| {[round(s, 2) for s in stats]}, evaluations {[w[5]['evals'] for w in want]}")
    assert all(w[0]["errcode"] is None and w[4] == 1 for w in want)
    assert all(8.0 < s < 12.0 for s in stats)
    assert [w[5]["n_e"] for w in want] == list(EDGE_ENTRIES)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_at_every_width(k):
    for max_minor in (WIDTHS_N, 0):
        _, want = widths_oracle(k, max_minor)
        applied = sum(w is not None and w[4] == 1 for w in want)
        print(f"k={k} max_minor={max_minor}: {applied} applied")
        assert applied >= 3 and not any(w is not None and w[4] == 2 for w in want)


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _rows(out, idx):
    return {key: v[idx] for key, v in out.items()}


_same_rows = T._same_rows


def _same(a, b, ctx=None):
    _same_rows(a, b, ctx)
    for key in FIRTH_KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, ctx)
    assert a["firth_state"].tolist() == b["firth_state"].tolist(), ctx


def _as_score_row(got, base, ctx=None):
    """`out` is glm_score_sparse's bit for bit, with its firth byte 0."""
    _same_rows(got, base, ctx)
    assert not got["firth"].any(), ctx


@pytest.fixture(scope="module")
def files(gpu_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_sparse_firth")
    return {n: T._File(gpu_lib, tmp, n) for n in PARITY_N}


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", PARITY_N)
def test_parity_with_the_oracle_for_every_form(gpu_lib, files, n, k):
    f = files[n]
    assert np.array_equal(f.geno, inputs(n).geno)
    Z = f.covariates(k)
    zc = Z if k else None
    nul = null_of(n, k)
    results, seen = {}, {}
    for max_minor in max_minors(n):
        sp = f.sparse(max_minor=max_minor)
        got = results[max_minor] = sp.glm_score_sparse_firth(f.y, zc, firth_cutoff=CUTOFF)
        for key in FIRTH_KEYS:
            assert got[key].shape == (f.m,) and got[key].dtype == np.float64
        assert got["firth_state"].shape == (f.m,) and got["firth_state"].dtype == np.uint8
        _as_score_row(got, sp.glm_score_sparse(f.y, zc), ctx=(n, k, max_minor))
        s = seen[max_minor] = FS.check_firth(got, f.x, f.geno, nul, max_minor, CUTOFF, TOL,
                                             want=oracle_case(n, k, max_minor))
        print(f"n={n} k={k} max_minor={max_minor}: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g} "
              f"(TOL {TOL:.3g})")
        assert s["applied"] >= 30
        sp.close()
    assert {0, 1, 2, 3} <= {r[1] for r in seen[n]["rows"] if not r[2]}
    if n == 4099:  # both sides of the wave / workgroup threshold, and dense-form rows
        entries = [r[4] for r in seen[n]["rows"]]
        assert min(entries) <= 1024 < max(entries)
        assert any(r[2] for r in seen[1]["rows"])
    # rows whose E (and so d) is the same under two max_minor values
    for a, b in ((0, 1), (0, n), (1, n)):
        ea = {r[0]: r for r in seen[a]["rows"]}
        both = 0
        for r in seen[b]["rows"]:
            o = ea.get(r[0])
            if o is None:
                continue
            ba, mask_a = FS.e_mask(f.geno[r[0]], o[1], o[2], nul)
            bb, mask_b = FS.e_mask(f.geno[r[0]], r[1], r[2], nul)
            if ba == bb and np.array_equal(mask_a, mask_b):
                ga = [results[a][key][r[0]] for key in FIRTH_KEYS]
                gb = [results[b][key][r[0]] for key in FIRTH_KEYS]
                assert max(FS.scales(*ga, *gb)) <= 2 * TOL, (n, k, a, b, r, ga, gb)
                both += 1
        assert both > 0


@pytest.fixture(scope="module")
def edge_file(gpu_lib, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("glm_score_sparse_firth_edge") / "edge.pgen")
    W.write_pgen(path, edge_rows(), [0] * len(EDGE_ENTRIES))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_the_wave_workgroup_edge(gpu_lib, edge_file, k):
    """1,023 and 1,024 entries are a wave's rows, and 1,024 pairs fill its LDS stash; 1,025 and 1,026 are the
    workgroup's."""
    case = inputs(EDGE_N)
    nul, x, want = edge_oracle(k)
    Z = case.covariates(k) if k else None
    sp = gpu_lib.Dataset.open(edge_file, sparse=True, max_minor=EDGE_N)
    info = sp.sparse_info()
    assert info.dense_variant_ct == 0 and info.sparse_variant_ct == len(EDGE_ENTRIES)
    got = sp.glm_score_sparse_firth(case.y, Z, firth_cutoff=CUTOFF)
    _as_score_row(got, sp.glm_score_sparse(case.y, Z), ctx=k)
    s = FS.check_firth(got, x, edge_rows(), nul, EDGE_N, CUTOFF, TOL_WIDTHS, want=want)
    print(f"k={k}: worst {s['worst']:.3g} (TOL {TOL_WIDTHS:.3g})")
    assert s["applied"] == len(EDGE_ENTRIES) and [r[4] for r in s["rows"]] == list(EDGE_ENTRIES)
    sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_width_feeding_the_kernel(gpu_lib, files, k):
    """The kernel has no width in it: this pins the solve's rows at every width GlmPadCovar returns, at k = KP and one
    above the width below, as what it reads."""
    f = files[WIDTHS_N]
    Z = f.covariates(k)
    for max_minor in (f.n, 0):
        nul, want = widths_oracle(k, max_minor)
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_firth(f.y, Z, firth_cutoff=CUTOFF)
        _as_score_row(got, sp.glm_score_sparse(f.y, Z), ctx=(k, max_minor))
        s = FS.check_firth(got, f.x, f.geno, nul, max_minor, CUTOFF, TOL_WIDTHS, idx=WIDTHS_ROWS, want=want)
        print(f"k={k} max_minor={max_minor}: {s['applied']} applied, worst {s['worst']:.3g} (TOL {TOL_WIDTHS:.3g})")
        assert s["applied"] >= 3
        sp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_against_the_dense_route(gpu_lib, files, n):
    """Base 0, base 3 and dense-form rows have the dense route's E: the same states, the values to rounding."""
    f = files[n]
    k = 1
    Z = f.covariates(k)
    dense = gpu_lib.Dataset.open(f.path)
    ref = dense.glm_score_multi_firth(f.y[None, :], Z, firth_cutoff=CUTOFF)
    dense.close()
    for max_minor in (0, f.n):
        sp = f.sparse(max_minor=max_minor)
        got = sp.glm_score_sparse_firth(f.y, Z, firth_cutoff=CUTOFF)
        sp.close()
        applied = 0
        for i in range(f.m):
            base, dense_form = S.row_form(f.geno[i], max_minor)
            if not (dense_form or base in (0, 3)):
                continue
            ctx = (n, max_minor, i, base, dense_form)
            assert got["firth_state"][i] == ref["firth_state"][i, 0], ctx
            assert got["errcode"][i] == ref["errcode"][i, 0], ctx
            if got["firth_state"][i] == 1:
                a = [got[key][i] for key in FIRTH_KEYS]
                b = [ref[key][i, 0] for key in FIRTH_KEYS]
                assert max(FS.scales(*a, *b)) <= 2 * TOL, (ctx, a, b)
                applied += 1
        print(f"n={n} max_minor={max_minor}: {applied} applied rows with the dense route's E")
        assert applied >= 20


@pytest.mark.gpu
def test_cutoff(gpu_lib, files):
    f = files[257]
    k = 1
    Z = f.covariates(k)
    nul = null_of(257, k)
    sp = f.sparse(max_minor=f.n)
    base = sp.glm_score_sparse(f.y, Z)
    never = sp.glm_score_sparse_firth(f.y, Z, firth_cutoff=math.inf)
    _as_score_row(never, base, ctx="inf")
    assert not never["firth_state"].any()
    for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
        assert np.array_equal(never[key], base[of], equal_nan=True), key
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
    at2 = sp.glm_score_sparse_firth(f.y, Z, firth_cutoff=CUTOFF)
    low = sp.glm_score_sparse_firth(f.y, Z, firth_cutoff=0.1)
    _as_score_row(low, base, ctx=0.1)
    s = FS.check_firth(low, f.x, f.geno, nul, f.n, 0.1, TOL, want=oracle_case(257, k, f.n, 0.1))
    print(f"cutoff 0.1: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g}")
    assert (low["firth_state"] == 1).sum() > (at2["firth_state"] == 1).sum()
    sp.close()


@pytest.mark.gpu
def test_a_row_does_not_depend_on_the_range_or_the_window(gpu_lib, files):
    L = gpu_lib
    f = files[4099]
    Z = f.covariates(3)
    v0 = next(v for v in range(150, M_R) if f.kinds[v] in (2, 3))  # a window that starts after an LD base
    v1 = min(M_R, v0 + 150)
    for max_minor in max_minors(f.n):
        sp = f.sparse(max_minor=max_minor)
        whole = sp.glm_score_sparse_firth(f.y, Z)
        assert (whole["firth_state"] == 1).sum() >= 30
        _same(sp.glm_score_sparse_firth(f.y, Z), whole, ctx="again")
        rc_a, _, out_a, firth_a = _raw(L, sp._h, f.y, Z, CUTOFF, 0, f.m)
        rc_b, _, out_b, firth_b = _raw(L, sp._h, f.y, Z, CUTOFF, 0, f.m)
        assert rc_a == rc_b == L.PGH_OK
        assert out_a.tobytes() == out_b.tobytes() and firth_a.tobytes() == firth_b.tobytes()
        rows = firth_a.view(L.GLM_FIRTH_ROW_DTYPE)
        assert not rows["pad"].any() and rows["state"].tolist() == whole["firth_state"].tolist()
        _same(sp.glm_score_sparse_firth(f.y, Z, v_begin=40, v_end=333), _rows(whole, slice(40, 333)), ctx=max_minor)
        empty = sp.glm_score_sparse_firth(f.y, Z, v_begin=77, v_end=77)
        assert all(empty[key].shape == (0,) for key in FIRTH_KEYS + ("firth_state", "beta"))
        part = f.sparse(max_minor=max_minor, variant_begin=v0, variant_end=v1)
        _same(part.glm_score_sparse_firth(f.y, Z), _rows(whole, slice(v0, v1)), ctx=(max_minor, v0))
        part.close()
        sp.close()


CHUNK = T.CHUNK  # variants per chunk of the GLM family


@pytest.mark.gpu
def test_rows_across_a_chunk_boundary(gpu_lib, tmp_path):
    """test_glm_score_sparse_spa.test_triples_across_a_chunk_boundary's recipe."""
    L = gpu_lib
    m, n = CHUNK + 300, 257
    prefix = str(tmp_path / "chunks")
    L.synth_write_files(prefix, m, n, 5152, 0.02)
    rng = np.random.default_rng(62)
    y = T._pheno(rng, n, case_rate=0.1)
    Z = T._covariates(rng, 2, y)
    for max_minor in (8, n):  # dense-form and sparse rows mixed, and every row sparse
        sp = L.Dataset.open(prefix + ".pgen", sparse=True, max_minor=max_minor)
        info = sp.sparse_info()
        assert info.sparse_variant_ct > 0 and (info.dense_variant_ct > 0) == (max_minor == 8)
        whole = sp.glm_score_sparse_firth(y, Z, v_begin=5)
        _as_score_row(whole, sp.glm_score_sparse(y, Z, v_begin=5), ctx=max_minor)
        applied = np.flatnonzero(whole["firth_state"] == 1)
        assert (applied < CHUNK - 5).any() and (applied >= CHUNK - 5).any()
        assert not (whole["firth_state"] == 2).any()
        for lo, hi in ((5 + CHUNK - 40, 5 + CHUNK + 60), (5, 5 + CHUNK), (5 + CHUNK, m), (m - 30, m)):
            _same(sp.glm_score_sparse_firth(y, Z, v_begin=lo, v_end=hi), _rows(whole, slice(lo - 5, hi - 5)),
                  ctx=(max_minor, lo))
        sp.close()


@pytest.mark.gpu
def test_sample_subset(gpu_lib, files):
    """test_glm_score_sparse_spa.test_sample_subset's subset: a count that is no multiple of 64."""
    f = files[4099]
    rng = np.random.default_rng(13)
    keep = rng.random(f.n) < 0.5
    assert int(keep.sum()) % 64
    y = f.y[keep]
    k = 3
    Z = T._covariates(rng, k, y)
    nul = O.Null(y, Z)
    assert nul.status is None
    idx = list(range(0, M_R, 2))
    for max_minor in max_minors(f.n):
        sp = f.sparse(max_minor=max_minor)
        ss = sp.subset(keep)
        got = sp.glm_score_sparse_firth(y, Z, subset=ss)
        _as_score_row(got, sp.glm_score_sparse(y, Z, subset=ss), ctx=max_minor)
        forms = [S.row_form(f.geno[i], max_minor) for i in range(f.m)]  # the form comes from all raw samples
        s = FS.check_firth(got, f.x[:, keep], f.geno[:, keep], nul, forms, CUTOFF, TOL, idx=idx)
        print(f"subset max_minor={max_minor}: {s['applied']} applied, {s['failed']} failed, worst {s['worst']:.3g}")
        assert s["applied"] >= 10
        ss.close()
        sp.close()


# whole include words, a ragged last word, one sample, a stride that cuts every word, tile edges, nobody
SHAPES = [(SS.N_SMALL, "word_block"), (SS.N_SMALL, "last_word"), (SS.N_SMALL, "first"), (SS.N_SMALL, "all_but_one"),
          (SS.N_SMALL, "stride4"), (SS.N_SMALL, "empty"), (SS.N_WIDE, "tile_edges"), (SS.N_WIDE, "third_tile")]


@pytest.fixture(scope="module")
def rare_worlds(gpu_lib, tmp_path_factory):
    from test_subset_shapes import _Rare

    tmp = tmp_path_factory.mktemp("glm_score_sparse_firth_shapes")
    return functools.lru_cache(maxsize=None)(lambda n: _Rare(gpu_lib, tmp, n))


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", SHAPES, ids=[f"{n}-{name}" for n, name in SHAPES])
def test_structured_subsets(gpu_lib, rare_worlds, n, shape):
    """tests/subset_shapes.py's masks over test_subset_shapes' rare matrix: the refusals or the rows glm_score_sparse
    gives, and against the oracle on the subset's samples where rows are fitted."""
    L = gpu_lib
    r = rare_worlds(n)
    mask = r.masks[shape]
    n_out = int(mask.sum())
    sub, x = r.codes[:, mask], r.x[:, mask]
    z = np.ascontiguousarray(r.z[:, mask])
    y = np.ascontiguousarray(r.y_bin[mask])
    have = ~np.isnan(y)
    one_class = not ((y[have] == 1.0).any() and (y[have] == 0.0).any())
    for mm, sp in r.forms.items():
        ss = r.subset(shape, sp)
        if shape == "empty" or one_class:
            text = "sample subset is empty" if shape == "empty" else "no cases or no controls"
            for call in (sp.glm_score_sparse, sp.glm_score_sparse_firth):
                with pytest.raises(L.PghArgError, match=text):
                    call(y, z, subset=ss)
            continue
        got = sp.glm_score_sparse_firth(y, z, firth_cutoff=CUTOFF, subset=ss)
        _as_score_row(got, sp.glm_score_sparse(y, z, subset=ss), ctx=(n, shape, mm))
        nul = O.Null(y, z)
        forms = [S.row_form(r.codes[i], mm) for i in range(SS.M)]  # the form comes from all raw samples
        s = FS.check_firth(got, x, sub, nul, forms, CUTOFF, TOL)
        print(f"{n} {shape} max_minor={mm} ({n_out} samples): {s['applied']} applied, worst {s['worst']:.3g}")
        if nul.status is not None:
            assert np.isnan(got["p_firth"]).all() and not got["firth_state"].any()
        elif n_out >= 127:
            assert s["applied"] >= 3, (n, shape, mm)


@pytest.mark.gpu
def test_undecided_rows(gpu_lib, tmp_path, files):
    L = gpu_lib
    path, geno, y = T._decision_file(tmp_path)
    Z = geno[5].astype(np.float64)[None, :]
    sp = L.Dataset.open(path, sparse=True, max_minor=geno.shape[1])
    got = sp.glm_score_sparse_firth(y, Z, firth_cutoff=0.1)
    _as_score_row(got, sp.glm_score_sparse(y, Z))
    assert list(got["errcode"]) == ["CONST_ALLELE", "CONST_ALLELE", "CONST_ALLELE", "TOO_FEW_SAMPLES", None,
                                    "SINGULAR_MATRIX", None, "CONST_ALLELE"]
    undecided = got["errcode"] != None  # noqa: E711
    for key in FIRTH_KEYS:
        assert np.isnan(got[key][undecided]).all() and not np.isnan(got[key][~undecided]).any(), key
    assert not got["firth_state"][undecided].any()
    sp.close()
    # a collinear-covariate call: the null status on every row it leaves undecided
    f = files[257]
    z = f.covariates(1)[0]
    sp = f.sparse(max_minor=f.n)
    got = sp.glm_score_sparse_firth(f.y, np.stack([z, z]))
    _as_score_row(got, sp.glm_score_sparse(f.y, np.stack([z, z])))
    assert "SINGULAR_MATRIX" in set(got["errcode"]) and not (got["errcode"] == None).any()  # noqa: E711
    assert all(np.isnan(got[key]).all() for key in FIRTH_KEYS) and not got["firth_state"].any()
    sp.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    dense = L.Dataset.open(path)
    sp = L.Dataset.open(path, sparse=True)
    n = sp.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    rows = sp.glm_score_sparse_firth(y, v_begin=0, v_end=8)
    assert rows["beta_firth"].shape == (8,) and rows["firth_state"].dtype == np.uint8
    y2 = y.copy()
    y2[4] = 2.0
    with pytest.raises(ValueError, match="phenotype must be 0 or 1"):
        sp.glm_score_sparse_firth(y2)
    with pytest.raises(ValueError, match="sparse-resident"):
        dense.glm_score_sparse_firth(y, v_begin=0, v_end=8)
    with pytest.raises(ValueError, match="at most 20 covariates"):
        sp.glm_score_sparse_firth(y, np.zeros((21, n)))
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse_firth(y, v_begin=0, v_end=sp.v_end + 1)
    with pytest.raises(ValueError, match="outside the resident range"):
        sp.glm_score_sparse_firth(y, v_begin=9, v_end=8)
    # the two of its own, and the dataset's form, through the C call: nothing is written
    for text, handle, cutoff, null_firth in (("firth_cutoff must be at least 0.1", sp._h, 0.0999, False),
                                             ("firth_cutoff must be at least 0.1", sp._h, NAN, False),
                                             ("firth_cutoff must be at least 0.1", sp._h, -1.0, False),
                                             ("null firth", sp._h, CUTOFF, True),
                                             ("needs a sparse-resident dataset", dense._h, CUTOFF, False)):
        rc, msg, out, firth = _raw(L, handle, y, None, cutoff, 0, 8, null_firth)
        assert rc == L.PGH_ERR_ARG and text in msg and _untouched(out, firth), (text, rc, msg)
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        sp.glm_score_sparse_firth(y, firth_cutoff=0.05)
    sp.close()
    dense.close()
