"""pgh_glm_score_multi_dosage_spa / Dataset.glm_score_multi_dosage_spa: the saddlepoint p-value of the logistic score
test on the dense route over a dataset that holds dosage tracks.  Against the FP64 oracle (tests/glm_spa_dosage_oracle.py:
b = 2 when sum_N x > n, otherwise 0; E = the samples of N whose value is not exactly b; V_rest = 0 by rule when E = N)
the errcodes and states are equal and p_spa is within TOL in state 1; `out` is pgh_glm_score_multi_dosage's bit for bit;
a variant without a track and a variant whose track restates its calls get pgh_glm_score_multi_spa's triple bit for
bit; and a row's triple does not depend on the other phenotypes, its place among them, the range, the window, the
phenotype block, the variant chunk, the scratch budget or the tracks of its neighbours.

TOL is 100 x the worst relative difference between the numpy model of the kernel's accumulation order
(tools/glm_score_dense_dosage_spa_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is
test_glm_score_sparse_spa's, for device exp / log1p and fma contraction.  The cases at every covariate width and at
the sample-count edges are held to TOL_WIDTHS, the same rule on their own rows: MODEL_WORST_WIDTHS is what
`python tools/glm_score_dense_dosage_spa_model.py --widths` prints."""

import ctypes as C
import functools
import math
import os
import sys
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import dosage_shapes as DS
import glm_score_oracle as O
import glm_spa_dosage_oracle as D
import pgen_writer as W
import subset_shapes as SS
import test_glm_score_multi_dosage as MD
import test_glm_score_multi_spa as MS
import test_glm_score_sparse_spa as SP
from test_dosage_tracks import make_dosage_file

NAN = float("nan")
NAME = "pgh_glm_score_multi_dosage_spa"
NONE = 0xFFFF
CUTOFF = 2.0
MODEL_WORST = 2.24e-12  # printed by tools/glm_score_dense_dosage_spa_model.py
TOL = 100 * MODEL_WORST
# printed by tools/glm_score_dense_dosage_spa_model.py --widths: the width and edge cases below, on the rows they check
MODEL_WORST_WIDTHS = 4.17e-12
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"

# (variants, samples, seed) of test_dosage_tracks.make_dosage_file: the parity files
MIXED = MD.MIXED
PARITY_K = (0, 1, 3)
# every width GlmForWidth instantiates, on every WIDTHS_STRIDE-th row of a file at the count that crosses a step
WIDTHS, WIDTHS_N, WIDTHS_M, WIDTHS_SEED, WIDTHS_STRIDE = SP.WIDTHS, SP.WIDTHS_N, 90, 50, 2
# the u16 row's padding and the mask's tail
EDGE64 = {63: (150, 703), 64: (150, 704), 65: (150, 705)}  # n: (variants, seed)
EDGE64_K = (0, 2)
# one 4,096-sample step of the walk, the first sample of a second step, a third step
STEPS = {4096: (45, 4196), 4097: (60, 4197), 8209: (30, 8309)}
STEPS_K = 3
# the designed rows of dosage_shapes that test_structured_tracks names
STRUCTURED_N = DS.N_TILE
STRUCTURED_K = 3
STRUCTURED_CUTOFF = 1.0
FAILING_SAMPLES = SP.FAILING_ROW[257][0]
FAILING_VALUES = [32000, 40, 7, 300, 90, 5]
FAILING_AT = 2  # the state-2 variant's place in its file


# ---- inputs ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def phenotypes(n):
    """y0 with 20 % cases, a 4 % phenotype (8 / n at the smallest sample counts, so that it has cases), a 30 %
    phenotype with a tenth of it NaN."""
    rng = np.random.default_rng(9000 + n)
    y0 = (rng.random(n) < 0.2).astype(np.float64)
    rare = (rng.random(n) < max(0.04, 8.0 / n)).astype(np.float64)
    common = (rng.random(n) < 0.3).astype(np.float64)
    common[rng.random(n) < 0.1] = NAN
    return np.stack([y0, rare, common])


@functools.lru_cache(maxsize=None)
def covariates(n, k):
    return np.random.default_rng(100 * n + k).normal(size=(k, n))


class Inputs:
    """The calls, the dosages (0xFFFF = none), the track kinds and the value rows of one file."""

    def __init__(self, geno, dos, dkinds):
        self.geno, self.dos, self.dkinds = geno, dos, list(dkinds)
        self.m, self.n = geno.shape
        self.x = DS.values(geno, dos)
        self.track = np.array([kind != 0 for kind in dkinds])
        self.full = self.track & (dos != NONE).all(axis=1)
        self.partial = self.track & ~self.full


@functools.lru_cache(maxsize=None)
def made(m, n, seed, enrich="parity", rate=0.35):
    """make_dosage_file's recipe, enriched among a phenotype's cases with probability `rate`: an explicit dosage gains
    9000, otherwise a hom-ref call becomes het.
    enrich = "parity": every third variant among y0's cases; of these every other one has its gain capped at 32768 and
    the others gain only where 9000 fits below it.  (The cap alone puts values exactly on b = 2, so that at n >= 1003,
    where enrichment decides b, no applied full track had E = N; and the 4 % and 30 % phenotypes had fewer than two
    applied rows by chance alone.)  So variant v with v % 9 == 1 is enriched among the 4 % phenotype's cases and with
    v % 9 == 2 among the 30 % phenotype's, capped.
    enrich = "each": variant v among the cases of phenotype v % 3, capped on every other one of a phenotype's variants
    (the width and edge files, where every phenotype needs applied rows on a few variants)."""
    with tempfile.TemporaryDirectory() as tmp:
        geno, dos, dkinds, _ = make_dosage_file(os.path.join(tmp, "recipe.pgen"), m, n, seed, False)
    Y = phenotypes(n)
    rng = np.random.default_rng(7000 + n)
    for v in range(m):
        capped = True
        if enrich == "each":
            y, capped = Y[v % 3], (v // 3) % 2 == 0
        elif v % 3 == 0:
            y, capped = Y[0], (v // 3) % 2 == 0
        elif v % 9 in (1, 2):
            y = Y[v % 9]
        else:
            continue
        hit = (y == 1.0) & (rng.random(n) < rate)
        has = hit & (dos[v] != NONE) & (capped | (dos[v] <= 32768 - 9000))
        dos[v, has] = np.minimum(dos[v, has].astype(np.int64) + 9000, 32768).astype(np.uint16)
        up = hit & (dos[v] == NONE) & (geno[v] == 0)
        geno[v, up] = 1
    return Inputs(geno, dos, dkinds)


def parity_inputs(n):
    m, _, seed = next(c for c in MIXED if c[1] == n)
    return made(m, n, seed)


# the enrichment rates of the "each" files: strong where a phenotype has a handful of cases, weak at the large counts,
# where 0.35 gives |stat| near 50 and a p that underflows
RATE_SMALL, RATE_LARGE = 0.6, 0.08


def widths_inputs():
    return made(WIDTHS_M, WIDTHS_N, WIDTHS_SEED, "each", RATE_LARGE)


def edge_inputs(n):
    m, seed = EDGE64[n] if n in EDGE64 else STEPS[n]
    return made(m, n, seed, "each", RATE_SMALL if n in EDGE64 else RATE_LARGE)


@functools.lru_cache(maxsize=None)
def oracle_case(inp, k, stride=1, cutoff=CUTOFF):
    """The oracle's columns of the three phenotypes over every stride-th row of `inp` (computed once)."""
    Z = covariates(inp.n, k)
    return [D.oracle_column(inp.x, y, Z, cutoff, idx=range(0, inp.m, stride)) for y in phenotypes(inp.n)]


def applied_rows(col):
    return [(i, w) for i, w in enumerate(col) if w is not None and w[2] == 1]


def failing_inputs():
    """The state-2 row in a small file of its own: ParityInputs(257)'s first rows as track-less neighbours, and at
    FAILING_AT a variant whose calls are all missing and whose track holds six values."""
    case = MS.inputs(257)
    geno = case.geno[:5].copy()
    dos = np.full(geno.shape, NONE, dtype=np.uint16)
    geno[FAILING_AT] = 3
    dos[FAILING_AT, FAILING_SAMPLES] = FAILING_VALUES
    dkinds = [0] * len(geno)
    dkinds[FAILING_AT] = 0x20
    return Inputs(geno, dos, dkinds), case.y, case.covariates(1)


@functools.lru_cache(maxsize=None)
def structured_inputs():
    """(layout, value rows, Z, y): dosage_shapes' file of one tile with STRUCTURED_K covariates and y0."""
    lay = DS.Layout(STRUCTURED_N)
    return lay, DS.values(lay.hard, lay.dos), covariates(STRUCTURED_N, STRUCTURED_K), phenotypes(STRUCTURED_N)[0]


def distinct_rows(x):
    """(rows, of): the distinct value rows and, per variant, which of them it holds (test_dosage_shapes._distinct_rows)."""
    seen, rows, of = {}, [], []
    for v in range(len(x)):
        key = x[v].tobytes()
        if key not in seen:
            seen[key] = len(rows)
            rows.append(v)
        of.append(seen[key])
    return rows, np.array(of)


@functools.lru_cache(maxsize=None)
def structured_oracle():
    """The oracle's row per distinct value row of the structured file, spread to every variant that holds it."""
    lay, x, Z, y = structured_inputs()
    rows, of = distinct_rows(x)
    col = D.oracle_column(x, y, Z, STRUCTURED_CUTOFF, idx=rows)
    return [col[rows[j]] for j in of]


STRUCTURED_NAMED = ("word16", "word17", "E512_tile0_ref", "E513_tile0_ref", "E512_spread_common", "E513_spread_common",
                    "E%d_tile0_ref" % DS.cut_counts(STRUCTURED_N)[0], "E%d_tile0_ref" % DS.cut_counts(STRUCTURED_N)[1],
                    "E%d_tile0_ref" % (STRUCTURED_N - 1), "all_on_missing")


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_symbol(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    assert f"{NAME}(" in header
    assert NAME in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.raw(), NAME)
    assert hasattr(lib.Dataset, "glm_score_multi_dosage_spa")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_arrays_of_the_wrong_shape_are_rejected(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi_dosage_spa(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi_dosage_spa(fake, np.zeros((2, 5)), np.zeros((2, 4)))


def _raw(L, h, phen, cutoff=CUTOFF, null=None, v0=0, v1=4, z=None, subset=None):
    """(rc, message, the three outputs untouched) of a raw call over [v0, v1) with the outputs filled beforehand."""
    phen = np.ascontiguousarray(phen, dtype=np.float64)
    out, p_spa, state = MS._fill(max(1, v1 - v0) * len(phen), L.GLM_ROW_DTYPE.itemsize)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = getattr(L.raw(), NAME)(h, subset, v0, v1, len(phen), p(phen), 0 if z is None else len(z), p(z),
                                C.c_double(cutoff), p(out), None if null == "p_spa" else p(p_spa),
                                None if null == "spa_state" else p(state), eb)
    return rc, eb.value.decode(), MS._untouched(out, p_spa, state)


@pytest.mark.parametrize("what,kw", [("a NULL dataset", {}), ("spa_cutoff must be at least 0.1", dict(cutoff=0.05)),
                                     ("spa_cutoff must be at least 0.1", dict(cutoff=NAN)),
                                     ("null p_spa or spa_state", dict(null="p_spa")),
                                     ("null p_spa or spa_state", dict(null="spa_state"))])
def test_bad_arguments_are_refused_with_the_outputs_untouched(lib, what, kw):
    rc, msg, untouched = _raw(lib, None, np.array([[0.0, 1.0]]), **kw)
    assert rc == lib.PGH_ERR_ARG and msg and untouched, (what, rc, msg, untouched)
    if kw:
        assert what in msg, (what, msg)


def _summary(inp, cols):
    """What the applied rows of the three phenotypes' oracle columns cover."""
    per = [applied_rows(col) for col in cols]
    rows = [(i, w) for a in per for i, w in a]
    return dict(per=[len(a) for a in per], applied=len(rows), full=sum(inp.full[i] for i, _ in rows),
                partial=sum(inp.partial[i] for i, _ in rows), hard=sum(not inp.track[i] for i, _ in rows),
                b2=sum(w[3] == 2 for _, w in rows), whole=sum(bool(w[5]) for _, w in rows),
                failed=sum(w is not None and w[2] == 2 for col in cols for w in col))


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_the_parity_inputs_reach_every_case_of_the_dosage_rule(n, k):
    """Conditions on the inputs, not on the device, so that no case can pass on rows that are left alone: the oracle
    decides every row (it asserts where the contract does not), and over the three phenotypes together the applied
    rows cover full and partial tracks, track-less variants, b = 2 and E = N."""
    inp = parity_inputs(n)
    s = _summary(inp, oracle_case(inp, k))
    print(f"n={n} k={k}: {s}")
    assert s["applied"] >= 20 and s["full"] >= 2 and s["partial"] >= 7 and s["hard"] >= 1, (n, k, s)
    assert s["b2"] >= 1 and s["whole"] >= 1 and min(s["per"]) >= 2, (n, k, s)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_at_every_width(k):
    inp = widths_inputs()
    s = _summary(inp, oracle_case(inp, k, WIDTHS_STRIDE))
    print(f"k={k}: {s}")
    assert min(s["per"]) >= 3 and s["whole"] >= 1, (k, s)


@pytest.mark.parametrize("n,k", [(n, k) for n in EDGE64 for k in EDGE64_K] + [(n, STEPS_K) for n in STEPS])
def test_the_edge_inputs_have_applied_rows(n, k):
    inp = edge_inputs(n)
    cols = oracle_case(inp, k)
    s = _summary(inp, cols)
    print(f"n={n} k={k}: {s}")
    assert min(s["per"]) >= 3, (n, k, s)
    if n == 4097:  # an entry in the first word of the walk's second step
        Y = phenotypes(n)
        assert any(not np.isnan(Y[p][4096]) and inp.x[i, 4096] not in (-9.0, float(w[3]))
                   for p, col in enumerate(cols) for i, w in applied_rows(col)), s


def test_the_state_2_row_is_one():
    inp, y, Z = failing_inputs()
    col = D.oracle_column(inp.x, y, Z, CUTOFF)
    row, p_spa, state, b, n_e, whole = col[FAILING_AT]
    print(f"the state-2 row: stat {row['stat']:.3g}, b = {b}, {n_e} entries, E = N: {whole}")
    assert row["errcode"] is None and abs(row["stat"]) > 3 and state == 2 and whole and n_e == 6
    assert all(w[2] != 2 for i, w in enumerate(col) if i != FAILING_AT)


def test_the_structured_inputs_are_decided_and_hold_the_named_rows():
    lay = structured_inputs()[0]
    col = structured_oracle()
    for name in STRUCTURED_NAMED:
        assert lay.variants(name), name
    for name in ("restated_sparse", "restated_gaps", "restated_full"):
        assert len(lay.variants(name)) == 4, name
    applied = applied_rows(col)
    whole = sum(bool(w[5]) for _, w in applied)
    print(f"structured tracks: {len(applied)} applied of {lay.m}, {whole} with E = N, "
          f"{sum(w[2] == 2 for w in col)} failed")
    assert len(applied) >= lay.m // 8 and whole >= 3


def test_the_model_agrees_with_the_oracle_within_the_printed_constants():
    """The smallest parity file at every k and one width case: the whole runs are the tool's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import glm_score_dense_dosage_spa_model as M
    finally:
        sys.path.pop(0)
    inp = parity_inputs(257)
    worst = max(M.run_case(inp, k, 1, quiet=True)[0] for k in PARITY_K)
    assert 0 < worst <= MODEL_WORST, worst
    worst = M.run_case(edge_inputs(65), 2, 1, quiet=True)[0]
    assert 0 < worst <= MODEL_WORST_WIDTHS, worst


# ---- on the GPU --------------------------------------------------------------------------------------------------

_col, _rows, _same, _same_rows = MS._col, MS._rows, MS._same, MS._same_rows


class _File:
    def __init__(self, tmp, name, inp, seed=0):
        self.inp = inp
        self.path = str(tmp / f"{name}.pgen")
        self.kinds = W.choose_kinds(inp.geno, np.random.default_rng(seed))
        W.write_pgen(self.path, inp.geno, self.kinds, dosage=inp.dos, dosage_kinds=inp.dkinds)
        self.hard_path = str(tmp / f"{name}_hard.pgen")
        self.ds = None

    def open(self, L):
        if self.ds is None:
            self.ds = L.Dataset.open(self.path)
        return self.ds

    def hard(self, L):
        """The same calls in a file without tracks, opened."""
        if not os.path.exists(self.hard_path):
            W.write_pgen(self.hard_path, self.inp.geno, self.kinds)
        return L.Dataset.open(self.hard_path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_dosage_spa")
    made_files = {}

    def get(name, inp):
        if name not in made_files:
            made_files[name] = _File(tmp, name, inp)
        return made_files[name]

    yield get
    for f in made_files.values():
        if f.ds is not None:
            f.ds.close()


def _check(got, cols, tol, ctx):
    """Every column against the oracle's; returns the applied rows per phenotype."""
    counts = []
    for p, col in enumerate(cols):
        applied, worst = D.check_column(got, p, col, tol, ctx=ctx)
        print(f"{ctx} phenotype {p}: {applied} applied, worst {worst:.3g} (tolerance {tol:.3g})")
        assert applied == len(applied_rows(col)), (ctx, p)
        counts.append(applied)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_parity_with_the_oracle(gpu_lib, files, n, k):
    inp = parity_inputs(n)
    ds = files(f"mixed_{n}", inp).open(gpu_lib)
    Y = phenotypes(n)
    zc = covariates(n, k) if k else None
    got = ds.glm_score_multi_dosage_spa(Y, zc, spa_cutoff=CUTOFF)
    assert got["p_spa"].shape == (inp.m, len(Y)) and got["spa_state"].shape == (inp.m, len(Y))
    assert got["p_spa"].dtype == np.float64 and got["spa_state"].dtype == np.uint8
    _same_rows(got, ds.glm_score_multi_dosage(Y, zc), ctx=(n, k))
    counts = _check(got, oracle_case(inp, k), TOL, f"n={n} k={k}")
    assert sum(counts) >= 20 and min(counts) >= 2


@pytest.mark.gpu
def test_the_state_2_row(gpu_lib, files):
    inp, y, Z = failing_inputs()
    ds = files("failing", inp).open(gpu_lib)
    got = ds.glm_score_multi_dosage_spa(y[None, :], Z, spa_cutoff=CUTOFF)
    D.check_column(got, 0, D.oracle_column(inp.x, y, Z, CUTOFF), TOL, ctx="failing")
    assert got["spa_state"][FAILING_AT, 0] == 2 and got["errcode"][FAILING_AT, 0] is None
    assert got["p_spa"][FAILING_AT, 0] == got["p"][FAILING_AT, 0]


@pytest.mark.gpu
def test_bit_for_bit_against_the_hardcall_route(gpu_lib, files, tmp_path):
    L = gpu_lib
    n, k = 1003, 3
    Y, Z = phenotypes(n), covariates(n, k)
    # (a) the track-less variants of a mixed file
    inp = parity_inputs(n)
    f = files(f"mixed_{n}", inp)
    got = f.open(L).glm_score_multi_dosage_spa(Y, Z, spa_cutoff=CUTOFF)
    hard = f.hard(L)
    want = hard.glm_score_multi_spa(Y, Z, spa_cutoff=CUTOFF)
    assert (~inp.track).sum() >= 10 and (want["spa_state"][~inp.track] == 1).any()
    _same(_rows(got, ~inp.track), _rows(want, ~inp.track), ctx="track-less variants")
    changed = ~np.array([np.array_equal(got["p_spa"][v], want["p_spa"][v], equal_nan=True) for v in range(inp.m)])
    assert changed[inp.track].any() and not changed[~inp.track].any()
    # (b) a file with no track at all through the new entry
    _same(hard.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=CUTOFF), want, ctx="no tracks")
    hard.close()
    # (c) tracks of each encoding that restate their calls (test_glm_score_multi_dosage._restated_case)
    case, hard_path = MD._restated_case(tmp_path, n)
    assert case.track.sum() > 60 and {0x20, 0x40, 0x60} <= set(case.dkinds)
    hard = L.Dataset.open(hard_path)
    want = hard.glm_score_multi_spa(Y, Z, spa_cutoff=1.0)
    hard.close()
    assert (want["spa_state"][case.track] == 1).sum() >= 20
    ds = L.Dataset.open(case.path)
    _same(ds.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=1.0), want, ctx="restated")
    ds.close()
    # (d) dosage_shapes' restated rows (sparse, with gaps, full) and its track-less variants
    lay, x, Zs, y = structured_inputs()
    f = files("structured", Inputs(lay.hard, lay.dos, lay.kinds.tolist()))
    got = f.open(L).glm_score_multi_dosage_spa(y[None, :], Zs, spa_cutoff=STRUCTURED_CUTOFF)
    hard = f.hard(L)
    want = hard.glm_score_multi_spa(y[None, :], Zs, spa_cutoff=STRUCTURED_CUTOFF)
    hard.close()
    calls = np.array([not lay.kinds[v] or lay.names[v].startswith("restated_") for v in range(lay.m)])
    for name in ("restated_sparse", "restated_gaps", "restated_full"):
        vs = lay.variants(name)
        assert calls[vs].all() and all(code is None for code in want["errcode"][vs, 0]), name
    assert (want["spa_state"][calls, 0] == 1).sum() >= 5  # (the oracle applies 8 of these 86 rows)
    _same(_rows(got, calls), _rows(want, calls), ctx="dosage_shapes")


@pytest.fixture(scope="module")
def case_1003(gpu_lib, files):
    """n = 1003, k = 3: the inputs and the whole-range result that the independence tests share."""
    inp = parity_inputs(1003)
    f = files("mixed_1003", inp)
    Y, Z = phenotypes(1003), covariates(1003, 3)
    whole = f.open(gpu_lib).glm_score_multi_dosage_spa(Y, Z, spa_cutoff=CUTOFF)
    assert all((whole["spa_state"][:, p] == 1).sum() >= 2 for p in range(len(Y)))
    return types.SimpleNamespace(inp=inp, f=f, ds=f.ds, Y=Y, Z=Z, whole=whole)


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_other_phenotypes_or_its_place(gpu_lib, case_1003):
    c = case_1003
    _same(c.ds.glm_score_multi_dosage_spa(c.Y, c.Z, spa_cutoff=CUTOFF), c.whole, ctx="again")
    for p in range(len(c.Y)):
        _same(_col(c.ds.glm_score_multi_dosage_spa(c.Y[p:p + 1], c.Z, spa_cutoff=CUTOFF), 0), _col(c.whole, p),
              ctx=("alone", p))
    moved = c.ds.glm_score_multi_dosage_spa(c.Y[::-1], c.Z, spa_cutoff=CUTOFF)
    for p in range(len(c.Y)):
        _same(_col(moved, len(c.Y) - 1 - p), _col(c.whole, p), ctx=("reversed", p))


@pytest.mark.gpu
@pytest.mark.parametrize("k,what", MD.LAYOUTS)
def test_phenotypes_at_and_across_the_column_blocks(gpu_lib, case_1003, k, what):
    """17 phenotypes: the three in turn at positions 0..15 and one of its own at 16.  k = 14: the k + 2 x-columns of a
    phenotype are one 16-column block; k = 13: every phenotype after the first straddles a block edge."""
    c = case_1003
    Z = covariates(1003, k)
    own = O.pheno(np.random.default_rng(17_000 + k), 1003, Z, case_rate=0.25, missing=0.05)
    Y17 = np.stack([c.Y[i % 3] for i in range(MD.LAYOUT_PHENOTYPES - 1)] + [own])
    three = c.ds.glm_score_multi_dosage_spa(c.Y, Z, spa_cutoff=CUTOFF)
    got = c.ds.glm_score_multi_dosage_spa(Y17, Z, spa_cutoff=CUTOFF)
    assert (three["spa_state"] == 1).sum() >= 10
    for p in range(MD.LAYOUT_PHENOTYPES - 1):
        _same(_col(got, p), _col(three, p % 3), ctx=(k, p))
    _same(_col(got, 16), _col(c.ds.glm_score_multi_dosage_spa(own[None, :], Z, spa_cutoff=CUTOFF), 0), ctx=(k, 16))


@pytest.mark.gpu
def test_a_triple_does_not_depend_on_the_range_the_window_or_the_scratch_budget(gpu_lib, case_1003):
    L = gpu_lib
    c = case_1003
    run = lambda ds, **kw: ds.glm_score_multi_dosage_spa(c.Y, c.Z, spa_cutoff=CUTOFF, **kw)
    _same(run(c.ds, v_begin=37), _rows(c.whole, slice(37, None)), ctx="v_begin = 37")
    part = L.Dataset.open(c.f.path, variant_begin=37, variant_end=c.inp.m)
    _same(run(part), _rows(c.whole, slice(37, c.inp.m)), ctx="window")
    _same(run(part, v_begin=41, v_end=63), _rows(c.whole, slice(41, 63)), ctx="window range")
    part.close()
    # The scratch budget.  At n = 1003 the smallest column block is 1024 sample rows x 64 columns x 8 bytes = 524,288
    # bytes and a phenotype's mask 256 bytes: a budget of which three quarters are less leaves one phenotype per block,
    # so the three run as three blocks.  What the block leaves goes to one workgroup's stash first (16 bytes x 1003
    # samples = 16,048; never less than one) and then bounds the chunk: per variant and phenotype 244 bytes of sums,
    # entries, count and row (k = 3) and 65 of [t, U, V], p_spa and the state, plus the expanded rows' 144 bytes per 64
    # samples and 4 bytes of list: 2,617 bytes.  1 byte: chunks of one variant; block + stash + 7 x 2,617: of seven.
    per_variant = 244 + 65 + 144 * 16 + 4
    lo, hi = 5, 75
    before = os.environ.get(SCRATCH_ENV)
    for budget, chunk in ((1, 1), (524_544 + 16_048 + 7 * per_variant, 7)):
        assert budget // 4 * 3 < 524_544 and max(1, (budget - 524_544 - 16_048) // per_variant) == chunk
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(SCRATCH_ENV, str(budget))
            _same(run(c.ds, v_begin=lo, v_end=hi), _rows(c.whole, slice(lo, hi)), ctx=budget)
    assert os.environ.get(SCRATCH_ENV) == before


@pytest.mark.gpu
def test_a_sample_subset_that_cuts_the_words(gpu_lib, case_1003):
    """Against the oracle on the subset's samples."""
    c = case_1003
    mask = SS.shapes(c.inp.n)[MS.SUBSET_SHAPE]
    assert mask[:16].sum() not in (0, 16)
    Z, Y = np.ascontiguousarray(c.Z[:, mask]), np.ascontiguousarray(c.Y[:, mask])
    x = c.inp.x[:, mask]
    ss = c.ds.subset(mask)
    got = c.ds.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=CUTOFF, subset=ss)
    _same_rows(got, c.ds.glm_score_multi_dosage(Y, Z, subset=ss), ctx=MS.SUBSET_SHAPE)
    total = 0
    for p, y in enumerate(Y):
        applied, worst = D.check_column(got, p, D.oracle_column(x, y, Z, CUTOFF), TOL, ctx=(MS.SUBSET_SHAPE, p))
        print(f"{MS.SUBSET_SHAPE} ({int(mask.sum())} samples) phenotype {p}: {applied} applied, worst {worst:.3g}")
        total += applied
    assert total >= 5
    ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """GlmScoreDenseDosageSpaKernel<KP> for every width GlmPadCovar returns, at k = KP and one above the width below."""
    inp = widths_inputs()
    ds = files("widths", inp).open(gpu_lib)
    Y, Z = phenotypes(inp.n), covariates(inp.n, k)
    got = ds.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=CUTOFF)
    _same_rows(got, ds.glm_score_multi_dosage(Y, Z), ctx=k)
    assert min(_check(got, oracle_case(inp, k, WIDTHS_STRIDE), TOL_WIDTHS, f"k={k}")) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(n, k) for n in EDGE64 for k in EDGE64_K] + [(n, STEPS_K) for n in STEPS])
def test_sample_count_edges(gpu_lib, files, n, k):
    """n = 63, 64, 65: the u16 row's padding and the mask's tail.  n = 4096: exactly one 4,096-sample step of the walk;
    4097: the first sample of a second step; 8209: a third step."""
    inp = edge_inputs(n)
    ds = files(f"edge_{n}", inp).open(gpu_lib)
    Y = phenotypes(n)
    zc = covariates(n, k) if k else None
    got = ds.glm_score_multi_dosage_spa(Y, zc, spa_cutoff=CUTOFF)
    _same_rows(got, ds.glm_score_multi_dosage(Y, zc), ctx=(n, k))
    assert min(_check(got, oracle_case(inp, k), TOL_WIDTHS, f"n={n} k={k}")) >= 3


@pytest.mark.gpu
def test_structured_tracks(gpu_lib, files):
    """dosage_shapes' file of one tile, one phenotype at cutoff 1.0, every row against the oracle; the encodings of a
    row agree bit for bit."""
    lay, x, Z, y = structured_inputs()
    ds = files("structured", Inputs(lay.hard, lay.dos, lay.kinds.tolist())).open(gpu_lib)
    got = ds.glm_score_multi_dosage_spa(y[None, :], Z, spa_cutoff=STRUCTURED_CUTOFF)
    col = structured_oracle()
    applied, worst = D.check_column(got, 0, col, TOL_WIDTHS, ctx="structured")
    print(f"structured tracks: {applied} applied of {lay.m}, worst {worst:.3g} (tolerance {TOL_WIDTHS:.3g})")
    assert applied == len(applied_rows(col))
    for name in STRUCTURED_NAMED:
        for v in lay.variants(name):
            print(f"  {name} ({hex(int(lay.kinds[v]))}): state {got['spa_state'][v, 0]}, p_spa {got['p_spa'][v, 0]:.6g}, "
                  f"p {got['p'][v, 0]:.6g}")
            assert got["spa_state"][v, 0] == col[v][2], (name, v)
    rows, of = distinct_rows(x)
    first = np.array(rows)[of]
    _same(_rows(got, slice(None)), _rows(got, first), ctx="the encodings of a row")


@pytest.mark.gpu
def test_refusals_and_trivia(gpu_lib, files):
    L = gpu_lib
    path = data_path("rare_small.pgen")
    sp = L.Dataset.open(path, sparse=True)
    group = L.Dataset.open_sharded(path, [0, 0])
    n = sp.n_samples
    y = (np.arange(n) % 3 == 0).astype(np.float64)
    Y = np.stack([y, 1.0 - y])
    for text, ds in (("needs a dense-resident dataset", sp), ("one device's dataset", group)):
        rc, msg, untouched = _raw(L, ds._h, Y)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, rc, msg, untouched)
    sp.close()
    group.close()
    inp = parity_inputs(257)
    ds = files("mixed_257", inp).open(L)
    Y, Z = phenotypes(257), covariates(257, 1)
    bad = Y.copy()
    bad[1, 4] = 2.0
    one = Y.copy()
    one[1] = np.where(np.isnan(Y[2]), NAN, 1.0)
    for text, phen in (("phenotype must be 0 or 1", bad), ("no cases or no controls", one)):
        rc, msg, untouched = _raw(L, ds._h, phen)
        assert rc == L.PGH_ERR_ARG and text in msg and "(phenotype 1)" in msg and untouched, (text, rc, msg)
    with pytest.raises(ValueError, match="spa_cutoff must be at least 0.1"):
        ds.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=0.05)
    # an empty range
    rc, msg, untouched = _raw(L, ds._h, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched, msg
    empty = ds.glm_score_multi_dosage_spa(Y, Z, v_begin=77, v_end=77)
    assert empty["p_spa"].shape == (0, len(Y)) and empty["spa_state"].shape == (0, len(Y))
    # a cutoff of +infinity never applies the saddlepoint
    base = ds.glm_score_multi_dosage(Y, Z)
    never = ds.glm_score_multi_dosage_spa(Y, Z, spa_cutoff=math.inf)
    _same_rows(never, base, ctx="inf")
    assert not never["spa_state"].any()
    assert np.array_equal(never["p_spa"], base["p"], equal_nan=True)
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
