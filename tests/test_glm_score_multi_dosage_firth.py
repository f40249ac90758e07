"""pgh_glm_score_multi_dosage_firth / Dataset.glm_score_multi_dosage_firth: the approximate Firth estimate of the dense
route's rows over a dataset that holds dosage tracks.  Against the FP64 oracle (tests/glm_firth_dosage_oracle.py: E =
the samples of N whose value is not exactly 0, no base code) the errcodes and states are equal, the rows that are not
applied carry NaN or `out`'s beta, se and p bit for bit, and the applied rows are within TOL on |delta beta| / se,
|delta se| / se and |delta p| / p; `out` is pgh_glm_score_multi_dosage's bit for bit with its firth byte 0; a variant
without a track and a variant whose track restates its calls get pgh_glm_score_multi_firth's pair bit for bit; and a
row's pair does not depend on the other phenotypes, its place among them, the range, the window, the phenotype block,
the variant chunk, the scratch budget or the tracks of its neighbours.

The inputs are test_glm_score_multi_dosage_spa's, imported: the three mixed files, the width file, the six edge files,
the phenotypes and the covariates, at cutoff 2.0.

TOL is 100 x the worst difference between the numpy model of the kernel's accumulation order
(tools/glm_score_dense_dosage_firth_model.py) and the oracle on the parity inputs, MODEL_WORST below: the factor is
test_glm_score_sparse_spa's, for device exp / expm1 / log1p and fma contraction.  The cases at every covariate width, at
the sample-count edges and on the structured tracks are held to TOL_WIDTHS, the same rule on their own rows:
MODEL_WORST_WIDTHS is what `python tools/glm_score_dense_dosage_firth_model.py --widths` prints.  The device's observed
worst stands beside each constant."""

import ctypes as C
import functools
import math
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, data_path

import glm_firth_dosage_oracle as D
import glm_score_oracle as O
import subset_shapes as SS
import test_glm_score_multi_dosage as MD
import test_glm_score_multi_dosage_spa as DSPA
import test_glm_score_multi_firth as MF
import test_glm_score_sparse_spa as SP
from test_glm_score_multi_dosage_spa import (Inputs, covariates, distinct_rows, edge_inputs, parity_inputs, phenotypes,
                                             structured_inputs, widths_inputs)

NAN = float("nan")
NAME = "pgh_glm_score_multi_dosage_firth"
CUTOFF = 2.0
# printed by tools/glm_score_dense_dosage_firth_model.py; on an MI355X the parity cases print 9.2e-13 at most
MODEL_WORST = 1.23e-12
TOL = 100 * MODEL_WORST
# printed by tools/glm_score_dense_dosage_firth_model.py --widths: the width, edge and structured cases below, on the
# rows they check; on an MI355X those cases print 1.72e-13 at most
MODEL_WORST_WIDTHS = 1.71e-13
TOL_WIDTHS = 100 * MODEL_WORST_WIDTHS
SCRATCH_ENV = "PGH_GLM_SCORE_SCRATCH_BYTES"
SUBSET_SHAPE = "stride4"  # every 16-sample word of the row is cut: four of its samples are kept

MIXED, PARITY_K = DSPA.MIXED, DSPA.PARITY_K
WIDTHS, WIDTHS_STRIDE = SP.WIDTHS, DSPA.WIDTHS_STRIDE
EDGE64, EDGE64_K, STEPS, STEPS_K = DSPA.EDGE64, DSPA.EDGE64_K, DSPA.STEPS, DSPA.STEPS_K
STRUCTURED_K, STRUCTURED_CUTOFF, STRUCTURED_NAMED = DSPA.STRUCTURED_K, DSPA.STRUCTURED_CUTOFF, DSPA.STRUCTURED_NAMED
FIRTH_KEYS = D.FIRTH_KEYS
# what the oracle gives at every (n, k) of the parity grid, over the three phenotypes together
PARITY_MIN = dict(applied=25, full=4, partial=15, hard=5, whole=4, separated=2, per=3)
PARITY_MAX_EVALS = 15


# ---- the oracle on the imported inputs ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_case(inp, k, stride=1, cutoff=CUTOFF):
    """The oracle's columns of the three phenotypes over every stride-th row of `inp` (computed once)."""
    Z = covariates(inp.n, k)
    return [D.oracle_column(inp.x, y, Z, cutoff, idx=range(0, inp.m, stride)) for y in phenotypes(inp.n)]


def applied_rows(col):
    return [(i, w) for i, w in enumerate(col) if w is not None and w[4] == 1]


@functools.lru_cache(maxsize=None)
def structured_oracle():
    """The oracle's row per distinct value row of the structured file, spread to every variant that holds it."""
    lay, x, Z, y = structured_inputs()
    rows, of = distinct_rows(x)
    col = D.oracle_column(x, y, Z, STRUCTURED_CUTOFF, idx=rows)
    return [col[rows[j]] for j in of]


def _summary(inp, cols):
    """What the applied rows of the three phenotypes' oracle columns cover."""
    per = [applied_rows(col) for col in cols]
    rows = [(i, w) for a in per for i, w in a]
    return dict(per=min(len(a) for a in per), applied=len(rows), full=int(sum(inp.full[i] for i, _ in rows)),
                partial=int(sum(inp.partial[i] for i, _ in rows)), hard=int(sum(not inp.track[i] for i, _ in rows)),
                whole=sum(bool(w[5]["whole"]) for _, w in rows), separated=sum(w[5]["separated"] for _, w in rows),
                evals=max((w[5]["evals"] for _, w in rows), default=0),
                failed=sum(w is not None and w[4] == 2 for col in cols for w in col))


# ---- no device ---------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_symbol(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    assert f"{NAME}(" in header
    assert NAME in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.raw(), NAME)
    assert hasattr(lib.Dataset, "glm_score_multi_dosage_firth")


@pytest.mark.parametrize("shape", [(5,), (0, 5), (2, 4), (2, 3, 5)])
def test_arrays_of_the_wrong_shape_are_rejected(lib, shape):
    """The shape checks run before the library is called: the stand-in dataset has no handle to call with."""
    fake = types.SimpleNamespace(v_begin=0, v_end=10, n_samples=5, _h=None)
    with pytest.raises(ValueError, match="phenotypes"):
        lib.Dataset.glm_score_multi_dosage_firth(fake, np.zeros(shape))
    with pytest.raises(ValueError, match="covariates"):
        lib.Dataset.glm_score_multi_dosage_firth(fake, np.zeros((2, 5)), np.zeros((2, 4)))
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        lib.Dataset.glm_score_multi_dosage_firth(fake, np.zeros((2, 5)), firth_cutoff=0.05)


def _raw(L, h, phen, cutoff=CUTOFF, null_firth=False, v0=0, v1=4, z=None, subset=None):
    """(rc, message, the two outputs untouched) of a raw call over [v0, v1) with the outputs filled beforehand."""
    phen = np.ascontiguousarray(phen, dtype=np.float64)
    out, firth = MF._fill(L, max(1, v1 - v0) * len(phen))
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = getattr(L.raw(), NAME)(h, subset, v0, v1, len(phen), p(phen), 0 if z is None else len(z), p(z),
                                C.c_double(cutoff), p(out), None if null_firth else p(firth), eb)
    return rc, eb.value.decode(), MF._untouched(out, firth)


@pytest.mark.parametrize("what,kw", [("a NULL dataset", {}), ("firth_cutoff must be at least 0.1", dict(cutoff=0.05)),
                                     ("firth_cutoff must be at least 0.1", dict(cutoff=NAN)),
                                     ("null firth", dict(null_firth=True))])
def test_bad_arguments_are_refused_with_the_outputs_untouched(lib, what, kw):
    rc, msg, untouched = _raw(lib, None, np.array([[0.0, 1.0]]), **kw)
    assert rc == lib.PGH_ERR_ARG and msg and untouched, (what, rc, msg, untouched)
    if kw:
        assert what in msg, (what, msg)


@pytest.mark.parametrize("k", PARITY_K)
@pytest.mark.parametrize("n", [n for _, n, _ in MIXED])
def test_the_parity_inputs_reach_every_case_of_the_dosage_rule(n, k):
    """Conditions on the inputs, not on the device, so that no case can pass on rows that are left alone: the oracle
    decides every row (it asserts where the contract does not) and fails none, and over the three phenotypes together
    the applied rows cover full and partial tracks, track-less variants, E = N and separated rows."""
    inp = parity_inputs(n)
    s = _summary(inp, oracle_case(inp, k))
    print(f"n={n} k={k}: {s}")
    assert s["failed"] == 0 and 0 < s["evals"] <= PARITY_MAX_EVALS, (n, k, s)
    for key, least in PARITY_MIN.items():
        assert s[key] >= least, (n, k, key, s)


@pytest.mark.parametrize("k", WIDTHS)
def test_the_width_inputs_have_applied_rows_at_every_width(k):
    inp = widths_inputs()
    s = _summary(inp, oracle_case(inp, k, WIDTHS_STRIDE))
    print(f"k={k}: {s}")
    assert s["per"] >= 3 and s["failed"] == 0, (k, s)


@pytest.mark.parametrize("n,k", [(n, k) for n in EDGE64 for k in EDGE64_K] + [(n, STEPS_K) for n in STEPS])
def test_the_edge_inputs_have_applied_rows(n, k):
    inp = edge_inputs(n)
    cols = oracle_case(inp, k)
    s = _summary(inp, cols)
    print(f"n={n} k={k}: {s}")
    assert s["per"] >= 3 and s["failed"] == 0, (n, k, s)
    if n == 4097:  # an entry in the first word of the walk's second step
        Y = phenotypes(n)
        assert any(not np.isnan(Y[p][4096]) and inp.x[i, 4096] not in (-9.0, 0.0)
                   for p, col in enumerate(cols) for i, _ in applied_rows(col)), s


def test_the_structured_inputs_are_decided_and_hold_the_named_rows():
    lay = structured_inputs()[0]
    col = structured_oracle()
    for name in STRUCTURED_NAMED:
        assert lay.variants(name), name
    for name in ("restated_sparse", "restated_gaps", "restated_full"):
        assert len(lay.variants(name)) == 4, name
    applied = applied_rows(col)
    whole = sum(bool(w[5]["whole"]) for _, w in applied)
    print(f"structured tracks: {len(applied)} applied of {lay.m}, {whole} with E = N, "
          f"{sum(w[4] == 2 for w in col)} failed")
    assert len(applied) >= lay.m // 8 and whole >= 3


def test_the_model_agrees_with_the_oracle_within_the_printed_constants():
    """The smallest parity file at every k and one edge case: the whole runs are the tool's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import glm_score_dense_dosage_firth_model as M
    finally:
        sys.path.pop(0)
    inp = parity_inputs(257)
    worst = max(M.run_case(inp, k, 1, quiet=True)[0] for k in PARITY_K)
    assert 0 < worst <= MODEL_WORST, worst
    worst = M.run_case(edge_inputs(65), 2, 1, quiet=True)[0]
    assert 0 < worst <= MODEL_WORST_WIDTHS, worst


# ---- on the GPU --------------------------------------------------------------------------------------------------

_col, _rows, _same, _same_rows = MF._col, MF._rows, MF._same, MF._same_rows


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("glm_score_multi_dosage_firth")
    made_files = {}

    def get(name, inp):
        if name not in made_files:
            made_files[name] = DSPA._File(tmp, name, inp)
        return made_files[name]

    yield get
    for f in made_files.values():
        if f.ds is not None:
            f.ds.close()


def _check(got, cols, tol, ctx):
    """Every column against the oracle's; returns the applied rows per phenotype."""
    counts = []
    assert not got["firth"].any(), ctx
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
    got = ds.glm_score_multi_dosage_firth(Y, zc, firth_cutoff=CUTOFF)
    for key in FIRTH_KEYS:
        assert got[key].shape == (inp.m, len(Y)) and got[key].dtype == np.float64
    assert got["firth_state"].shape == (inp.m, len(Y)) and got["firth_state"].dtype == np.uint8
    _same_rows(got, ds.glm_score_multi_dosage(Y, zc), ctx=(n, k))
    counts = _check(got, oracle_case(inp, k), TOL, f"n={n} k={k}")
    assert sum(counts) >= PARITY_MIN["applied"] and min(counts) >= PARITY_MIN["per"]


@pytest.mark.gpu
def test_bit_for_bit_against_the_hardcall_route(gpu_lib, files, tmp_path):
    L = gpu_lib
    n, k = 1003, 3
    Y, Z = phenotypes(n), covariates(n, k)
    # (a) the track-less variants of a mixed file
    inp = parity_inputs(n)
    f = files(f"mixed_{n}", inp)
    got = f.open(L).glm_score_multi_dosage_firth(Y, Z, firth_cutoff=CUTOFF)
    with pytest.raises(ValueError, match="hardcalls only"):
        f.ds.glm_score_multi_firth(Y, Z, firth_cutoff=CUTOFF)
    hard = f.hard(L)
    want = hard.glm_score_multi_firth(Y, Z, firth_cutoff=CUTOFF)
    assert (~inp.track).sum() >= 10 and (want["firth_state"][~inp.track] == 1).any()
    _same(_rows(got, ~inp.track), _rows(want, ~inp.track), ctx="track-less variants")
    changed = ~np.array([np.array_equal(got["beta_firth"][v], want["beta_firth"][v], equal_nan=True)
                         for v in range(inp.m)])
    assert changed[inp.track].any() and not changed[~inp.track].any()
    # (b) a file with no track at all through the new entry
    _same(hard.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=CUTOFF), want, ctx="no tracks")
    hard.close()
    # (c) tracks of each encoding that restate their calls (test_glm_score_multi_dosage._restated_case)
    case, hard_path = MD._restated_case(tmp_path, n)
    assert case.track.sum() > 60 and {0x20, 0x40, 0x60} <= set(case.dkinds)
    hard = L.Dataset.open(hard_path)
    want = hard.glm_score_multi_firth(Y, Z, firth_cutoff=1.0)
    hard.close()
    assert (want["firth_state"][case.track] == 1).sum() >= 20
    ds = L.Dataset.open(case.path)
    _same(ds.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=1.0), want, ctx="restated")
    ds.close()
    # (d) dosage_shapes' restated rows (sparse, with gaps, full) and its track-less variants
    lay, x, Zs, y = structured_inputs()
    f = files("structured", Inputs(lay.hard, lay.dos, lay.kinds.tolist()))
    got = f.open(L).glm_score_multi_dosage_firth(y[None, :], Zs, firth_cutoff=STRUCTURED_CUTOFF)
    hard = f.hard(L)
    want = hard.glm_score_multi_firth(y[None, :], Zs, firth_cutoff=STRUCTURED_CUTOFF)
    hard.close()
    calls = np.array([not lay.kinds[v] or lay.names[v].startswith("restated_") for v in range(lay.m)])
    for name in ("restated_sparse", "restated_gaps", "restated_full"):
        vs = lay.variants(name)
        assert calls[vs].all() and all(code is None for code in want["errcode"][vs, 0]), name
    assert (want["firth_state"][calls, 0] == 1).sum() >= 5
    _same(_rows(got, calls), _rows(want, calls), ctx="dosage_shapes")


@pytest.fixture(scope="module")
def case_1003(gpu_lib, files):
    """n = 1003, k = 3: the inputs and the whole-range result that the independence tests share."""
    inp = parity_inputs(1003)
    f = files("mixed_1003", inp)
    Y, Z = phenotypes(1003), covariates(1003, 3)
    whole = f.open(gpu_lib).glm_score_multi_dosage_firth(Y, Z, firth_cutoff=CUTOFF)
    assert all((whole["firth_state"][:, p] == 1).sum() >= PARITY_MIN["per"] for p in range(len(Y)))
    return types.SimpleNamespace(inp=inp, f=f, ds=f.ds, Y=Y, Z=Z, whole=whole)


@pytest.mark.gpu
def test_a_pair_does_not_depend_on_the_other_phenotypes_or_its_place(gpu_lib, case_1003):
    c = case_1003
    _same(c.ds.glm_score_multi_dosage_firth(c.Y, c.Z, firth_cutoff=CUTOFF), c.whole, ctx="again")
    for p in range(len(c.Y)):
        _same(_col(c.ds.glm_score_multi_dosage_firth(c.Y[p:p + 1], c.Z, firth_cutoff=CUTOFF), 0), _col(c.whole, p),
              ctx=("alone", p))
    moved = c.ds.glm_score_multi_dosage_firth(c.Y[::-1], c.Z, firth_cutoff=CUTOFF)
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
    three = c.ds.glm_score_multi_dosage_firth(c.Y, Z, firth_cutoff=CUTOFF)
    got = c.ds.glm_score_multi_dosage_firth(Y17, Z, firth_cutoff=CUTOFF)
    assert (three["firth_state"] == 1).sum() >= 10
    for p in range(MD.LAYOUT_PHENOTYPES - 1):
        _same(_col(got, p), _col(three, p % 3), ctx=(k, p))
    _same(_col(got, 16), _col(c.ds.glm_score_multi_dosage_firth(own[None, :], Z, firth_cutoff=CUTOFF), 0), ctx=(k, 16))


@pytest.mark.gpu
def test_a_pair_does_not_depend_on_the_range_the_window_or_the_scratch_budget(gpu_lib, case_1003):
    L = gpu_lib
    c = case_1003
    run = lambda ds, **kw: ds.glm_score_multi_dosage_firth(c.Y, c.Z, firth_cutoff=CUTOFF, **kw)
    _same(run(c.ds, v_begin=37), _rows(c.whole, slice(37, None)), ctx="v_begin = 37")
    part = L.Dataset.open(c.f.path, variant_begin=37, variant_end=c.inp.m)
    _same(run(part), _rows(c.whole, slice(37, c.inp.m)), ctx="window")
    _same(run(part, v_begin=41, v_end=63), _rows(c.whole, slice(41, 63)), ctx="window range")
    part.close()
    # The scratch budget, as test_glm_score_multi_dosage_spa splits it.  At n = 1003 the smallest column block is 1024
    # sample rows x 64 columns x 8 bytes = 524,288 bytes and a phenotype's mask 256 bytes: a budget of which three
    # quarters are less leaves one phenotype per block, so the three run as three blocks.  What the block leaves goes to
    # one workgroup's stash first (16 bytes x 1003 samples = 16,048; never less than one) and then bounds the chunk: per
    # variant and phenotype 244 bytes of sums, entries, count and row (k = 3) and 32 of the Firth row, plus the expanded
    # rows' 144 bytes per 64 samples and 4 bytes of list: 2,584 bytes.  1 byte: chunks of one variant; block + stash +
    # 7 x 2,584: of seven.
    per_variant = 244 + 32 + 144 * 16 + 4
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
    mask = SS.shapes(c.inp.n)[SUBSET_SHAPE]
    assert mask[:16].sum() not in (0, 16)
    Z, Y = np.ascontiguousarray(c.Z[:, mask]), np.ascontiguousarray(c.Y[:, mask])
    x = c.inp.x[:, mask]
    ss = c.ds.subset(mask)
    got = c.ds.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=CUTOFF, subset=ss)
    _same_rows(got, c.ds.glm_score_multi_dosage(Y, Z, subset=ss), ctx=SUBSET_SHAPE)
    total = 0
    for p, y in enumerate(Y):
        applied, worst = D.check_column(got, p, D.oracle_column(x, y, Z, CUTOFF), TOL, ctx=(SUBSET_SHAPE, p))
        print(f"{SUBSET_SHAPE} ({int(mask.sum())} samples) phenotype {p}: {applied} applied, worst {worst:.3g}")
        total += applied
    assert total >= 5
    ss.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_instantiated_width(gpu_lib, files, k):
    """The kernel has no width of its own; the block's leading dimension and the phenotype's column, p (k + 2), follow
    every width GlmPadCovar returns, at k = KP and one above the width below."""
    inp = widths_inputs()
    ds = files("widths", inp).open(gpu_lib)
    Y, Z = phenotypes(inp.n), covariates(inp.n, k)
    got = ds.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=CUTOFF)
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
    got = ds.glm_score_multi_dosage_firth(Y, zc, firth_cutoff=CUTOFF)
    _same_rows(got, ds.glm_score_multi_dosage(Y, zc), ctx=(n, k))
    assert min(_check(got, oracle_case(inp, k), TOL_WIDTHS, f"n={n} k={k}")) >= 3


@pytest.mark.gpu
def test_structured_tracks(gpu_lib, files):
    """dosage_shapes' file of one tile, one phenotype at cutoff 1.0, every row against the oracle; the encodings of a
    row agree bit for bit."""
    lay, x, Z, y = structured_inputs()
    ds = files("structured", Inputs(lay.hard, lay.dos, lay.kinds.tolist())).open(gpu_lib)
    got = ds.glm_score_multi_dosage_firth(y[None, :], Z, firth_cutoff=STRUCTURED_CUTOFF)
    col = structured_oracle()
    applied, worst = D.check_column(got, 0, col, TOL_WIDTHS, ctx="structured")
    print(f"structured tracks: {applied} applied of {lay.m}, worst {worst:.3g} (tolerance {TOL_WIDTHS:.3g})")
    assert applied == len(applied_rows(col))
    for name in STRUCTURED_NAMED:
        for v in lay.variants(name):
            print(f"  {name} ({hex(int(lay.kinds[v]))}): state {got['firth_state'][v, 0]}, beta_firth "
                  f"{got['beta_firth'][v, 0]:.6g}, beta {got['beta'][v, 0]:.6g}")
            assert got["firth_state"][v, 0] == col[v][4], (name, v)
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
    rc, msg, untouched = _raw(L, ds._h, Y, null_firth=True)
    assert rc == L.PGH_ERR_ARG and "null firth" in msg and untouched, (rc, msg)
    with pytest.raises(ValueError, match="firth_cutoff must be at least 0.1"):
        ds.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=0.05)
    # pgh_glm_score_multi_firth still refuses the file with tracks, with its text
    out, firth = MF._fill(L, 4 * len(Y))
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = L.raw().pgh_glm_score_multi_firth(ds._h, None, 0, 4, len(Y), MF._ptr(Y), 0, None, C.c_double(CUTOFF),
                                           MF._ptr(out), MF._ptr(firth), eb)
    assert rc == L.PGH_ERR_ARG and "hardcalls only" in eb.value.decode() and MF._untouched(out, firth)
    # an empty range
    rc, msg, untouched = _raw(L, ds._h, Y, v0=3, v1=3)
    assert rc == L.PGH_OK and untouched, msg
    empty = ds.glm_score_multi_dosage_firth(Y, Z, v_begin=77, v_end=77)
    assert all(empty[key].shape == (0, len(Y)) for key in FIRTH_KEYS + ("firth_state", "beta"))
    # a cutoff of +infinity never applies it
    base = ds.glm_score_multi_dosage(Y, Z)
    never = ds.glm_score_multi_dosage_firth(Y, Z, firth_cutoff=math.inf)
    _same_rows(never, base, ctx="inf")
    assert not never["firth_state"].any()
    for key, of in zip(FIRTH_KEYS, ("beta", "se", "p")):
        assert np.array_equal(never[key], base[of], equal_nan=True), key
    assert np.isnan(base["p"]).any() and not np.isnan(base["p"]).all()
    # the C rows: pad is zero and out's firth byte stays 0
    out, firth = MF._fill(L, inp.m * len(Y))
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = getattr(L.raw(), NAME)(ds._h, None, 0, inp.m, len(Y), MF._ptr(Y), len(Z), MF._ptr(Z), C.c_double(CUTOFF),
                                MF._ptr(out), MF._ptr(firth), eb)
    assert rc == L.PGH_OK, eb.value
    rows_c, firth_c = out.view(L.GLM_ROW_DTYPE), firth.view(L.GLM_FIRTH_ROW_DTYPE)
    assert not firth_c["pad"].any() and not rows_c["firth"].any() and (firth_c["state"] == 1).any()
