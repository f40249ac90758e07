"""The int8 fixed-point score contraction (score_i8.hip) held to its digit-level contract.

tests/score_i8_model.py restates the scheme in Python integers.  The GPU tests here assert

  * `device == F` bit for bit where every digit sum, every epilogue addition and k0 are exactly representable
    (grid-aligned weights under one large scale-fixing weight), and
  * `|device - E| <= (u / 2) sum_v (c + miss) + R` on real weights, E the real-number sum and R the floating-point
    allowance that `score_i8_model.allowance` derives from the operation counts,

and the CPU tests check, on the very same inputs, that the model passes those assertions and that four faulty models
(a lost lowest digit, truncation for rint, a dropped carry, one digit position's multiplier off by 256) fail them
at some sample of every weight column -- which is what keeps the GPU tests from being vacuous.

What cannot be asserted as the plain rule would have it, and why:
  * Center mode is never exact: sd = sqrt(2 f (1 - f)) is irrational for every dyadic f, so k0 = sum w t0 is a sum
    of inexact doubles whose order (block tree, atomics) is not fixed.  There the integer part is still exact and the
    assertion is |device - F| <= (k0_depth + 1) g sum |w t0| + g |F| (the k0 sum and the one final addition), on the
    samples that are hom-ref at the scale-fixing row -- a center-mode row cannot be both scored and carried by nobody.
    That allowance is about 2 u at the five-sample shape and below 0.1 u at the others (asserted below 3 u); the
    truncating mutant, the mildest one, is off by tens of u.  For the same reason the power-of-two scaling test runs
    in the two modes where, without flips, k0 = 0.
  * The top digit (position 6, or 4 of the dosage sum) cannot reach -128 / 127: |x| <= 2^(8 digits - 2) keeps it
    within +-64.  The inputs reach +-64 there and -128 and 127 at every other position, in both planes.
  * The dosage sum has coefficients alpha = +-1 and beta = -3 or +-(3 - mean).  Without imputation, and with dyadic
    means, they are multiples of the upper digits' units and only a fault in the top digit can show; with the
    non-dyadic subset means of the real-weight inputs every mutant differs from F, which the device must equal
    there too (the dosage sum's integer sums are exact at any test size).  Its bound is asserted as well, but
    Q counts every unit of operand while only the missing plane is rounded, so the bound alone would not see them.
"""

import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import score_i8_model as M

gpu = pytest.mark.gpu

MODES = {"impute": M.MEAN_IMPUTE, "noimpute": M.NO_MEAN_IMPUTATION, "center": M.CENTER}
# resident rows, listed variants, samples.  A: one padded tile, one partial stripe.  B: exactly the 16-tile minimum
# slice, one atomic add per output.  C: 33 tiles -> 34 -> three slices of 16; two sample groups at every TS.
SHAPES = {"A": (90, 70, 5), "B": (1024, 1024, 513), "C": (2400, 2100, 1030)}
# 7 C + 6 digit columns: 1 .. 10 tiles of sixteen, and 23 takes a second pass
NCOLS = [1, 2, 4, 7, 9, 11, 13, 16, 18, 20, 22, 23]
SCALE_ROW = {M.MEAN_IMPUTE: 0, M.NO_MEAN_IMPUTATION: 0, M.CENTER: 1}
P_HI = [127, -128, 127, -128, 127, -128, 1]
P_LO = [-128, 127, -128, 127, -128, 127, -1]
MUTANTS = {"six_digits": dict(digits=6), "truncate": dict(rounding="truncate"), "no_carry": dict(drop_carry=True),
           "mult_off": dict(mult_off=3)}
DOSAGE_MUTANTS = {"four_digits": dict(digits=4), "truncate": dict(rounding="truncate"), "no_carry": dict(drop_carry=True),
                  "mult_off": dict(mult_off=2), "mult_off_top": dict(mult_off=4)}


def _pattern_value(p):
    return sum(d * 256 ** j for j, d in enumerate(p))


def _listed(shape, rng):
    resident, m, n = SHAPES[shape]
    vidx = np.arange(m) if resident == m else np.sort(rng.choice(resident, size=m, replace=False))
    return resident, m, n, vidx.astype(np.uint32)


def _special_rows(codes, n, n_missing, observed_for_scale):
    """Rows 0..5 of the list.  0: all hom-ref (scale-fixing outside center mode: it multiplies nothing).  1: a low,
    dyadic mean (center mode's scale-fixing row: small |t0| next to its |beta|).  2..5: two carriers and the row's
    missing calls, for the coefficients that hold the digit extremes -- their large values meet few samples."""
    codes[0] = 0
    codes[1] = 0
    hets = [0] if n < 16 else [0, n // 2]
    codes[1, hets] = 1
    pool = [s for s in range(n) if s not in hets]
    codes[1, pool[len(pool) - (n - observed_for_scale):]] = 3
    for i in range(2, 6):
        codes[i] = 0
        codes[i, (7 * i) % n] = 1
        codes[i, (7 * i + 1) % n] = 2
        for k in range(n_missing):
            codes[i, (7 * i + 2 + k) % n] = 3


# --------------------------------------------------------------------------------------------------------------
# grid-aligned inputs: device == F
# --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_matrix(shape):
    """Every row has n - 2^floor(log2 n) missing calls, so every mean is dyadic and every table entry outside center
    mode is an exact double."""
    rng = np.random.default_rng(sum(map(ord, shape)))
    resident, m, n, vidx = _listed(shape, rng)
    observed = 1 << (n.bit_length() - 1)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(resident, n), p=[0.5, 0.3, 0.2])
    for r in range(resident):
        codes[r, rng.choice(n, size=n - observed, replace=False)] = 3
    listed = codes[vidx].copy()
    _special_rows(listed, n, n - observed, observed)
    codes[vidx] = listed
    flip = (rng.random(m) < 0.4).astype(np.uint8)
    flip[:6] = 0  # (a flipped special row would put an off-grid 2 w into k0)
    return M.pack_codes(codes), vidx, listed, flip


@functools.lru_cache(maxsize=None)
def exact_inputs(shape, mode):
    _, _, listed, flip = exact_matrix(shape)
    return M.Inputs(listed, flip, mode)


@functools.lru_cache(maxsize=None)
def exact_weights(shape, mode, j):
    """Column j: ordinary weights are multiples of u / 4 (ties and off-grid quarters for rint, but k0 = sum 2 w on
    the grid) small enough that the sums stay below 2^53 u; rows 2..5 carry the digit extremes of the code plane and
    of the missing plane; the scale-fixing row puts the largest coefficient at 0.999 2^e: a top digit of +-64."""
    inp = exact_inputs(shape, mode)
    rng = np.random.default_rng(1000 + j)
    e = (j * 37) % 97 - 48
    u = 2.0 ** (e - 54)
    _, d, x, _ = inp.parts("weight")
    bits = 50 - math.ceil(math.log2(12 * inp.m))
    w = rng.integers(-(1 << (bits + 2)), 1 << (bits + 2), size=inp.m).astype(np.float64) * (u / 4.0)
    if mode == M.CENTER:
        # center mode is asserted within an allowance of up to 2 u (module docstring): every alpha positive, so that
        # what truncation loses adds up row by row to far more than that instead of walking randomly
        w = np.abs(w) * np.where(d < 0.0, -1.0, 1.0)
    hi, lo = (_pattern_value(P_HI), _pattern_value(P_LO))[:: 1 if j % 2 == 0 else -1]
    w[2], w[3] = hi * u / d[2], lo * u / d[3]
    w[4], w[5] = hi * u / x[4], lo * u / x[5]
    s = SCALE_ROW[mode]
    w[s] = (-1.0 if j % 2 else 1.0) * 0.999 * 2.0 ** e / abs(x[s])
    return w


@functools.lru_cache(maxsize=None)
def exact_column(shape, mode, j, mutant=None, fused=False):
    return M.column_model(exact_inputs(shape, mode), exact_weights(shape, mode, j), **(MUTANTS[mutant] if mutant else {}),
                          fused=fused)


@functools.lru_cache(maxsize=None)
def exact_dosage(shape, mode, mutant=None):
    return M.column_model(exact_inputs(shape, mode), None, "dosage", **(DOSAGE_MUTANTS[mutant] if mutant else {}))


def asserted_samples(shape, mode):
    """Center mode: the samples that are hom-ref at the scale-fixing row (see the module docstring)."""
    inp = exact_inputs(shape, mode)
    return np.flatnonzero(inp.codes[1] == 0) if mode == M.CENTER else np.arange(inp.n)


def center_allowance(inp, col):
    """|device - F| in center mode: k0's terms pass through k0_depth roundings of partial sums below sum |w t0| and
    the device may fuse their products (F rounds them); the digit part is exact; one final addition rounds F."""
    return [(M.k0_depth(inp.m) + 1) * M.GAMMA * col.k0_abs + M.GAMMA * abs(f) for f in col.F]


def check_exact(shape, mode, col, got):
    """The assertion the GPU tests make of a grid-aligned column (got: one value per sample); also run on the model
    itself and on the mutants by the CPU tests.  Returns the samples that violate it."""
    rows = asserted_samples(shape, mode)
    if mode != M.CENTER:
        want = np.array([float(f) for f in col.F])
        return [s for s in rows if not got[s] == want[s]]
    allow = center_allowance(exact_inputs(shape, mode), col)
    return [s for s in rows if abs(Fraction(float(got[s])) - col.F[s]) > allow[s]]


EXACT_CASES = ([("A", mo, nc) for mo in MODES for nc in NCOLS] + [("B", mo, nc) for mo in MODES for nc in (1, 4, 16)] +
               [("C", "noimpute", nc) for nc in NCOLS] + [("C", mo, nc) for mo in ("impute", "center") for nc in (2, 9)])


def exact_cols(shape, mode):
    """How many of the columns 0, 1, 2 .. the GPU cases of this shape and mode use."""
    return max(nc for sh, mo, nc in EXACT_CASES if (sh, mo) == (shape, mode))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_model_passes_the_exact_assertions_and_every_mutant_fails_them(shape, mode):
    md = MODES[mode]
    inp = exact_inputs(shape, md)
    rows = asserted_samples(shape, md)
    assert len(rows) >= inp.n - 8
    for j in range(exact_cols(shape, mode)):
        col = exact_column(shape, md, j)
        assert col.e == (j * 37) % 97 - 48
        # every partial sum of the epilogue, in any order and over any slices, is an integer below 2^53 units
        assert float(col.mass[rows].max()) < 2.0 ** 53 * (1 - 2.0 ** -20), (j, float(col.mass.max()))
        if md != M.CENTER:
            # ... and k0 and the final addition are exact too: F is a double
            assert all(Fraction(float(f)) == f for f in col.F), j
        else:
            # the cut does not depend on whether x = -t0 - 3 d was fused, except at the scale row, which the
            # asserted samples do not carry
            other = exact_column(shape, md, j, fused=True)
            keep = np.arange(inp.m) != SCALE_ROW[md]
            assert np.array_equal(col.A, other.A) and np.array_equal(col.B[keep], other.B[keep]) and col.e == other.e
            allow = center_allowance(inp, col)
            assert max(allow[s] for s in rows) < 3 * col.u
        model_out = np.array([float(f) for f in col.F])
        assert check_exact(shape, md, col, model_out) == []
        for name in MUTANTS:
            bad = exact_column(shape, md, j, name)
            if md != M.CENTER:
                assert any(bad.F[s] != col.F[s] for s in rows), (j, name)
            else:
                # beyond twice the allowance: no rounding inside it can carry a mutant back
                allow = center_allowance(inp, col)
                assert any(abs(bad.F[s] - col.F[s]) > 2 * allow[s] for s in rows), (j, name)
    if md != M.CENTER:
        dos = exact_dosage(shape, md)
        assert all(Fraction(float(f)) == f for f in dos.F)
        clean = np.flatnonzero((inp.codes == 3).sum(axis=0) == 0)
        scored = np.where(inp.flip[:, None] != 0, 2 - inp.codes.astype(np.int64), inp.codes.astype(np.int64))
        assert all(dos.F[s] == int(scored[:, s].sum()) for s in clean)
        # (dyadic means are multiples of 2^-10: they fit in the top two digits, and only a fault there shows here;
        # the subset means of the real-weight inputs below fill all five)
        assert exact_dosage(shape, md, "mult_off_top").F != dos.F


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_exact_inputs_reach_the_digit_extremes_in_both_planes(shape, mode):
    md = MODES[mode]
    for j in range(exact_cols(shape, mode)):
        col = exact_column(shape, md, j)
        for plane in (col.a, col.b):
            for pos in range(6):
                assert plane[:, pos].min() == -128 and plane[:, pos].max() == 127, (j, pos)
            assert plane[:, 6].min() < 0 < plane[:, 6].max(), j
        # the column's largest coefficient (0.999 2^e on the scale row) holds the top digit's own limit
        assert abs(int(col.b[SCALE_ROW[md], 6])) == 64, j


def _plan_run(ds, vidx, w, flip, mode, mask):
    import torch
    n = ds.n_samples
    ss = None if mask is None else ds.subset(mask)
    plan = ds.score_plan(vidx, w, flip, mode, ss)
    d_score = torch.zeros((n, w.shape[1]), dtype=torch.float64, device="cuda")
    d_dos = torch.zeros(n, dtype=torch.float64, device="cuda")
    d_ac = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.run_dev(d_score.data_ptr(), d_dos.data_ptr(), d_ac.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    s, d = d_score.cpu().numpy(), d_dos.cpu().numpy()
    return (s, d) if mask is None else (s[mask], d[mask])


def device_runs(L, ds, vidx, w, flip, mode, mask=None):
    """The one-shot pgh_score, and for nine columns and more (the TS = 4 shapes) a kept plan as well: it streams the
    tile-major copy through the software-pipelined loop."""
    ss = None if mask is None else ds.subset(mask)
    s, d, _ = ds.score(vidx, w, flip=flip, mode=mode, subset=ss)
    yield "score", s, d
    if w.shape[1] >= 9:
        s, d = _plan_run(ds, vidx, w, flip, mode, mask)
        yield "plan", s, d


_datasets = {}


def dataset(L, kind, shape):
    if (kind, shape) not in _datasets:
        rows = (exact_matrix if kind == "exact" else bound_matrix)(shape)[0]
        _datasets[(kind, shape)] = L.Dataset.from_host_rows(rows, SHAPES[shape][2])
    return _datasets[(kind, shape)]


def check_exact_dosage(shape, md, d, tag):
    if md == M.CENTER:
        assert not d.any(), tag
        return
    want = np.array([float(f) for f in exact_dosage(shape, md).F])
    assert np.array_equal(d, want), (tag, int((d != want).sum()))


@gpu
@pytest.mark.parametrize("shape,mode,ncols", EXACT_CASES)
def test_device_equals_the_fixed_point_model_bit_for_bit(gpu_lib, shape, mode, ncols):
    md = MODES[mode]
    _, vidx, _, flip = exact_matrix(shape)
    w = np.stack([exact_weights(shape, md, j) for j in range(ncols)], axis=1)
    for tag, s, d in device_runs(gpu_lib, dataset(gpu_lib, "exact", shape), vidx, w, flip, md):
        for j in range(ncols):
            bad = check_exact(shape, md, exact_column(shape, md, j), s[:, j])
            assert bad == [], (tag, j, len(bad), bad[:5])
        check_exact_dosage(shape, md, d, tag)


# --------------------------------------------------------------------------------------------------------------
# real weights: |device - E| <= Q + R
# --------------------------------------------------------------------------------------------------------------

BOUND_COLS = {"A": 2, "B": 4, "C": 9}


@functools.lru_cache(maxsize=None)
def bound_matrix(shape):
    """Random calls with 3 % missing, flips, and a sample subset (tables come from the subset's counts; the contraction
    runs over everybody).  Row 0 is hom-ref everywhere, row 1 has a low mean inside the subset."""
    rng = np.random.default_rng(77 + sum(map(ord, shape)))
    resident, m, n, vidx = _listed(shape, rng)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(resident, n), p=[0.5, 0.3, 0.2])
    codes[rng.random((resident, n)) < 0.03] = 3
    mask = rng.random(n) < 0.6
    if n < 16:
        mask[:] = True
        mask[2] = False
    listed = codes[vidx].copy()
    listed[0] = 0
    listed[1] = 0
    inc = np.flatnonzero(mask)
    listed[1, inc[: 1 if n < 16 else 2]] = 1
    if n >= 16:
        listed[1, inc[-2:]] = 3
    codes[vidx] = listed
    flip = (rng.random(m) < 0.4).astype(np.uint8)
    return M.pack_codes(codes), vidx, listed, flip, mask


@functools.lru_cache(maxsize=None)
def bound_inputs(shape, mode):
    _, _, listed, flip, mask = bound_matrix(shape)
    return M.Inputs(listed, flip, mode, include=mask)


@functools.lru_cache(maxsize=None)
def bound_weights(shape, mode, j):
    """Real weights: magnitudes within a factor 2 (even columns) or over six decades (odd ones), 2^11 and more below
    the column's scale-fixing weight -- R scales with the coefficients, Q with u, and a bound that R swamps would let
    the mutants through.  Every alpha is positive with a fractional part of 0.9 u, so that what truncation loses adds
    up sample by sample instead of walking randomly."""
    inp = bound_inputs(shape, mode)
    rng = np.random.default_rng(5000 + j)
    e = (j * 29) % 61 - 30
    u = 2.0 ** (e - 54)
    _, d, x, _ = inp.parts("weight")
    mag = 2.0 ** (e - 12) * (rng.uniform(1.0, 2.0, inp.m) if j % 2 == 0 else 2.0 * 10.0 ** rng.uniform(-6.0, 0.0, inp.m))
    target = (np.floor(mag / u) + 0.9) * u
    w = np.where(d != 0.0, target / np.where(d != 0.0, d, 1.0), mag)
    s = SCALE_ROW[mode]
    w[s] = (-1.0 if j % 2 else 1.0) * 0.999 * 2.0 ** e / abs(x[s])
    return w


@functools.lru_cache(maxsize=None)
def bound_column(shape, mode, j, mutant=None):
    """(model, E, Q, R); j = None: the dosage sum."""
    inp = bound_inputs(shape, mode)
    w, target = (None, "dosage") if j is None else (bound_weights(shape, mode, j), "weight")
    good = M.column_model(inp, w, target)
    if mutant:
        return M.column_model(inp, w, target, **(MUTANTS if j is not None else DOSAGE_MUTANTS)[mutant])
    Q, R = M.allowance(inp, w, good, target)
    return good, M.true_sum(inp, w, good.u, target), Q, R


def bound_violations(shape, mode, j, got, slack=1):
    """Samples of the subset at which |got - E| > Q + slack R (got: one value per sample of the subset)."""
    _, E, Q, R = bound_column(shape, mode, j)
    inc = np.flatnonzero(bound_inputs(shape, mode).include)
    return [k for k, s in enumerate(inc) if abs(Fraction(float(got[k])) - E[s]) > Q[s] + slack * R[s]]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_model_is_within_the_bound_and_every_mutant_is_outside_it(shape, mode):
    md = MODES[mode]
    inp = bound_inputs(shape, md)
    inc = np.flatnonzero(inp.include)
    for j in range(BOUND_COLS[shape]):
        good, E, Q, R = bound_column(shape, md, j)
        assert good.e == (j * 29) % 61 - 30
        # the model, and the model with the other contraction of x, sit inside the quantisation term plus the
        # table and product part of R
        assert bound_violations(shape, md, j, [float(good.F[s]) for s in inc]) == []
        # R does not swamp Q: at the subset's most loaded sample it is below half of it
        top = max(inc, key=lambda s: Q[s])
        assert R[top] * 2 < Q[top], (j, float(R[top] / good.u), float(Q[top] / good.u))
        for name in MUTANTS:
            bad = bound_column(shape, md, j, name)
            # outside the bound by a further R: no rounding the allowance covers can carry the mutant back inside
            assert bound_violations(shape, md, j, [float(bad.F[s]) for s in inc], slack=2) != [], (j, name)
    if md != M.CENTER:
        good, E, Q, R = bound_column(shape, md, None)
        assert bound_violations(shape, md, None, [float(good.F[s]) for s in inc]) == []
        # the dosage sum's integers stay far below 2^53 units at any test size: the device must equal F as well
        assert float(good.mass.max()) + float(good.k0_abs / good.u) < 2.0 ** 52
        assert all(Fraction(float(f)) == f for f in good.F)
        for name in DOSAGE_MUTANTS if md == M.MEAN_IMPUTE else ["mult_off_top"]:
            bad = bound_column(shape, md, None, name)
            assert any(bad.F[s] != good.F[s] for s in inc), name


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_device_is_within_the_derived_bound_of_the_real_number_sum(gpu_lib, shape, mode):
    md = MODES[mode]
    _, vidx, _, flip, mask = bound_matrix(shape)
    ncols = BOUND_COLS[shape]
    w = np.stack([bound_weights(shape, md, j) for j in range(ncols)], axis=1)
    for tag, s, d in device_runs(gpu_lib, dataset(gpu_lib, "bound", shape), vidx, w, flip, md, mask):
        for j in range(ncols):
            bad = bound_violations(shape, md, j, s[:, j])
            assert bad == [], (tag, j, len(bad), bad[:5])
        if md == M.CENTER:
            assert not d.any()
        else:
            # the dosage sum, with its own u = 2^(e - 38), in place of the other tests' 1e-9 -- and, its integer sums
            # being exact at this size, equal to the 5-digit model
            assert bound_violations(shape, md, None, d) == [], tag
            want = np.array([float(bound_column(shape, md, None)[0].F[s]) for s in np.flatnonzero(mask)])
            assert np.array_equal(d, want), (tag, int((d != want).sum()))


# --------------------------------------------------------------------------------------------------------------
# power-of-two scaling, edge columns
# --------------------------------------------------------------------------------------------------------------

# columns -> {scaled column: (its base column, k)}: the scaled column is 2^k times the base.  A column's seven digits
# start at lane 7 t % 16 of a tile.  Nine columns: 0, 1, 3, 5, 7 start at lanes 0, 7, 5, 3, 1, so each sits in one tile
# and goes through the same three shuffle additions.  Twenty columns (ten tiles): t and t + 16 start at the same lane,
# so column 18 straddles two tiles exactly as column 2 does -- two partial sums, two atomic adds onto zero, which
# commute.  (A scaled copy at another lane would be summed in another order and might round differently.)
SCALINGS = {9: {1: (0, -900), 3: (0, -1), 5: (0, 1), 7: (0, 900)},
            20: {16: (0, 900), 17: (1, 1), 18: (2, -900), 19: (3, -1)}}


@functools.lru_cache(maxsize=None)
def scaling_weights(mode, ncols):
    """Real weights over shape B (one slice per output).  With no flips k0 = 0 outside center mode, so every step of
    the device -- the cut, the integer sums, the lane sums, the atomic adds -- commutes with a power of two."""
    w = np.stack([bound_weights("B", mode, j) for j in range(ncols)], axis=1)
    for c, (base, k) in SCALINGS[ncols].items():
        w[:, c] = np.ldexp(w[:, base], k)
    return w


@pytest.mark.parametrize("mode", ["impute", "noimpute"])
@pytest.mark.parametrize("ncols", SCALINGS)
def test_model_scales_exactly_with_powers_of_two(mode, ncols):
    md = MODES[mode]
    _, _, listed, _, mask = bound_matrix("B")
    inp = M.Inputs(listed, None, md, include=mask)
    w = scaling_weights(md, ncols)
    for c, (b, k) in SCALINGS[ncols].items():
        # the same number of digits in the column's first tile: the same additions in the same order
        assert min(7, 16 - (7 * c) % 16) == min(7, 16 - (7 * b) % 16)
        base, col = M.column_model(inp, w[:, b]), M.column_model(inp, w[:, c])
        assert base.k0 == 0 and any(base.F)
        assert col.e == base.e + k and np.array_equal(col.a, base.a) and np.array_equal(col.b, base.b)
        assert col.F == [f * Fraction(2) ** k for f in base.F]
        # a fault in one of the two columns alone (here: the scaled one cut by truncation) breaks the equality
        bad = M.column_model(inp, w[:, c], rounding="truncate")
        assert bad.F != [f * Fraction(2) ** k for f in base.F]


@gpu
@pytest.mark.parametrize("mode", ["impute", "noimpute"])
@pytest.mark.parametrize("ncols", SCALINGS)
def test_power_of_two_scaling_of_a_column_is_exact(gpu_lib, mode, ncols):
    md = MODES[mode]
    _, vidx, _, _, mask = bound_matrix("B")
    w = scaling_weights(md, ncols)
    for tag, s, _ in device_runs(gpu_lib, dataset(gpu_lib, "bound", "B"), vidx, w, None, md, mask):
        for c, (b, k) in SCALINGS[ncols].items():
            assert s[:, b].any()
            assert np.array_equal(s[:, c], np.ldexp(s[:, b], k)), (tag, c)


EDGE_LAYOUTS = {6: {1: "zero", 3: "single", 5: "pow2"}, 10: {0: "pow2", 4: "zero", 9: "single"}}


@functools.lru_cache(maxsize=None)
def edge_weights(shape, mode, ncols):
    """Ordinary grid-aligned columns with three edge columns among them: all zero; one nonzero weight; and a column
    whose largest coefficient is exactly a power of two -- the scale row's weight is fl(2^e / 3), and
    beta = fl(-3 w) = -2^e although 3 w < 2^e over the reals: frexp must see the double."""
    inp = exact_inputs(shape, mode)
    w = np.stack([exact_weights(shape, mode, j) for j in range(ncols)], axis=1)
    for c, kind in EDGE_LAYOUTS[ncols].items():
        if kind == "zero":
            w[:, c] = 0.0
        elif kind == "single":
            w[:, c] = 0.0
            w[6 + int(np.argmin(inp.flip[6:])), c] = 0.7853981633974483  # (an unflipped row: no 2 w in k0)
        else:
            e = (c * 37) % 97 - 48
            w[0, c] = 2.0 ** (e - 1) / 3.0
            assert w[0, c] * -3.0 == -(2.0 ** (e - 1)) and Fraction(w[0, c]) * 3 < Fraction(2) ** (e - 1)
    return w


@pytest.mark.parametrize("shape", ["A", "C"])
@pytest.mark.parametrize("mode", ["impute", "noimpute"])
@pytest.mark.parametrize("ncols", EDGE_LAYOUTS)
def test_model_of_the_edge_columns(shape, mode, ncols):
    md = MODES[mode]
    inp = exact_inputs(shape, md)
    w = edge_weights(shape, md, ncols)
    for c, kind in EDGE_LAYOUTS[ncols].items():
        col = M.column_model(inp, w[:, c])
        assert all(Fraction(float(f)) == f for f in col.F)
        if kind == "zero":
            assert col.e == 0 and not any(col.F)
        elif kind == "single":
            assert any(col.F) and np.count_nonzero(col.A) == 1
        else:
            # the boundary: the largest coefficient is 2^(e-1) = 0.5 x 2^e, so the exponent is e, not e - 1
            assert col.e == (c * 37) % 97 - 48 and int(col.B[0]) == -(2 ** 53)
            assert float(col.mass.max()) < 2.0 ** 53


@gpu
@pytest.mark.parametrize("shape", ["A", "C"])
@pytest.mark.parametrize("mode", ["impute", "noimpute"])
@pytest.mark.parametrize("ncols", EDGE_LAYOUTS)
def test_edge_columns_next_to_ordinary_ones(gpu_lib, shape, mode, ncols):
    md = MODES[mode]
    _, vidx, _, flip = exact_matrix(shape)
    inp = exact_inputs(shape, md)
    w = edge_weights(shape, md, ncols)
    for tag, s, d in device_runs(gpu_lib, dataset(gpu_lib, "exact", shape), vidx, w, flip, md):
        for c in range(ncols):
            kind = EDGE_LAYOUTS[ncols].get(c)
            # an ordinary column is what it is without the edge columns next to it: the same F
            col = M.column_model(inp, w[:, c]) if kind else exact_column(shape, md, c)
            want = np.array([float(f) for f in col.F])
            assert np.array_equal(s[:, c], want), (tag, c, kind)
        check_exact_dosage(shape, md, d, tag)
