"""A plain restatement of the fixed-point scheme behind plink_score's int8 contraction (DESIGN.md section 3.4,
`k_score_tables`, `k_i8_ranges`, `k_i8_columns`, `k_i8_digits`), in numpy and Python integers.  It does not call the
library; tests/test_score_fixed_point.py holds the device to it.

Per target column (a weight column, or the unweighted dosage sum with w = 1 and the dosage tables):

    alpha_v = w_v d_v,   beta_v = w_v (t3_v - t0_v - 3 d_v),   k0 = sum_v w_v t0_v,       d_v = t1_v - t0_v
    e = frexp(max_v max(|alpha_v|, |beta_v|)),   u = 2^(e - (8 digits - 2))
    A_v = rint(alpha_v / u),   B_v = rint(beta_v / u)       (ties to even), cut into signed base-256 digits
    F[s] = k0 + u sum_v (A_v c(v,s) + B_v miss(v,s))        c = the raw 2-bit code 0..3, miss = [c == 3]

`column_model` returns F as exact Fractions; its `rounding`, `drop_carry`, `digits` and `mult_off` parameters build the
faulty variants ("mutants") that the tests must be able to tell from the real thing.  `true_sum` is the real-number
sum E from exact tables (the mean as a rational, 1/sd to 200 bits), and `allowance` the two terms of the bound
|device - E| <= Q + R.

The per-variant tables are doubles on the device, and F is defined on those doubles: `tables` repeats
`k_score_tables` operation by operation (IEEE +, -, *, /, sqrt are correctly rounded on both sides).  One thing is
left open by the C++ source: `t3 - t0 - 3.0 * d` may or may not be contracted into a fused multiply-add.  The two
forms differ only in center mode (3 d is exact elsewhere); `Inputs.x` holds the unfused value, `Inputs.x_fused` the
other, and the tests check that their inputs cut to the same integers either way.
"""

import math
from fractions import Fraction

import numpy as np

WEIGHT_DIGITS, DOSAGE_DIGITS = 7, 5
MEAN_IMPUTE, NO_MEAN_IMPUTATION, CENTER = 0, 1, 2
EPS = Fraction(1, 2 ** 53)  # unit roundoff of a double
# (1 + EPS)^k - 1 <= k GAMMA for k <= 64 roundings in a row (Higham, gamma_k = k eps / (1 - k eps))
GAMMA = EPS / (1 - 64 * EPS)
# sum_j |d_j| 256^j <= MASS |x| for the signed base-256 digits d_j of an integer x != 0: with top digit t != 0 at
# position p, |x| >= 256^p (|t| - 128/255) and the sum is <= 256^p (|t| + 128/255); worst at |t| = 1: 1.502 / 0.498
MASS = Fraction(31, 10)
E_BITS = 64  # true_sum keeps its coefficients to 2^-64 u


def pack_codes(codes):
    """codes uint8 [m][n] in 0..3 -> packed 2-bit rows, sample s in bits 2 (s % 4) of byte s / 4."""
    m, n = codes.shape
    c = np.zeros((m, (n + 3) // 4 * 4), dtype=np.uint8)
    c[:, :n] = codes
    c = c.reshape(m, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def class_counts(codes, include=None):
    """int64 [m][4]: how many of the included samples carry code 0, 1, 2, 3 at each variant."""
    c = codes if include is None else codes[:, np.asarray(include, dtype=bool)]
    return np.stack([(c == g).sum(axis=1) for g in range(4)], axis=1).astype(np.int64)


def tables(counts, flip, mode):
    """The doubles of k_score_tables: ts (weight columns) and td (dosage sum), float64 [m][4]."""
    counts = np.asarray(counts, dtype=np.int64)
    m = len(counts)
    fl = np.zeros(m, dtype=bool) if flip is None else np.asarray(flip).astype(bool)
    het, hom = counts[:, 1].astype(np.float64), counts[:, 2].astype(np.float64)
    nm = (counts[:, 0] + counts[:, 1] + counts[:, 2]).astype(np.float64)
    ts, td = np.zeros((m, 4)), np.zeros((m, 4))
    ok = nm > 0
    g = np.arange(3.0)
    scored = np.where(fl[:, None], 2.0 - g[None, :], g[None, :])
    with np.errstate(all="ignore"):
        mean = (het + 2.0 * hom) / nm
        if mode == CENTER:
            freq = mean / 2.0
            sd = np.sqrt(2.0 * freq * (1.0 - freq))
            ok = ok & (sd != 0.0)
            mean_scored = np.where(fl, 2.0 - mean, mean)
            ts[ok, :3] = ((scored - mean_scored[:, None]) / sd[:, None])[ok]
        else:
            ts[ok, :3] = scored[ok]
            td[ok, :3] = scored[ok]
            if mode == MEAN_IMPUTE:
                ts[ok, 3] = td[ok, 3] = np.where(fl, 2.0 - mean, mean)[ok]
    return ts, td


class Inputs:
    """One scored list: codes uint8 [m][N] of the listed variants over ALL samples (the contraction runs over all of
    them; a subset only selects which are counted and returned), the include mask, flips and the mode."""

    def __init__(self, codes, flip, mode, include=None):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.m, self.n = self.codes.shape
        self.flip = np.zeros(self.m, dtype=np.uint8) if flip is None else np.asarray(flip, dtype=np.uint8)
        self.mode = mode
        self.include = None if include is None else np.asarray(include, dtype=bool)
        self.counts = class_counts(self.codes, self.include)
        self.ts, self.td = tables(self.counts, self.flip, mode)
        self.code_t = np.ascontiguousarray(self.codes.T, dtype=np.float64)  # [N][m]
        self.miss_t = np.ascontiguousarray((self.codes == 3).T, dtype=np.float64)
        self.load = (self.code_t + self.miss_t).sum(axis=1).astype(np.int64)  # sum_v (c + miss) per sample
        self._parts = {}

    def tab(self, target):
        return self.ts if target == "weight" else self.td

    def parts(self, target):
        """t0, d, x (unfused) and x_fused of the target's table, float64 [m] each."""
        if target not in self._parts:
            tab = self.tab(target)
            t0, d = tab[:, 0], tab[:, 1] - tab[:, 0]
            first = tab[:, 3] - t0
            x = first - 3.0 * d
            x_fused = np.array([float(Fraction(a) - 3 * Fraction(b)) for a, b in zip(first, d)])
            self._parts[target] = (t0, d, x, x_fused)
        return self._parts[target]


def coefficients(inp, w, target="weight", fused=False):
    """alpha, beta and the terms of k0 as the doubles CoefOf computes (w = None: the dosage sum, w = 1)."""
    t0, d, x, x_fused = inp.parts(target)
    w = np.ones(inp.m) if w is None else np.asarray(w, dtype=np.float64)
    return w * d, w * (x_fused if fused else x), w * t0


def split_digits(x, digits, drop_carry=False):
    """Signed base-256 digits of int64 x, least significant first (Digits() of score_i8.hip)."""
    x = np.array(x, dtype=np.int64)
    out = np.empty((len(x), digits), dtype=np.int64)
    for j in range(digits):
        q = ((x + 128) & 255) - 128
        out[:, j] = q
        x = (x >> 8) if drop_carry else ((x - q) >> 8)
    return out


class Column:
    pass


def column_model(inp, w, target="weight", digits=None, rounding="nearest", drop_carry=False, mult_off=None, fused=False):
    """The fixed-point value of one target column.  Mutation parameters: `digits` (default 7, or 5 for the dosage sum),
    `rounding` "nearest" (ties to even) or "truncate", `drop_carry` (no carry out of a negative digit), `mult_off`
    (that digit position counts 256 times too much)."""
    if digits is None:
        digits = WEIGHT_DIGITS if target == "weight" else DOSAGE_DIGITS
    alpha, beta, k0_terms = coefficients(inp, w, target, fused)
    colmax = float(max(np.abs(alpha).max(), np.abs(beta).max()))
    e = math.frexp(colmax)[1] if colmax > 0.0 else 0
    shift = 8 * digits - 2 - e
    rnd = np.rint if rounding == "nearest" else np.trunc
    col = Column()
    col.e, col.digits = e, digits
    col.u = Fraction(2) ** (-shift)
    col.alpha, col.beta = alpha, beta
    # ldexp is exact here: |alpha| 2^shift <= 2^(8 digits - 2), and what underflows rounds to 0 either way
    col.A = rnd(np.ldexp(alpha, shift)).astype(np.int64)
    col.B = rnd(np.ldexp(beta, shift)).astype(np.int64)
    col.a = split_digits(col.A, digits, drop_carry)
    col.b = split_digits(col.B, digits, drop_carry)
    # the digit columns accumulate in integers: sums stay below 2^24, exact in a float64 matrix product
    sums = (inp.code_t @ col.a.astype(np.float64) + inp.miss_t @ col.b.astype(np.float64)).astype(np.int64)
    mult = [256 ** j * (256 if j == mult_off else 1) for j in range(digits)]
    col.k0 = sum((Fraction(float(t)) for t in k0_terms), Fraction(0))
    col.N = [sum(int(v) * mu for v, mu in zip(row, mult)) for row in sums]
    col.F = [col.k0 + n * col.u for n in col.N]
    # an upper bound of every partial sum of the epilogue, in units of u, and of the terms of k0
    col.mass = (inp.code_t @ (np.abs(col.a).astype(np.float64) @ np.array([256.0 ** j for j in range(digits)])) +
                inp.miss_t @ (np.abs(col.b).astype(np.float64) @ np.array([256.0 ** j for j in range(digits)])))
    col.k0_abs = sum((abs(Fraction(float(t))) for t in k0_terms), Fraction(0))
    return col


def _contract(ints, plane_t):
    """sum_v ints[v] * plane[v][s] for Python integers of any size, exactly: 24-bit limbs through float64 products."""
    sign = np.array([1.0 if x >= 0 else -1.0 for x in ints])
    mag = [abs(x) for x in ints]
    n_limbs = max(1, (max(mag).bit_length() + 23) // 24) if mag else 1
    limbs = np.array([[(x >> (24 * k)) & 0xFFFFFF for k in range(n_limbs)] for x in mag], dtype=np.float64)
    part = (plane_t @ (limbs * sign[:, None])).astype(np.int64)
    return [sum(int(v) << (24 * k) for k, v in enumerate(row)) for row in part]


def _exact_tables(inp, target):
    """T0, D = T1 - T0 and X = T3 - T0 - 3 D per variant as Fractions (center mode: 1/sd to 200 bits)."""
    out = []
    for i in range(inp.m):
        c0, het, hom, _ = (int(v) for v in inp.counts[i])
        nm = c0 + het + hom
        fl = bool(inp.flip[i])
        zero = (Fraction(0), Fraction(0), Fraction(0))
        if nm == 0:
            out.append(zero)
            continue
        mean = Fraction(het + 2 * hom, nm)
        if inp.mode == CENTER:
            if target != "weight":
                out.append(zero)
                continue
            var = mean * (1 - mean / 2)  # 2 f (1 - f), f = mean / 2
            if var == 0:
                out.append(zero)
                continue
            inv_sd = Fraction(math.isqrt((var.denominator << 400) // var.numerator), 1 << 200)
            mean_scored = 2 - mean if fl else mean
            t0 = ((2 if fl else 0) - mean_scored) * inv_sd
            d = (-1 if fl else 1) * inv_sd
            out.append((t0, d, -t0 - 3 * d))
        else:
            t0, d = Fraction(2 if fl else 0), Fraction(-1 if fl else 1)
            t3 = Fraction(0) if inp.mode == NO_MEAN_IMPUTATION else (2 - mean if fl else mean)
            out.append((t0, d, t3 - t0 - 3 * d))
    return out


def true_sum(inp, w, u, target="weight"):
    """E[s] = sum_v w_v T_v[g(v, s)] over the reals, to within (load[s] + 1) 2^-64 u / 2 (the coefficients are kept
    to 2^-64 u; `allowance` carries that term)."""
    ws = [Fraction(1)] * inp.m if w is None else [Fraction(float(x)) for x in w]
    scale = Fraction(2) ** E_BITS / u
    a_int, b_int, k0 = [], [], Fraction(0)
    for wv, (t0, d, x) in zip(ws, _exact_tables(inp, target)):
        a_int.append(round(wv * d * scale))
        b_int.append(round(wv * x * scale))
        k0 += wv * t0
    code = _contract(a_int, inp.code_t)
    miss = _contract(b_int, inp.miss_t)
    return [k0 + Fraction(c + b) / scale for c, b in zip(code, miss)]


def k0_depth(m):
    """Roundings a term of k0 can pass through in k_i8_ranges: six butterfly steps of its wave, two adds across the four
    waves, one atomic add per 256-variant block (blocks = ceil(m / 256) <= 1024: a thread holds at most one term)."""
    assert m <= 256 * 1024
    return 6 + 2 + (m + 255) // 256


def slices(m):
    """Slices of LaunchI8 at test size: an even tile count, 16 tiles per slice -- the minimum, which LaunchI8 applies
    before (and instead of) PGH_I8_TPS_MAX whenever the chip-filling share of a slice is below it, as it is for any
    list of fewer than some 10,000 tiles over a few sample groups."""
    n_tiles = ((m + 63) // 64 + 1) & ~1
    return (n_tiles + 15) // 16


def allowance(inp, w, col, target="weight"):
    """(Q, R) per sample, as Fractions, of  |device - E| <= Q + R.

    Q = (u / 2) sum_v (c + miss): one rounding of A_v and one of B_v, each at most u / 2 per unit of operand.

    R, the floating-point allowance, term by term (eps = 2^-53; g = GAMMA covers the compounding of up to 64 roundings):
      * table entries (k_score_tables).  Outside center mode t0, t1 are 0, 1, 2 exactly and only t3 = the mean (one
        division, and 2 - mean when flipped) is rounded: |dt3| <= 2 g; x = (t3 - t0) - 3 d then costs two roundings of
        values below 3: |dx| <= 7 g (0 without imputation, where x = -3 d exactly).  In center mode: mean (1 rounding),
        om = 1 - f (|dom| <= g (f + om)), var = 2 f om (relative g (3 + f / om)), sd (half of that + g),
        num_g = scored - mean_scored (|dnum| <= 2 g + g |num|), t_g = num_g / sd:
        |dt_g| <= |t_g| (rel_sd + g) + dnum_g / sd;  d = t1 - t0: dd = dt0 + dt1 + g |d|;
        x = (0 - t0) - 3 d: dx = dt0 + 3 dd + 3 g |d| + g |x|.
      * the two coefficient products: d_alpha = |w| dd + g |w d|, d_beta = |w| dx + g |w x|, each multiplied by the
        operand it meets: sum_v (d_alpha_v c + d_beta_v miss).
      * k0: d_k_v = |w| dt0 + g |w t0| per term, and k0_depth(m) roundings of partial sums that are each at most
        sum |w t0| (k_i8_ranges: butterfly, four waves, one atomic per block).
      * the epilogue.  A digit lane's value mult * int32 is exact.  Per slice: three gated shuffle additions, a second
        atomic where a column's digits straddle two tiles, and the atomic additions themselves -- at most five roundings
        per slice -- then one addition of k0: (5 slices + 1) roundings of values that never exceed
        M = MASS sum_v ((|alpha_v| + u) c + (|beta_v| + u) miss) + |k0|.
      * true_sum's own resolution: (load + 1) 2^-64 u.
    """
    g = float(GAMMA)
    wabs = np.ones(inp.m) if w is None else np.abs(np.asarray(w, dtype=np.float64))
    t0, d, x, _ = inp.parts(target)
    tab = inp.tab(target)
    zeros = np.zeros(inp.m)
    if inp.mode == NO_MEAN_IMPUTATION:
        dt0, dd, dx = zeros, zeros, zeros
    elif inp.mode == MEAN_IMPUTE:
        dt0, dd, dx = zeros, zeros, np.where(np.abs(tab).sum(axis=1) > 0, 7.0 * g, 0.0)
    else:
        live = np.abs(tab).sum(axis=1) > 0
        nm = np.maximum(inp.counts[:, :3].sum(axis=1), 1).astype(np.float64)
        mean = (inp.counts[:, 1] + 2.0 * inp.counts[:, 2]) / nm
        f = np.where(live, mean / 2.0, 0.5)
        om = 1.0 - f
        sd = np.sqrt(2.0 * f * om)
        rel_sd = g * (3.0 + f / om) / 2.0 + g
        dt = []
        for k in (0, 1):
            num = np.abs(tab[:, k]) * sd
            dt.append(np.abs(tab[:, k]) * (rel_sd + g) + (2.0 * g + g * num) / sd)
        dt0 = np.where(live, dt[0], 0.0)
        dd = np.where(live, dt[0] + dt[1] + g * np.abs(d), 0.0)
        dx = np.where(live, dt[0] + 3.0 * dd + 3.0 * g * np.abs(d) + g * np.abs(x), 0.0)
    d_alpha = wabs * dd + g * wabs * np.abs(d)
    d_beta = wabs * dx + g * wabs * np.abs(x)
    d_k0 = float((wabs * dt0 + g * wabs * np.abs(t0)).sum()) + k0_depth(inp.m) * g * float((wabs * np.abs(t0)).sum())
    u = float(col.u)
    big = float(MASS) * (inp.code_t @ (wabs * np.abs(d) + u) + inp.miss_t @ (wabs * np.abs(x) + u)) + float(col.k0_abs)
    r = inp.code_t @ d_alpha + inp.miss_t @ d_beta + d_k0 + (5 * slices(inp.m) + 1) * g * big
    res = Fraction(1, 2 ** E_BITS) * col.u
    Q = [int(ld) * col.u / 2 for ld in inp.load]
    R = [Fraction(float(rv)) + (int(ld) + 1) * res for rv, ld in zip(r, inp.load)]
    return Q, R
