"""FP64 numpy oracle of pgh_glm_score_sparse_spa: the saddlepoint p-value of the logistic score test.

The rules are the header's (include/pgenhip.h); the numbers are computed another way than the device computes them.
N and x come from the dense calls; gt is the Householder-QR residual of x on the covariates (glm_score_oracle's
route), not d - Zt t from a Cholesky factor; mu is the sigmoid of the oracle's own null fit, not 1 - r; V_rest is summed
over the samples outside E, not V - V_E; K is written with logaddexp; the root of K'(s) = q comes from bisection to the
last bit, not from Newton steps; and p from math.erfc.  Whether a root exists when V_rest = 0 is decided from the
support of the score.  The base code and the form a dataset holds a row in are inputs: they make E."""

import math

import numpy as np

import glm_score_oracle as O

NAN = float("nan")
UNDECIDED = 1e-6  # how near a support bound (in sqrt V) or the cutoff a case may lie before the contract stops deciding


def row_form(codes, max_minor):
    """(base code, held in the dense form) of a row of codes under Dataset.open(sparse=True, max_minor=...): the
    majority code (ties: the lower one); sparse iff its m entries are at most max_minor, or with max_minor = 0 iff
    they take fewer bytes than the dense row (4 m < pitch)."""
    counts = np.bincount(codes, minlength=4)
    m = int(len(codes) - counts.max())
    if max_minor == 0:
        record = (len(codes) + 3) // 4
        align = 128 if record >= 512 else 16
        return int(counts.argmax()), not 4 * m < max((record + align - 1) // align * align, align)
    return int(counts.argmax()), m > max_minor


def entry_mask(codes, base, dense_form):
    """The samples a row holds as called entries: a dense-form row counts as a base-0 row."""
    b = 0 if dense_form else base
    return (codes != 3) & (codes != b) if b != 3 else codes != 3


class Cgf:
    """K, K', K'' of one row.  g, mu, w: over E.  v_rest: the normal term."""

    def __init__(self, g, mu, v_rest):
        self.g, self.mu, self.v_rest = g, mu, v_rest
        self.lm, self.l1m = np.log(mu), np.log1p(-mu)

    def pi(self, s):
        a = self.lm - self.l1m + self.g * s  # logit
        e = np.exp(-np.abs(a))
        return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))

    def k0(self, s):
        return float(np.sum(np.logaddexp(self.l1m, self.lm + self.g * s) - s * self.mu * self.g)) + 0.5 * self.v_rest * s * s

    def k1(self, s):
        return float(np.sum(self.g * (self.pi(s) - self.mu))) + self.v_rest * s

    def k2(self, s):
        p = self.pi(s)
        # 1 - pi without cancellation: pi of the mirrored logit
        a = self.lm - self.l1m + self.g * s
        e = np.exp(-np.abs(a))
        q = np.where(a >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        return float(np.sum(self.g * self.g * p * q)) + self.v_rest

    def support(self):
        """(min, max) of sum_E g (Y - mu) over Y in {0, 1}^E."""
        hi = np.maximum(self.g * (1 - self.mu), -self.g * self.mu)
        lo = np.minimum(self.g * (1 - self.mu), -self.g * self.mu)
        return float(lo.sum()), float(hi.sum())

    def root(self, q, v):
        """The root of K'(s) = q by bisection, or None when there is none (v_rest == 0, q outside the support)."""
        sv = math.sqrt(v)
        if self.v_rest == 0.0:
            lo, hi = self.support()
            bound = hi if q > 0 else lo
            assert abs(q - bound) > UNDECIDED * sv, ("q is too near the support bound to decide", q, bound)
            if not lo < q < hi:
                return None
        sign = 1.0 if q > 0 else -1.0
        a, b = 0.0, 1.0 / sv
        for _ in range(60):
            if sign * (self.k1(sign * b) - q) >= 0:
                break
            a, b = b, 2 * b
        else:
            raise AssertionError(("no bracket within 2^60 / sqrt V: not a case the contract decides", q, self.v_rest))
        while True:
            m = 0.5 * (a + b)
            if m == a or m == b:
                return sign * m
            if sign * (self.k1(sign * m) - q) >= 0:
                b = m
            else:
                a = m

    def tail(self, q, v):
        s = self.root(q, v)
        if s is None:
            return None
        rad = 2.0 * (s * q - self.k0(s))
        k2 = self.k2(s)
        if not rad > 0 or not k2 > 0:
            return None
        om = math.copysign(math.sqrt(rad), s)
        nu = s * math.sqrt(k2)
        if not nu / om > 0 or not math.isfinite(nu / om):
            return None
        return 0.5 * math.erfc(abs(om + math.log(nu / om) / om) / math.sqrt(2.0))


def cgf_of(x, codes, nul, base, dense_form):
    """(Cgf, U, V) of a fitted row.  x: values with -9 = missing; codes: the row's codes."""
    use = (x != -9.0) & nul.in_s
    xs, w, r, zt = x[use], nul.w[use], nul.r[use], nul.zt[use]
    sw = np.sqrt(w)
    qq, rr = np.linalg.qr(zt * sw[:, None])
    g = xs - zt @ np.linalg.solve(rr, qq.T @ (sw * xs))
    mu = 1.0 / (1.0 + np.exp(-(zt @ nul.beta)))
    in_e = entry_mask(codes, base, dense_form)[use]
    v = float(np.sum(w * g * g))
    v_rest = 0.0 if (base == 3 and not dense_form) else float(np.sum(w[~in_e] * g[~in_e] ** 2))
    return Cgf(g[in_e], mu[in_e], v_rest), float(g @ r), v


def spa_row(x, codes, nul, base, dense_form, cutoff):
    """(row, p_spa, state) of one variant: the row is glm_score_oracle's."""
    row = O.oracle_row(x, nul)
    if row["errcode"] is not None:
        return row, NAN, 0
    assert abs(abs(row["stat"]) - cutoff) > UNDECIDED, ("|stat| is too near the cutoff to decide", row["stat"])
    if not abs(row["stat"]) > cutoff:
        return row, row["p"], 0
    cgf, u, v = cgf_of(x, codes, nul, base, dense_form)
    tails = [cgf.tail(q, v) for q in (abs(u), -abs(u))]
    if any(t is None for t in tails) or not math.isfinite(sum(tails)):
        return row, row["p"], 2
    return row, sum(tails), 1


def check_spa(got, xs, codes, nul, max_minor, cutoff, tol, idx=None):
    """got: Dataset.glm_score_sparse_spa's dict; xs / codes: a value row (-9 = missing) and a code row per variant (the
    codes of ALL raw samples decide the form; with a subset pass the form through `max_minor` as a list of (base,
    dense_form)).  Asserts the states, p_spa within tol (relative) in state 1 and bit-equal to p otherwise.  Returns
    a dict of what it saw."""
    seen = dict(applied=0, failed=0, differ=0, worst=0.0, rows=[])
    for i in (range(len(xs)) if idx is None else idx):
        base, dense_form = max_minor[i] if isinstance(max_minor, list) else row_form(codes[i], max_minor)
        row, p_spa, state = spa_row(xs[i], codes[i], nul, base, dense_form, cutoff)
        ctx = (i, base, dense_form, state, p_spa, row, got["p_spa"][i], got["spa_state"][i], got["p"][i])
        assert got["errcode"][i] == row["errcode"], ctx
        assert got["spa_state"][i] == state, ctx
        if row["errcode"] is not None:
            assert math.isnan(got["p_spa"][i]), ctx
            continue
        if state != 1:
            assert got["p_spa"][i] == got["p"][i], ctx
            seen["failed"] += state == 2
            continue
        diff = abs(got["p_spa"][i] - p_spa) / p_spa if p_spa > 0 else float(got["p_spa"][i] != 0)
        seen["worst"] = max(seen["worst"], diff)
        assert diff <= tol, (diff, ctx)
        seen["applied"] += 1
        seen["differ"] += not 0.5 <= p_spa / row["p"] <= 2.0
        seen["rows"].append((i, base, dense_form, int(entry_mask(codes[i], base, dense_form).sum())))
    return seen


def enriched_matrix(geno, y, rng, factor=5.0):
    """Every fourth hom-ref-majority variant gets ALT calls among the cases at `factor` x its het rate (at least
    2 / n)."""
    geno = geno.copy()
    n = geno.shape[1]
    cases = np.flatnonzero(y == 1.0)
    ref = [v for v in range(len(geno)) if np.bincount(geno[v], minlength=4).argmax() == 0]
    for v in ref[::4]:
        rate = max(factor * float((geno[v] == 1).mean()), 2.0 / n)
        hit = cases[rng.random(len(cases)) < rate]
        geno[v, hit] = 1
    return geno
