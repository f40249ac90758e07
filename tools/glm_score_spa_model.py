#!/usr/bin/env python3
"""A numpy model of GlmScoreSpaKernel's arithmetic in the kernel's accumulation order, run on the CPU against the
oracle (tests/glm_spa_oracle.py) on the inputs of the parity test of tests/test_glm_score_sparse_spa.py.  It is where
that test's tolerance comes from (pgh_glm_score_sparse_spa): 100 x the worst relative
difference of p_spa printed here.

The model follows the device: mu recovered from r, t and V from the Cholesky factor of [[H_N, c], [c', A]] with d = x - b
for the row's base code, gt = d - Zt t as a chain over the covariates, V_rest = V - V_E, every sum over E as one chain
per lane at the team's stride, a butterfly over the 64 lanes and the waves in order, one exp of -|gt s| per entry and
tail, and the safeguarded Newton iteration with its 64 evaluations.  A multiply and an add stand where the kernel has an
fma.

usage: python tools/glm_score_spa_model.py [--widths]
--widths: the inputs of the test's width cases instead (its MODEL_WORST_WIDTHS)."""

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import glm_score_oracle as O  # noqa: E402
import glm_spa_oracle as S  # noqa: E402

LONG = 1024
MAX_EVAL = 64
STOP = 1e-12
ULPS = 2.0 ** -50


def team_sum(v, team):
    """One chain per lane at the team's stride, a butterfly per wave, the waves in order."""
    lanes = np.zeros(team)
    for j in range(0, len(v), team):
        part = v[j:j + team]
        lanes[:len(part)] += part
    waves = []
    for w0 in range(0, team, 64):
        x = lanes[w0:w0 + 64].copy()
        off = 32
        while off:
            x = x + x[np.arange(64) ^ off]
            off >>= 1
        waves.append(x[0])
    s = waves[0]
    for w in waves[1:]:
        s += w
    return float(s)


def pi_q(x, mu):
    a = np.exp(-np.abs(x))
    nu = 1.0 - mu
    num_p = np.where(x > 0, mu, mu * a)
    num_q = np.where(x > 0, nu * a, nu)
    inv = 1.0 / (num_p + num_q)
    return num_p * inv, num_q * inv


def k_term(x, mu):
    m = np.where(x > 0, 1.0 - mu, mu)
    return np.where(x > 0, x, 0.0) + np.log1p(m * np.expm1(-np.abs(x))) - mu * x


class Root:
    def __init__(self, q, v):
        self.u, self.lo, self.hi, self.grow, self.done = q / v, 0.0, math.inf, 1.0 / math.sqrt(v), False

    def step(self, f, fp, q, tol):
        if self.done:
            return True
        if not math.isfinite(f) or not math.isfinite(fp):
            return False
        if f < q:
            self.lo = self.u
        else:
            self.hi = self.u
        with np.errstate(all="ignore"):
            un = self.u + float(np.float64(q - f) / np.float64(fp))
        if self.hi == math.inf:
            if not un <= self.u + self.grow:
                un = self.u + self.grow
                self.grow *= 2.0
        elif not (self.lo <= un <= self.hi):
            un = 0.5 * (self.lo + self.hi)
        self.done = abs(un - self.u) <= max(tol, ULPS * self.u) or self.hi - self.lo <= tol
        self.u = un
        return True


def tail(u, q, kk, k2):
    rad = 2.0 * (u * q - kk)
    if not rad > 0 or not k2 > 0:
        return math.nan
    om = math.sqrt(rad)
    ratio = u * math.sqrt(k2) / om
    if not ratio > 0 or not math.isfinite(ratio):
        return math.nan
    return 0.5 * math.erfc(abs(om + math.log(ratio) / om) * 0.70710678118654752440)


def phase_b(g, mu, q, v, v_rest, team):
    """(p_spa, evaluations) from a team's stash of (g, mu) pairs as the device computes them; p_spa None: state 2."""
    tol = STOP / math.sqrt(v)
    ra, rb = Root(q, v), Root(q, v)
    ok, evals = True, 0
    while ok and evals < MAX_EVAL and not (ra.done and rb.done):
        pa, qa = pi_q(g * ra.u, mu)
        pb, qb = pi_q(-g * rb.u, mu)
        s0, s1 = team_sum(g * (pa - mu), team), team_sum(g * g * (pa * qa), team)
        s2, s3 = team_sum(g * (pb - mu), team), team_sum(g * g * (pb * qb), team)
        evals += 1
        ok = ra.step(v_rest * ra.u + s0, s1 + v_rest, q, tol) and rb.step(v_rest * rb.u - s2, s3 + v_rest, q, tol)
    if not (ok and ra.done and rb.done):
        return None, evals
    total = 0.0
    for uu, sg in ((ra.u, 1.0), (rb.u, -1.0)):
        pa, qa = pi_q(sg * g * uu, mu)
        kk = team_sum(k_term(sg * g * uu, mu), team) + 0.5 * v_rest * uu * uu
        total += tail(uu, q, kk, team_sum(g * g * (pa * qa), team) + v_rest)
    if not math.isfinite(total):
        return None, evals
    return total, evals


def model_row(codes, nul, base, dense_form, cutoff):
    """(p, p_spa, state, evaluations) of a FITTED row as the device computes them."""
    b = 0 if (dense_form or base == 3) else base
    use = (codes != 3) & nul.in_s
    zt, w, r = nul.zt[use], nul.w[use], nul.r[use]
    d = codes[use].astype(np.float64) - b
    k1 = zt.shape[1]
    a = np.zeros((k1 + 1, k1 + 1))
    a[:k1, :k1] = (zt * w[:, None]).T @ zt
    a[k1, :k1] = a[:k1, k1] = (w * d) @ zt
    a[k1, k1] = (w * d) @ d
    low = np.linalg.cholesky(a)
    f = np.linalg.solve(low[:k1, :k1], zt.T @ r)
    u = float(d @ r - low[k1, :k1] @ f)
    lxx = float(low[k1, k1])
    v = lxx * lxx
    stat = u / lxx
    p = math.erfc(abs(stat) * 0.70710678118654752440)
    if not abs(stat) > cutoff:
        return p, p, 0, 0
    t = np.linalg.solve(low[:k1, :k1].T, low[k1, :k1])
    in_e = S.entry_mask(codes, base, dense_form)[use]
    team = 256 if (dense_form or int((codes != base).sum()) > LONG) else 64
    g = d[in_e] - t[0]
    for j in range(1, k1):
        g = g - zt[in_e, j] * t[j]
    ri = r[in_e]
    mu = np.where(ri > 0, 1.0 - ri, -ri)
    v_e = team_sum(w[in_e] * g * g, team)
    v_rest = 0.0 if (base == 3 and not dense_form) else max(v - v_e, 0.0)
    total, evals = phase_b(g, mu, abs(u), v, v_rest, team)
    if total is None:
        return p, p, 2, evals
    return p, total, 1, evals


def main():
    import test_glm_score_sparse_spa as T

    widths = "--widths" in sys.argv[1:]
    worst_all, evals_all = 0.0, []
    for n in (T.WIDTHS_N,) if widths else T.PARITY_N:
        case = T.ParityInputs(n)
        for k in T.WIDTHS if widths else T.PARITY_K:
            y, Z = case.y, case.covariates(k)
            nul = O.Null(y, Z)
            assert nul.status is None
            for max_minor in (0, n) if widths else (0, 1, n):
                worst, applied, differ, failed, kinds = 0.0, 0, 0, 0, set()
                for i in T.WIDTHS_ROWS if widths else range(len(case.geno)):
                    base, dense_form = S.row_form(case.geno[i], max_minor)
                    row, p_spa, state = S.spa_row(case.x[i], case.geno[i], nul, base, dense_form, T.CUTOFF)
                    if row["errcode"] is not None:
                        continue
                    p, mp, mstate, evals = model_row(case.geno[i], nul, base, dense_form, T.CUTOFF)
                    assert mstate == state, (n, k, max_minor, i, base, dense_form, state, mstate, evals, row)
                    if state == 1:
                        worst = max(worst, abs(mp - p_spa) / p_spa)
                        applied += 1
                        differ += not 0.5 <= p_spa / row["p"] <= 2
                        evals_all.append(evals)
                        kinds.add((base, dense_form))
                    failed += state == 2
                print(f"n={n} k={k} max_minor={max_minor}: {applied} applied, {differ} beyond 2x, {failed} failed, "
                      f"worst {worst:.3g}, forms {sorted(kinds)}", flush=True)
                worst_all = max(worst_all, worst)
    print(f"worst relative difference of p_spa: {worst_all:.3g}; evaluations per applied row: mean "
          f"{np.mean(evals_all):.2f}, max {max(evals_all)}")
    if widths:
        return
    # the long-row test's inputs: its dense-form rows of more than 10,000 entries
    case = T.long_inputs()
    nul = O.Null(case.y, case.covariates(T.LONG_K))
    worst, applied, evals_long = 0.0, 0, []
    for i in range(len(case.geno)):
        base, dense_form = S.row_form(case.geno[i], 1)
        if not dense_form or S.entry_mask(case.geno[i], base, dense_form).sum() <= 10_000:
            continue
        row, p_spa, state = S.spa_row(case.x[i], case.geno[i], nul, base, dense_form, T.CUTOFF)
        if row["errcode"] is not None:
            continue
        p, mp, mstate, evals = model_row(case.geno[i], nul, base, dense_form, T.CUTOFF)
        assert mstate == state, (i, base, dense_form, state, mstate, evals, row)
        if state == 1:
            worst = max(worst, abs(mp - p_spa) / p_spa)
            applied += 1
            evals_long.append(evals)
    print(f"long rows (n={T.LONG_N}, k={T.LONG_K}, max_minor=1): {applied} applied, worst {worst:.3g}, evaluations mean "
          f"{np.mean(evals_long):.2f}, max {max(evals_long)}")


if __name__ == "__main__":
    main()
