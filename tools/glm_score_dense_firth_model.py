#!/usr/bin/env python3
"""A numpy model of GlmScoreDenseFirthKernel's arithmetic in the kernel's accumulation order, run on the CPU against the
oracle (tests/glm_firth_oracle.py) on the inputs of the parity test of tests/test_glm_score_multi_firth.py.  It is where
that test's tolerance comes from (pgh_glm_score_multi_firth): 100 x the worst difference printed
here, over |delta beta| / se, |delta se| / se and |delta p| / p of the applied rows.

The model follows the device: E = the samples of N with a code of 1 or 2 in sample order; mu recovered from r; G as one
chain per thread over the entries of its 16-code words (thread = word mod 256), a butterfly over the 64 lanes and the
waves in order; and per evaluation pi, 1 - pi and K from one exp of -|x beta| per entry (expm1 and log1p of it for K),
five chains per thread over the stash at the workgroup's stride and the same reduction, then the safeguarded Newton
step with its 64 evaluations.  A multiply and an add stand where the kernel has an fma.  Which rows are applied is the
oracle's decision (it refuses a |stat| within 1e-6 of the cutoff).

usage: python tools/glm_score_dense_firth_model.py [--widths]
--widths: the inputs of the test's width and sample-count cases instead (its MODEL_WORST_WIDTHS)."""

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_score_oracle as O  # noqa: E402
import glm_firth_oracle as F  # noqa: E402
import glm_score_spa_model as M  # noqa: E402
from glm_score_dense_spa_model import TEAM, word_sum  # noqa: E402


def phase_b(x, mu, g, TEAM=TEAM):
    """(beta, se, p, evaluations) from the team's stash of (x, mu) pairs as the device computes them (TEAM: its
    threads, the workgroup's here; tools/glm_score_sparse_firth_model.py also has a wave's 64); beta None: state 2."""
    sgn, u, lo, hi, grow, tol, l0 = 0.0, 0.0, 0.0, math.inf, 0.0, 0.0, 0.0
    for ev in range(1, F.MAX_EVAL + 1):
        beta = sgn * u
        pi, qi = M.pi_q(x * beta, mu)
        v = pi * qi
        xx = x * x
        k0 = M.team_sum(M.k_term(x * beta, mu), TEAM)
        k1 = M.team_sum(x * (pi - mu), TEAM)
        k2 = M.team_sum(xx * v, TEAM)
        k3 = M.team_sum((xx * x) * (v * (qi - pi)), TEAM)
        k4 = M.team_sum((xx * xx) * (v * (1.0 - 6.0 * v)), TEAM)
        if not k2 > 0:
            return None, None, None, ev
        r3 = k3 / k2
        ls = beta * g - k0 + 0.5 * math.log(k2)
        f = g - k1 + 0.5 * r3
        h = k2 - 0.5 * (k4 / k2 - r3 * r3)
        h = h if h > 0 else k2
        if not (math.isfinite(ls) and math.isfinite(f) and math.isfinite(h)):
            return None, None, None, ev
        if ev == 1:
            sgn, l0 = (1.0 if f > 0 else -1.0), ls
            grow = 1.0 / math.sqrt(k2)
            tol = F.STOP * grow
        fs = sgn * f
        done = fs == 0.0
        if not done:
            if fs > 0:
                lo = u
            else:
                hi = u
            un = u + fs / h
            if hi == math.inf:
                if not un <= u + grow:
                    un = u + grow
                    grow *= 2.0
            elif not lo <= un <= hi:
                un = 0.5 * (lo + hi)
            d = abs(un - u)
            done = d <= tol or hi - lo <= tol or d <= F.ULPS * u
        if done:
            dev = max(2.0 * (ls - l0), 0.0)
            return beta, 1.0 / math.sqrt(k2), math.erfc(math.sqrt(dev) * 0.70710678118654752440), ev
        u = un
    return None, None, None, F.MAX_EVAL


def model_row(codes, nul):
    """(beta, se, p, evaluations) of an APPLIED row as the device computes them."""
    in_e = (codes != 3) & (codes != 0) & nul.in_s
    x = codes[in_e].astype(np.float64)
    r = nul.r[in_e]
    mu = np.where(r > 0, 1.0 - r, -r)
    g = word_sum(x * r, np.flatnonzero(in_e))
    return phase_b(x, mu, g)


def run(cases):
    """cases: (n, k, row stride).  Prints a line per phenotype; returns (worst, evaluations)."""
    import test_glm_score_multi_firth as T

    worst_all, evals_all = 0.0, []
    for n, k, stride in cases:
        case = T.inputs(n)
        Y = T.phenotypes(case)
        Z = case.covariates(k)
        for p, y in enumerate(Y):
            nul = O.Null(y, Z)
            assert nul.status is None
            worst, applied, failed, separated, flipped = [0.0, 0.0, 0.0], 0, 0, 0, 0
            for i in range(0, len(case.geno), stride):
                row, beta, se, pv, state, info = F.firth_row(case.x[i], case.geno[i], nul, T.CUTOFF)
                if state == 0:
                    continue
                mb, mse, mp, evals = model_row(case.geno[i], nul)
                assert (mb is None) == (state == 2), (n, k, p, i, state, mb, evals, row)
                failed += state == 2
                if state == 1:
                    worst = [max(a, b) for a, b in zip(worst, (abs(mb - beta) / se, abs(mse - se) / se, abs(mp - pv) / pv))]
                    applied += 1
                    separated += info["separated"]
                    flipped += beta * row["beta"] < 0
                    evals_all.append(evals)
            print(f"n={n} k={k} phenotype {p}: {applied} applied ({separated} separated, {flipped} of the other sign), "
                  f"{failed} failed, worst beta {worst[0]:.3g} se {worst[1]:.3g} p {worst[2]:.3g}", flush=True)
            worst_all = max(worst_all, *worst)
    return worst_all, evals_all


def main():
    import test_glm_score_multi_firth as T

    if "--widths" in sys.argv[1:]:
        # the inputs of test_every_instantiated_width and test_sample_count_edges, on the rows they check
        cases = [(T.WIDTHS_N, k, T.WIDTHS_STRIDE) for k in T.WIDTHS] + [(n, T.EDGE_K, stride) for n, stride in T.EDGES]
    else:
        cases = [(n, k, 1) for n in T.PARITY_N for k in T.PARITY_K]
    worst_all, evals_all = run(cases)
    print(f"worst difference over |delta beta| / se, |delta se| / se, |delta p| / p: {worst_all:.3g}; evaluations per "
          f"applied row: mean {np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
