#!/usr/bin/env python3
"""A numpy model of GlmScoreDenseSpaKernel's arithmetic in the kernel's accumulation order, run on the CPU against the
oracle (tests/glm_spa_oracle.py) on the inputs of the parity test of tests/test_glm_score_multi_spa.py.  It is where
that test's tolerance comes from (pgh_glm_score_multi_spa): 100 x the worst relative difference
of p_spa printed here.

The model follows the device: t, U and V from the Cholesky factor of [[H_N, c], [c', A]] with d = x; b = 2 when the
hom-alt calls among N outnumber the hom-ref ones, otherwise 0; E = the samples of N with x != b; gt = x - Zt t as a
chain over the covariates; mu recovered from r; V_E as one chain per thread over the entries of its 16-code words
(thread = word mod 256), a butterfly over the 64 lanes and the waves in order; V_rest = max(V - V_E, 0); and phase B
over the stash in sample order with the workgroup as the team, which is tools/glm_score_spa_model.py's phase_b.  A
multiply and an add stand where the kernel has an fma.

usage: python tools/glm_score_dense_spa_model.py [--widths]
--widths: the inputs of the test's width and sample-count cases instead (its MODEL_WORST_WIDTHS)."""

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_score_oracle as O  # noqa: E402
import glm_spa_oracle as S  # noqa: E402
import glm_score_spa_model as M  # noqa: E402

TEAM = 256


def dense_base(codes, in_s):
    """The dense route's b: 2 when the hom-alt calls among N outnumber the hom-ref ones, otherwise 0."""
    c = np.bincount(codes[in_s], minlength=4)
    return 2 if c[2] > c[0] else 0


def word_sum(v, sample):
    """One chain per thread over the entries of its words in sample order, then the team's reduction."""
    lanes = np.zeros(TEAM)
    for x, s in zip(v, sample):
        lanes[(s >> 4) % TEAM] += x
    return M.team_sum(lanes, TEAM)


def model_row(codes, nul, cutoff):
    """(p, p_spa, state, evaluations) of a FITTED row as the device computes them."""
    use = (codes != 3) & nul.in_s
    zt, w, r = nul.zt[use], nul.w[use], nul.r[use]
    d = codes[use].astype(np.float64)
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
    in_e = d != dense_base(codes, nul.in_s)
    g = d[in_e] - t[0]
    for j in range(1, k1):
        g = g - zt[in_e, j] * t[j]
    ri = r[in_e]
    mu = np.where(ri > 0, 1.0 - ri, -ri)
    v_e = word_sum(w[in_e] * g * g, np.flatnonzero(use)[in_e])
    total, evals = M.phase_b(g, mu, abs(u), v, max(v - v_e, 0.0), TEAM)
    if total is None:
        return p, p, 2, evals
    return p, total, 1, evals


def run(cases):
    """cases: (n, k, row stride).  Prints a line per phenotype; returns (worst, evaluations)."""
    import test_glm_score_multi_spa as T

    worst_all, evals_all = 0.0, []
    for n, k, stride in cases:
        case = T.inputs(n)
        Y = T.phenotypes(case)
        Z = case.covariates(k)
        for p, y in enumerate(Y):
            nul = O.Null(y, Z)
            assert nul.status is None
            worst, applied, differ, failed, b2 = 0.0, 0, 0, 0, 0
            for i in range(0, len(case.geno), stride):
                b = dense_base(case.geno[i], nul.in_s)
                row, p_spa, state = S.spa_row(case.x[i], case.geno[i], nul, b, False, T.CUTOFF)
                if row["errcode"] is not None:
                    continue
                _, mp, mstate, evals = model_row(case.geno[i], nul, T.CUTOFF)
                assert mstate == state, (n, k, p, i, b, state, mstate, evals, row)
                if state == 1:
                    worst = max(worst, abs(mp - p_spa) / p_spa)
                    applied += 1
                    b2 += b == 2
                    differ += not 0.5 <= p_spa / row["p"] <= 2
                    evals_all.append(evals)
                failed += state == 2
            print(f"n={n} k={k} phenotype {p}: {applied} applied ({b2} with b = 2), {differ} beyond 2x, {failed} failed, "
                  f"worst {worst:.3g}", flush=True)
            worst_all = max(worst_all, worst)
    return worst_all, evals_all


def main():
    import test_glm_score_multi_spa as T

    if "--widths" in sys.argv[1:]:
        # the inputs of test_every_instantiated_width and test_sample_count_edges, on the rows they check
        cases = [(T.WIDTHS_N, k, T.WIDTHS_STRIDE) for k in T.WIDTHS] + [(n, T.EDGE_K, stride) for n, stride in T.EDGES]
    else:
        cases = [(n, k, 1) for n in T.PARITY_N for k in T.PARITY_K]
    worst_all, evals_all = run(cases)
    print(f"worst relative difference of p_spa: {worst_all:.3g}; evaluations per applied row: mean "
          f"{np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
