#!/usr/bin/env python3
"""A numpy model of pgh_glm_score_sparse_multi_spa's arithmetic in the route's accumulation order, run on the CPU against
the oracle (tests/glm_spa_oracle.py) on the inputs of the parity test of tests/test_glm_score_sparse_multi_spa.py.  It is
where that test's tolerance comes from (pgh_glm_score_sparse_multi_spa): 100 x the worst
relative difference of p_spa printed here.

The model follows the device.  U0, A and c of a (row, phenotype) are the many-phenotype entry kernel's sums: the row's
entries (a dense-form row's samples) in consecutive segments of 1,024, each segment one chain in entry order, the
segments added in ascending order, with the covariates centred per entry on the phenotype's own pattern means.  t, U
and V come from the Cholesky factor of [[H_N, c], [c', A]].  Then the saddlepoint kernel's team sums, which are
tools/glm_score_spa_model.py's: gt = d - Zt t as a chain over the covariates, mu recovered from r, V_E as one chain per
lane at the team's stride, a butterfly over the 64 lanes and the waves in order, V_rest = V - V_E, and its phase_b.  A
multiply and an add stand where the kernels have an fma.

usage: python tools/glm_score_sparse_multi_spa_model.py [--widths]
--widths: the inputs of the test's width cases instead (its MODEL_WORST_WIDTHS)."""

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_spa_oracle as S  # noqa: E402
import glm_score_spa_model as M  # noqa: E402

SEG = M.LONG  # kGlmSparseLong: the entries of one segment, and the longest row of the wave form


def segment_sum(v, at):
    """v[i] joins the chain of segment at[i] // SEG in order; the segments' chains are added in ascending order."""
    total = 0.0
    for seg in np.unique(at // SEG):
        part = v[at // SEG == seg]
        total = total + (float(np.cumsum(part)[-1]) if len(part) else 0.0)
    return total


def model_row(codes, nul, base, dense_form, cutoff):
    """(p, p_spa, state, evaluations) of a FITTED row as the device computes them."""
    b = 0 if (dense_form or base == 3) else base
    use = (codes != 3) & nul.in_s
    zt, w, r = nul.zt[use], nul.w[use], nul.r[use]
    d = codes[use].astype(np.float64) - b
    # where the used called samples stand in the walk: a dense-form row's sample index, else the rank among the
    # row's entries (the samples whose code is not the base code, whatever their phenotype); a sample that is not an
    # entry has d = 0 and joins no sum
    is_entry = (codes != 0) if dense_form else (codes != base)
    at_all = np.arange(len(codes)) if dense_form else np.cumsum(is_entry) - 1
    walked = is_entry[use]
    at = at_all[use][walked]
    k1 = zt.shape[1]
    wd = (w * d)[walked]
    a = np.zeros((k1 + 1, k1 + 1))
    a[:k1, :k1] = (zt * w[:, None]).T @ zt
    for j in range(k1):
        a[k1, j] = a[j, k1] = segment_sum(wd * zt[walked, j], at)
    a[k1, k1] = segment_sum(wd * d[walked], at)
    low = np.linalg.cholesky(a)
    f = np.linalg.solve(low[:k1, :k1], zt.T @ r)
    u = float(segment_sum(d[walked] * r[walked], at) - low[k1, :k1] @ f)
    lxx = float(low[k1, k1])
    v = lxx * lxx
    stat = u / lxx
    p = math.erfc(abs(stat) * 0.70710678118654752440)
    if not abs(stat) > cutoff:
        return p, p, 0, 0
    t = np.linalg.solve(low[:k1, :k1].T, low[k1, :k1])
    in_e = S.entry_mask(codes, base, dense_form)[use]
    team = 256 if (dense_form or int((codes != base).sum()) > SEG) else 64
    g = d[in_e] - t[0]
    for j in range(1, k1):
        g = g - zt[in_e, j] * t[j]
    ri = r[in_e]
    mu = np.where(ri > 0, 1.0 - ri, -ri)
    v_e = M.team_sum(w[in_e] * g * g, team)
    v_rest = 0.0 if (base == 3 and not dense_form) else max(v - v_e, 0.0)
    total, evals = M.phase_b(g, mu, abs(u), v, v_rest, team)
    if total is None:
        return p, p, 2, evals
    return p, total, 1, evals


def main():
    import test_glm_score_sparse_multi_spa as T

    widths = "--widths" in sys.argv[1:]
    worst_all, evals_all = 0.0, []
    for n in (T.WIDTHS_N,) if widths else T.PARITY_N:
        case = T.inputs(n)
        for k in T.WIDTHS if widths else T.PARITY_K:
            for p in range(len(T.phenotypes(n))):
                nul = T.null_of(n, k, p)
                want = T.oracle_rows(n, k, p, widths)
                worst, applied, failed, kinds = 0.0, 0, 0, set()
                for i, forms in enumerate(want):
                    for (base, dense_form), (row, p_spa, state) in (forms or {}).items():
                        if row["errcode"] is not None:
                            continue
                        _, mp, mstate, evals = model_row(case.geno[i], nul, base, dense_form, T.CUTOFF)
                        assert mstate == state, (n, k, p, i, base, dense_form, state, mstate, evals, row)
                        if state == 1:
                            worst = max(worst, abs(mp - p_spa) / p_spa)
                            applied += 1
                            evals_all.append(evals)
                            kinds.add((base, dense_form))
                        failed += state == 2
                print(f"n={n} k={k} phenotype {p}: {applied} applied, {failed} failed, worst {worst:.3g}, forms "
                      f"{sorted(kinds)}", flush=True)
                worst_all = max(worst_all, worst)
    print(f"worst relative difference of p_spa: {worst_all:.3g}; evaluations per applied row: mean "
          f"{np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
