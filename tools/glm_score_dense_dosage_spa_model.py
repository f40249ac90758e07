#!/usr/bin/env python3
"""A numpy model of GlmScoreDenseDosageSpaKernel's arithmetic in the kernel's accumulation order, run on the CPU against
the oracle (tests/glm_spa_dosage_oracle.py) on the inputs of tests/test_glm_score_multi_dosage_spa.py.  It is where that
test's tolerances come from (pgh_glm_score_multi_dosage_spa): 100 x the worst relative
difference of p_spa printed here.

The model follows the device: t, U and V from the Cholesky factor of [[H_N, c], [c', A]] with d = x; b = 2 when
sum_N x > n, otherwise 0; E = the samples of N whose value is not exactly b; gt = x - Zt t as a chain over the
covariates; mu recovered from r; V_E as one chain per thread over the entries of its 16-sample words (thread = word mod
256), a butterfly over the 64 lanes and the waves in order (tools/glm_score_dense_spa_model.py's word_sum: the u16 walk
has the 2-bit walk's geometry); V_rest = 0 when E = N, otherwise max(V - V_E, 0); and phase B over the stash in sample
order with the workgroup as the team, which is tools/glm_score_spa_model.py's phase_b.  A multiply and an add stand
where the kernel has an fma.

usage: python tools/glm_score_dense_dosage_spa_model.py [--widths]
--widths: the inputs of the test's width and edge cases instead (its MODEL_WORST_WIDTHS)."""

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_score_oracle as O  # noqa: E402
import glm_spa_dosage_oracle as D  # noqa: E402
import glm_score_dense_spa_model as DM  # noqa: E402
import glm_score_spa_model as M  # noqa: E402


def model_row(x, nul, cutoff):
    """(p, p_spa, state, evaluations) of a FITTED row as the device computes them."""
    use = (x != -9.0) & nul.in_s
    zt, w, r = nul.zt[use], nul.w[use], nul.r[use]
    d = x[use]
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
    in_e = d != float(D.dosage_base(x, nul.in_s))
    g = d[in_e] - t[0]
    for j in range(1, k1):
        g = g - zt[in_e, j] * t[j]
    ri = r[in_e]
    mu = np.where(ri > 0, 1.0 - ri, -ri)
    v_e = DM.word_sum(w[in_e] * g * g, np.flatnonzero(use)[in_e])
    v_rest = 0.0 if in_e.all() else max(v - v_e, 0.0)
    total, evals = M.phase_b(g, mu, abs(u), v, v_rest, DM.TEAM)
    if total is None:
        return p, p, 2, evals
    return p, total, 1, evals


def run_case(inp, k, stride, cutoff=None, quiet=False, evals_all=None, label=""):
    """One file of the test at k covariates on every stride-th row.  Returns (worst, applied)."""
    import test_glm_score_multi_dosage_spa as T

    cutoff = T.CUTOFF if cutoff is None else cutoff
    Z = T.covariates(inp.n, k)
    worst_all, applied_all = 0.0, 0
    for p, y in enumerate(T.phenotypes(inp.n)):
        nul = O.Null(y, Z)
        assert nul.status is None
        worst, applied, failed, b2, whole = 0.0, 0, 0, 0, 0
        for i in range(0, inp.m, stride):
            row, p_spa, state, b, n_e, e_is_n = D.spa_row(inp.x[i], nul, cutoff)
            if row["errcode"] is not None:
                continue
            _, mp, mstate, evals = model_row(inp.x[i], nul, cutoff)
            assert mstate == state, (inp.n, k, p, i, b, state, mstate, evals, row)
            if state == 1:
                worst = max(worst, abs(mp - p_spa) / p_spa if p_spa > 0 else float(mp != 0))
                applied += 1
                b2 += b == 2
                whole += bool(e_is_n)
                if evals_all is not None:
                    evals_all.append(evals)
            failed += state == 2
        if not quiet:
            print(f"{label}n={inp.n} k={k} phenotype {p}: {applied} applied ({b2} with b = 2, {whole} with E = N), "
                  f"{failed} failed, worst {worst:.3g}", flush=True)
        worst_all = max(worst_all, worst)
        applied_all += applied
    return worst_all, applied_all


def main():
    import test_glm_score_multi_dosage_spa as T

    evals_all = []
    if "--widths" in sys.argv[1:]:
        cases = [(T.widths_inputs(), k, T.WIDTHS_STRIDE, "widths ") for k in T.WIDTHS]
        cases += [(T.edge_inputs(n), k, 1, "edge ") for n in T.EDGE64 for k in T.EDGE64_K]
        cases += [(T.edge_inputs(n), T.STEPS_K, 1, "step ") for n in T.STEPS]
    else:
        cases = [(T.parity_inputs(n), k, 1, "") for _, n, _ in T.MIXED for k in T.PARITY_K]
    worst = max(run_case(inp, k, stride, evals_all=evals_all, label=label)[0] for inp, k, stride, label in cases)
    if "--widths" in sys.argv[1:]:
        # the structured tracks, one phenotype at their own cutoff, are held to the same constant
        lay, x, Z, y = T.structured_inputs()
        nul = O.Null(y, Z)
        rows, _ = T.distinct_rows(x)
        w_s, applied = 0.0, 0
        for i in rows:
            row, p_spa, state = D.spa_row(x[i], nul, T.STRUCTURED_CUTOFF)[:3]
            if row["errcode"] is not None:
                continue
            _, mp, mstate, evals = model_row(x[i], nul, T.STRUCTURED_CUTOFF)
            assert mstate == state, (lay.names[i], state, mstate, evals, row)
            if state == 1:
                w_s = max(w_s, abs(mp - p_spa) / p_spa if p_spa > 0 else float(mp != 0))
                applied += 1
                evals_all.append(evals)
        print(f"structured tracks (n={lay.n}, k={T.STRUCTURED_K}, cutoff {T.STRUCTURED_CUTOFF}): {applied} applied, "
              f"worst {w_s:.3g}", flush=True)
        worst = max(worst, w_s)
    print(f"worst relative difference of p_spa: {worst:.3g}; evaluations per applied row: mean "
          f"{np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
