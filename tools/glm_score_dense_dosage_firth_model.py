#!/usr/bin/env python3
"""A numpy model of GlmScoreDenseDosageFirthKernel's arithmetic in the kernel's accumulation order, run on the CPU
against the oracle (tests/glm_firth_dosage_oracle.py) on the inputs of tests/test_glm_score_multi_dosage_firth.py.  It is
where that test's tolerances come from (pgh_glm_score_multi_dosage_firth): 100 x the worst
difference printed here, over |delta beta| / se, |delta se| / se and |delta p| / p of the applied rows.

The model follows the device: E = the samples of N whose value is not exactly 0, in sample order; x = value / 16384; mu
recovered from r; G as one chain per thread over the entries of its 16-sample words in 4,096-sample steps (thread = word
mod 256), a butterfly over the 64 lanes and the waves in order (tools/glm_score_dense_spa_model.py's word_sum: the u16
walk has the 2-bit walk's geometry); and phase B over the stash with the workgroup as the team: 256 strided chains, the
butterfly and the iteration, which is tools/glm_score_dense_firth_model.py's phase_b.  A multiply and an add stand where
the kernel has an fma.  Which rows are applied is the oracle's decision (it refuses a |stat| within 1e-6 of the cutoff).

usage: python tools/glm_score_dense_dosage_firth_model.py [--widths]
--widths: the inputs of the test's width, edge and structured cases instead (its MODEL_WORST_WIDTHS)."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_score_oracle as O  # noqa: E402
import glm_firth_dosage_oracle as D  # noqa: E402
from glm_score_dense_firth_model import phase_b  # noqa: E402
from glm_score_dense_spa_model import word_sum  # noqa: E402


def model_row(x, nul):
    """(beta, se, p, evaluations) of an APPLIED row as the device computes them."""
    in_e = (x != -9.0) & (x != 0) & nul.in_s
    xe = x[in_e]
    r = nul.r[in_e]
    mu = np.where(r > 0, 1.0 - r, -r)
    g = word_sum(xe * r, np.flatnonzero(in_e))
    return phase_b(xe, mu, g)


def run_rows(x, rows, nul, cutoff, evals_all=None, ctx=None):
    """The rows `rows` of the value rows x under one null model.  Returns (worst, applied, failed, info of the applied)."""
    worst, applied, failed, infos = 0.0, 0, 0, []
    for i in rows:
        row, beta, se, pv, state, info = D.firth_row(x[i], nul, cutoff)
        if state == 0:
            continue
        mb, mse, mp, evals = model_row(x[i], nul)
        assert (mb is None) == (state == 2), (ctx, i, state, mb, evals, row)
        failed += state == 2
        if state == 1:
            worst = max(worst, abs(mb - beta) / se, abs(mse - se) / se, abs(mp - pv) / pv)
            applied += 1
            infos.append(info)
            if evals_all is not None:
                evals_all.append(evals)
    return worst, applied, failed, infos


def run_case(inp, k, stride, cutoff=None, quiet=False, evals_all=None, label=""):
    """One file of the test at k covariates on every stride-th row.  Returns (worst, applied)."""
    import test_glm_score_multi_dosage_firth as T

    cutoff = T.CUTOFF if cutoff is None else cutoff
    Z = T.covariates(inp.n, k)
    worst_all, applied_all = 0.0, 0
    for p, y in enumerate(T.phenotypes(inp.n)):
        nul = O.Null(y, Z)
        assert nul.status is None
        worst, applied, failed, infos = run_rows(inp.x, range(0, inp.m, stride), nul, cutoff, evals_all, (inp.n, k, p))
        if not quiet:
            print(f"{label}n={inp.n} k={k} phenotype {p}: {applied} applied ({sum(i['whole'] for i in infos)} with "
                  f"E = N, {sum(i['separated'] for i in infos)} separated), {failed} failed, worst {worst:.3g}", flush=True)
        worst_all = max(worst_all, worst)
        applied_all += applied
    return worst_all, applied_all


def main():
    import test_glm_score_multi_dosage_firth as T

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
        w_s, applied, failed, _ = run_rows(x, rows, nul, T.STRUCTURED_CUTOFF, evals_all, "structured")
        print(f"structured tracks (n={lay.n}, k={T.STRUCTURED_K}, cutoff {T.STRUCTURED_CUTOFF}): {applied} applied, "
              f"{failed} failed, worst {w_s:.3g}", flush=True)
        worst = max(worst, w_s)
    print(f"worst difference over |delta beta| / se, |delta se| / se, |delta p| / p: {worst:.3g}; evaluations per "
          f"applied row: mean {np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
