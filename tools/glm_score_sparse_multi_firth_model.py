#!/usr/bin/env python3
"""The numpy model of GlmScoreSparseMultiFirthKernel's arithmetic in the kernel's accumulation order, run on the CPU
against the oracle (tests/glm_firth_sparse_oracle.py, one glm_score_oracle.Null per phenotype) on the inputs of
tests/test_glm_score_sparse_multi_firth.py.  It is where that test's tolerance comes from (DESIGN.md section 3.10,
pgh_glm_score_sparse_multi_firth): 100 x the worst difference printed here, over |delta beta| / se, |delta se| / se and
|delta p| / p of the applied rows.

The kernel runs the one-phenotype route's row function (SparseFirthRow, glm_firth.hpp) per listed (variant, phenotype)
row, with r read from the phenotype's column of the pair block: the walk, the order of the pairs, G as a lane chain and a
team reduction, and phase B are GlmScoreSparseFirthKernel's.  So the model is tools/glm_score_sparse_firth_model.py's
model_row, imported, under each phenotype's own null fit.  Which rows are applied is the oracle's decision (it refuses a
|stat| within 1e-6 of the cutoff); the model's state (an estimate, or none) must equal the oracle's for every such row.

usage: python tools/glm_score_sparse_multi_firth_model.py [--widths]
--widths: the rows of the test's wave / workgroup edge cases, at k = 0, 3 and 20, instead (its MODEL_WORST_WIDTHS)."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_firth_sparse_oracle as FS  # noqa: E402
import glm_score_oracle as O  # noqa: E402
from glm_score_sparse_firth_model import model_row  # noqa: E402


def compare(label, rows, worst_all, evals_all):
    """rows: (codes, nul, base, dense_form, firth_row_sparse's tuple).  Prints a line; returns the worst so far."""
    worst, applied, failed, kinds = [0.0, 0.0, 0.0], 0, 0, set()
    for codes, nul, base, dense_form, (row, beta, se, pv, state, info) in rows:
        if state == 0:
            continue
        mb, mse, mp, evals, team = model_row(codes, nul, base, dense_form)
        assert (mb is None) == (state == 2), (label, base, dense_form, state, mb, evals, row)
        failed += state == 2
        if state == 1:
            worst = [max(a, c) for a, c in zip(worst, FS.scales(mb, mse, mp, beta, se, pv))]
            applied += 1
            evals_all.append(evals)
            kinds.add((base, dense_form, team))
    print(f"{label}: {applied} applied, {failed} failed, worst beta {worst[0]:.3g} se {worst[1]:.3g} p {worst[2]:.3g}, "
          f"(base, dense form, team) {sorted(kinds)}", flush=True)
    return max(worst_all, *worst)


def main():
    import test_glm_score_sparse_multi_firth as T

    worst_all, evals_all = 0.0, []
    if "--widths" in sys.argv[1:]:
        case, geno = T.inputs(T.EDGE_N), T.edge_rows()
        for k in T.EDGE_K:
            _, cols = T.edge_oracle(k)
            for p, y in enumerate(T.phenotypes(T.EDGE_N)):
                nul = O.Null(y, case.covariates(k))
                rows = [(geno[v], nul, 0, False, cols[p][v]) for v in range(len(geno))]
                worst_all = compare(f"edge rows k={k} phenotype {p}", rows, worst_all, evals_all)
    else:
        for n in T.PARITY_N:
            case = T.inputs(n)
            for k in T.PARITY_K:
                for p in range(len(T.phenotypes(n))):
                    nul = T.null_of(n, k, p)
                    rows = [(case.geno[i], nul, base, dense_form, w) for i, forms in enumerate(T.oracle_rows(n, k, p))
                            for (base, dense_form), w in forms.items()]
                    worst_all = compare(f"n={n} k={k} phenotype {p}", rows, worst_all, evals_all)
    print(f"worst difference over |delta beta| / se, |delta se| / se, |delta p| / p: {worst_all:.3g}; evaluations per "
          f"applied row: mean {np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
