#!/usr/bin/env python3
"""A numpy model of GlmScoreSparseFirthKernel's arithmetic in the kernel's accumulation order, run on the CPU against
the oracle (tests/glm_firth_sparse_oracle.py) on the inputs of the parity test of
tests/test_glm_score_sparse_firth.py.  It is where that test's tolerance comes from (DESIGN.md section 3.10,
pgh_glm_score_sparse_firth): 100 x the worst difference printed here, over |delta beta| / se, |delta se| / se and
|delta p| / p of the applied rows.

The model follows the device for both teams, a wave (64 threads: a sparse row of at most 1,024 entries) and the
workgroup (256: a longer sparse row, or a row held in the dense form, walked sample by sample): the row's entries in
entry order, lane = the entry's place in the row mod the team; E = the used called entries with d = x - b != 0; mu
recovered from r; G = sum_E d r as one chain per lane in visit order, a butterfly over the 64 lanes and the waves in
order 0..3; the pairs (d, mu) in the stash in entry order; and per evaluation
tools/glm_score_dense_firth_model.py's phase B at the team's stride.  A multiply and an add stand where the kernel has
an fma.  Which rows are applied is the oracle's decision (it refuses a |stat| within 1e-6 of the cutoff).

usage: python tools/glm_score_sparse_firth_model.py [--widths]
--widths: the inputs of the test's width and wave / workgroup edge cases instead (its MODEL_WORST_WIDTHS)."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import glm_firth_sparse_oracle as FS  # noqa: E402
import glm_spa_oracle as S  # noqa: E402
import glm_score_spa_model as M  # noqa: E402
from glm_score_dense_firth_model import phase_b  # noqa: E402

LONG = 1024


def lane_sum(v, place, team):
    """sum v as the walk takes it: term j joins the chain of lane place[j] mod team in visit order; then
    glm_score_spa_model.team_sum's butterfly and wave order (on one step of `team` lane sums)."""
    lanes = np.zeros(team)
    for t, at in zip(v, place):
        lanes[at % team] += t
    return M.team_sum(lanes, team)


def model_row(codes, nul, base, dense_form):
    """(beta, se, p, evaluations, team) of an APPLIED row as the device computes them."""
    n = len(codes)
    if dense_form:
        held = np.arange(n)                  # the pool row: every sample is a step of the walk
        team = 256
    else:
        held = np.flatnonzero(codes != base)  # the entries, in sample order
        team = 256 if len(held) > LONG else 64
    b = 0 if (dense_form or base == 3) else base
    c = codes[held]
    in_e = (c != 3) & (c != b) & nul.in_s[held]
    place = np.flatnonzero(in_e)
    d = c[in_e].astype(np.float64) - b
    r = nul.r[held[in_e]]
    mu = np.where(r > 0, 1.0 - r, -r)
    g = lane_sum(d * r, place, team)
    return phase_b(d, mu, g, team) + (team,)


def run(cases):
    """cases: (label, codes, x, nul, forms per row or max_minor, rows).  Prints a line per case; returns (worst,
    evaluations)."""
    import test_glm_score_sparse_firth as T

    worst_all, evals_all = 0.0, []
    for label, codes, x, nul, forms, rows in cases:
        worst, applied, failed, kinds = [0.0, 0.0, 0.0], 0, 0, set()
        for i in rows:
            base, dense_form = forms[i] if isinstance(forms, list) else S.row_form(codes[i], forms)
            row, beta, se, pv, state, info = FS.firth_row_sparse(x[i], codes[i], nul, base, dense_form, T.CUTOFF)
            if state == 0:
                continue
            mb, mse, mp, evals, team = model_row(codes[i], nul, base, dense_form)
            assert (mb is None) == (state == 2), (label, i, state, mb, evals, row)
            failed += state == 2
            if state == 1:
                worst = [max(a, c) for a, c in zip(worst, FS.scales(mb, mse, mp, beta, se, pv))]
                applied += 1
                evals_all.append(evals)
                kinds.add((base, dense_form, team))
        print(f"{label}: {applied} applied, {failed} failed, worst beta {worst[0]:.3g} se {worst[1]:.3g} p {worst[2]:.3g}, "
              f"(base, dense form, team) {sorted(kinds)}", flush=True)
        worst_all = max(worst_all, *worst)
    return worst_all, evals_all


def main():
    import test_glm_score_sparse_firth as T

    cases = []
    if "--widths" in sys.argv[1:]:
        # the inputs of test_every_width_feeding_the_kernel and test_the_wave_workgroup_edge, on the rows they check
        case = T.inputs(T.WIDTHS_N)
        for k in T.WIDTHS:
            for max_minor in (T.WIDTHS_N, 0):
                nul, _ = T.widths_oracle(k, max_minor)
                cases.append((f"n={case.n} k={k} max_minor={max_minor}", case.geno, case.x, nul, max_minor, T.WIDTHS_ROWS))
        for k in T.EDGE_K:
            nul, x, _ = T.edge_oracle(k)
            cases.append((f"edge rows k={k}", T.edge_rows(), x, nul, T.EDGE_N, range(len(T.EDGE_ENTRIES))))
    else:
        for n in T.PARITY_N:
            case = T.inputs(n)
            for k in T.PARITY_K:
                for max_minor in T.max_minors(n):
                    cases.append((f"n={n} k={k} max_minor={max_minor}", case.geno, case.x, T.null_of(n, k), max_minor,
                                  range(case.m)))
    worst_all, evals_all = run(cases)
    print(f"worst difference over |delta beta| / se, |delta se| / se, |delta p| / p: {worst_all:.3g}; evaluations per "
          f"applied row: mean {np.mean(evals_all):.2f}, max {max(evals_all)}")


if __name__ == "__main__":
    main()
