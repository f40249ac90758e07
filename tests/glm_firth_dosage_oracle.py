"""FP64 numpy oracle of pgh_glm_score_multi_dosage_firth: the approximate Firth estimate of a row of real-valued genotype
values (the explicit dosage / 16384, else the call; -9 = neither).

The dosage rule of include/pgenhip.h on top of glm_firth_oracle's Cgf (K through K'''' with logaddexp and the logit, the
contract's iteration, numpy's pairwise sums) and glm_score_oracle's Null and oracle_row:
  E = the samples of N with x != 0 exactly; there is no base code, whatever the row's majority.
mu is recovered from nul.r, as the contract defines it."""

import math

import numpy as np

import glm_firth_oracle as F
import glm_score_oracle as O

NAN = float("nan")
GRID = 16384
FIRTH_KEYS = ("beta_firth", "se_firth", "p_firth")


def cgf_of(x, nul):
    """(Cgf, E is separated: its samples all cases or all controls, |E|, E == N) of a row of values."""
    use = (x != -9.0) & nul.in_s
    v = np.rint(x[use] * GRID)
    assert np.array_equal(v / GRID, x[use]), "the values lie on the 2^-14 grid"
    in_e = (x != -9.0) & (x != 0) & nul.in_s
    r = nul.r[in_e]
    separated = bool(len(r) and ((r > 0).all() or (r < 0).all()))
    return F.Cgf(x[in_e], r), separated, int(in_e.sum()), bool(in_e.sum() == use.sum())


def firth_row(x, nul, cutoff):
    """(row, beta, se, p, state, info) of one variant; the row is glm_score_oracle's.  info: evals, separated, n_e,
    whole (E == N).  Asserts where the contract does not decide (glm_firth_oracle.UNDECIDED)."""
    row = O.oracle_row(x, nul)
    info = dict(evals=0, separated=False, n_e=None, whole=None)
    if row["errcode"] is not None:
        return row, NAN, NAN, NAN, 0, info
    assert abs(abs(row["stat"]) - cutoff) > F.UNDECIDED, ("|stat| is too near the cutoff to decide", row["stat"])
    if not abs(row["stat"]) > cutoff:
        return row, row["beta"], row["se"], row["p"], 0, info
    cgf, info["separated"], info["n_e"], info["whole"] = cgf_of(x, nul)
    beta, se, p, info["evals"] = cgf.solve()
    if beta is None:
        return row, row["beta"], row["se"], row["p"], 2, info
    return row, beta, se, p, 1, info


def oracle_column(xs, y, Z, cutoff, idx=None):
    """firth_row per variant of one phenotype; None where idx leaves a variant out."""
    nul = O.Null(y, Z)
    assert nul.status is None, nul.status
    out = [None] * len(xs)
    for i in (range(len(xs)) if idx is None else idx):
        out[i] = firth_row(xs[i], nul, cutoff)
    return out


def check_column(got, p, want, tol, ctx=None):
    """Column p of Dataset.glm_score_multi_dosage_firth's dict against oracle_column's rows: equal errcodes and states,
    NaN in every field where the row is not fitted, bit-equal to out's beta, se and p in states 0 and 2, and in state 1
    within tol on test_glm_score_multi_firth.check_column's three differences: |delta beta| / se, |delta se| / se,
    |delta p| / p.  Returns (applied, worst)."""
    applied, worst = 0, 0.0
    for i, w in enumerate(want):
        if w is None:
            continue
        row, beta, se, pv, state, _ = w
        g = [got[key][i, p] for key in FIRTH_KEYS]
        at = (ctx, i, p, row, beta, se, pv, state, g, got["firth_state"][i, p], got["errcode"][i, p])
        assert got["errcode"][i, p] == row["errcode"], at
        assert got["firth_state"][i, p] == state, at
        if row["errcode"] is not None:
            assert all(math.isnan(v) for v in g), at
        elif state != 1:
            assert g == [got[key][i, p] for key in ("beta", "se", "p")], at
        else:
            diffs = (abs(g[0] - beta) / se, abs(g[1] - se) / se, abs(g[2] - pv) / pv)
            worst = max(worst, *diffs)
            assert max(diffs) <= tol, (diffs, at)
            applied += 1
    return applied, worst
