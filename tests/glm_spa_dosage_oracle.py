"""FP64 numpy oracle of pgh_glm_score_multi_dosage_spa: the saddlepoint p-value of the logistic score test of a row of
real-valued genotype values (the explicit dosage / 16384, else the call; -9 = neither).

The dosage rule of include/pgenhip.h on top of glm_spa_oracle's Cgf (K, K', K'' with logaddexp, the root by bisection to
the last bit, the support's decision when V_rest = 0) and glm_score_oracle's Null and oracle_row:
  b = 2 if sum_N x > n, otherwise 0 -- compared in integers on the 2^-14 grid;
  E = the samples of N with x != b;
  V_rest = 0 by rule when E = N, otherwise summed over N \\ E (not V - V_E).
gt is the Householder-QR residual of x on the covariates and mu the sigmoid of the oracle's own null fit, as in
glm_spa_oracle.cgf_of."""

import math

import numpy as np

import glm_score_oracle as O
import glm_spa_oracle as S

NAN = float("nan")
GRID = 16384


def dosage_base(x, in_s):
    """b of one row of values for the samples in_s: an exact comparison of sum_N x with n."""
    use = (x != -9.0) & in_s
    v = np.rint(x[use] * GRID).astype(np.int64)
    assert np.array_equal(v / GRID, x[use]), "the values lie on the 2^-14 grid"
    return 2 if int(v.sum()) > GRID * int(use.sum()) else 0


def cgf_of(x, nul, b):
    """(Cgf, U, V, |E|, E == N) of a fitted row."""
    use = (x != -9.0) & nul.in_s
    xs, w, r, zt = x[use], nul.w[use], nul.r[use], nul.zt[use]
    sw = np.sqrt(w)
    qq, rr = np.linalg.qr(zt * sw[:, None])
    g = xs - zt @ np.linalg.solve(rr, qq.T @ (sw * xs))
    mu = 1.0 / (1.0 + np.exp(-(zt @ nul.beta)))
    in_e = xs != float(b)
    whole = bool(in_e.all())
    v_rest = 0.0 if whole else float(np.sum(w[~in_e] * g[~in_e] ** 2))
    return S.Cgf(g[in_e], mu[in_e], v_rest), float(g @ r), float(np.sum(w * g * g)), int(in_e.sum()), whole


def spa_row(x, nul, cutoff):
    """(row, p_spa, state, b, |E|, E == N) of one variant; the row is glm_score_oracle's.  |E| and E == N are None
    where the saddlepoint is not attempted.  Asserts where the contract does not decide (glm_spa_oracle.UNDECIDED)."""
    row = O.oracle_row(x, nul)
    b = dosage_base(x, nul.in_s)
    if row["errcode"] is not None:
        return row, NAN, 0, b, None, None
    assert abs(abs(row["stat"]) - cutoff) > S.UNDECIDED, ("|stat| is too near the cutoff to decide", row["stat"])
    if not abs(row["stat"]) > cutoff:
        return row, row["p"], 0, b, None, None
    cgf, u, v, n_e, whole = cgf_of(x, nul, b)
    tails = [cgf.tail(q, v) for q in (abs(u), -abs(u))]
    if any(t is None for t in tails) or not math.isfinite(sum(tails)):
        return row, row["p"], 2, b, n_e, whole
    return row, sum(tails), 1, b, n_e, whole


def oracle_column(xs, y, Z, cutoff, idx=None):
    """spa_row per variant of one phenotype; None where idx leaves a variant out."""
    nul = O.Null(y, Z)
    assert nul.status is None, nul.status
    out = [None] * len(xs)
    for i in (range(len(xs)) if idx is None else idx):
        out[i] = spa_row(xs[i], nul, cutoff)
    return out


def check_column(got, p, want, tol, ctx=None):
    """Column p of Dataset.glm_score_multi_dosage_spa's dict against oracle_column's rows: equal errcodes and states,
    p_spa within tol (relative) in state 1, bit-equal to p in states 0 and 2, NaN where the row is not fitted.
    Returns (applied, worst)."""
    applied, worst = 0, 0.0
    for i, w in enumerate(want):
        if w is None:
            continue
        row, p_spa, state = w[:3]
        g_p, g_spa, g_state = got["p"][i, p], got["p_spa"][i, p], got["spa_state"][i, p]
        at = (ctx, i, p, w, g_p, g_spa, g_state, got["errcode"][i, p])
        assert got["errcode"][i, p] == row["errcode"], at
        assert g_state == state, at
        if row["errcode"] is not None:
            assert math.isnan(g_spa), at
        elif state != 1:
            assert g_spa == g_p, at
        else:
            diff = abs(g_spa - p_spa) / p_spa if p_spa > 0 else float(g_spa != 0)  # (glm_spa_oracle.check_spa's rule)
            worst = max(worst, diff)
            assert diff <= tol, (diff, at)
            applied += 1
    return applied, worst
