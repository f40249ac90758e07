"""FP64 numpy oracle of pgh_glm_score_sparse_firth: the approximate Firth estimate of the sparse route's rows.

The rules are the header's (include/pgenhip.h), taken literally: b is the row's base code (0 for a missing-majority row
and for a row held in the dense form), d = x - b, E = the row's used called entries with d != 0, and everything else is
pgh_glm_score_multi_firth's contract with d in place of x.  The numbers are computed another way than the device
computes them: the row and its |stat| are glm_score_oracle's (a Householder QR over the dense calls, no base code), E
is cut from the dense code row by a mask rather than walked as an entry list, K, its derivatives and the iteration are
glm_firth_oracle.Cgf's (logaddexp, the logit, numpy's pairwise sums over E rather than lane chains and a butterfly).
The base code and the form a dataset holds a row in are inputs: they make E and d."""

import math

import numpy as np

import glm_firth_oracle as F
import glm_score_oracle as O
import glm_spa_oracle as S

NAN = float("nan")


def e_mask(codes, base, dense_form, nul):
    """(b, the samples of E): the used called entries with d != 0."""
    b = 0 if (dense_form or base == 3) else base
    return b, (codes != 3) & (codes != b) & nul.in_s


def cgf_of(x, codes, nul, base, dense_form):
    """(Cgf over E under d-coding, |E|)"""
    b, in_e = e_mask(codes, base, dense_form, nul)
    assert np.array_equal(x[in_e], codes[in_e].astype(np.float64))
    return F.Cgf(x[in_e] - float(b), nul.r[in_e]), int(in_e.sum())


def firth_row_sparse(x, codes, nul, base, dense_form, cutoff, row=None):
    """(row, beta, se, p, state, info) of one variant: the row is glm_score_oracle's (pass it when it is already there:
    it does not depend on the form).  info: evals, n_e."""
    row = O.oracle_row(x, nul) if row is None else row
    info = dict(evals=0, n_e=0)
    if row["errcode"] is not None:
        return row, NAN, NAN, NAN, 0, info
    assert abs(abs(row["stat"]) - cutoff) > F.UNDECIDED, ("|stat| is too near the cutoff to decide", row["stat"])
    if not abs(row["stat"]) > cutoff:
        return row, row["beta"], row["se"], row["p"], 0, info
    cgf, info["n_e"] = cgf_of(x, codes, nul, base, dense_form)
    assert info["n_e"] > 0, "a fitted row has a non-empty E"
    beta, se, p, info["evals"] = cgf.solve()
    if beta is None:
        return row, row["beta"], row["se"], row["p"], 2, info
    return row, beta, se, p, 1, info


def scales(got_beta, got_se, got_p, beta, se, p):
    """The three scales of the family's Firth checks: |d beta| / se, |d se| / se, |d p| / p."""
    return (abs(got_beta - beta) / se, abs(got_se - se) / se,
            abs(got_p - p) / p if p > 0 else float(got_p != 0))


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def check_firth(got, xs, codes, nul, max_minor, cutoff, tol, idx=None, want=None):
    """got: Dataset.glm_score_sparse_firth's dict; xs / codes: a value row (-9 = missing) and a code row per variant
    (the codes of ALL raw samples decide the form; with a subset pass the form through `max_minor` as a list of (base,
    dense_form)).  want: firth_row_sparse's tuple per variant for these forms and this cutoff, when a caller has
    computed them once and shares them.  Asserts the errcodes and states, the three values within tol on their scales
    in state 1, NaN for a row that is not fitted and out's values bit for bit otherwise.  Returns a dict of what it
    saw; rows: (row, base, dense_form, |E|, entries)."""
    seen = dict(applied=0, failed=0, worst=0.0, max_evals=0, rows=[])
    for i in (range(len(xs)) if idx is None else idx):
        base, dense_form = max_minor[i] if isinstance(max_minor, list) else S.row_form(codes[i], max_minor)
        exp = want[i] if want is not None else firth_row_sparse(xs[i], codes[i], nul, base, dense_form, cutoff)
        row, beta, se, p, state, info = exp
        gb, gs, gp, gst = got["beta_firth"][i], got["se_firth"][i], got["p_firth"][i], got["firth_state"][i]
        ctx = (i, base, dense_form, state, (beta, se, p), (gb, gs, gp, gst), row, info)
        assert got["errcode"][i] == row["errcode"], ctx
        assert not got["firth"][i], ctx
        assert gst == state, ctx
        if row["errcode"] is not None:
            assert math.isnan(gb) and math.isnan(gs) and math.isnan(gp), ctx
            continue
        if state != 1:
            assert same_bits(gb, got["beta"][i]) and same_bits(gs, got["se"][i]) and same_bits(gp, got["p"][i]), ctx
            seen["failed"] += state == 2
            continue
        diff = max(scales(gb, gs, gp, beta, se, p))
        seen["worst"] = max(seen["worst"], diff)
        assert diff <= tol, (diff, ctx)
        seen["applied"] += 1
        seen["max_evals"] = max(seen["max_evals"], info["evals"])
        seen["rows"].append((i, base, dense_form, info["n_e"], int(S.entry_mask(codes[i], base, dense_form).sum())))
    return seen
