"""FP64 numpy oracle of pgh_glm_score_multi_firth: the approximate Firth estimate of the dense route's rows.

The rules are the header's (include/pgenhip.h), taken literally: the covariate part is fixed at the null fit, E = the
called samples of the phenotype with x != 0, and the penalised likelihood of the variant's own coefficient is written
with the cumulant generating function K over E.  The numbers are computed another way than the device computes them:
the row and its |stat| are glm_score_oracle's (a Householder QR), K is written with logaddexp and pi with the logit,
and every sum is numpy's pairwise sum over E rather than 256 chains and a butterfly.  mu is recovered from nul.r, as
the contract defines it."""

import math

import numpy as np

import glm_score_oracle as O

NAN = float("nan")
MAX_EVAL = 64
STOP = 1e-10
ULPS = 2.0 ** -50
UNDECIDED = 1e-6  # how near the cutoff |stat| may lie before the contract stops deciding


class Cgf:
    """K and its derivatives over E, and l*, F, H of the contract.  x, r: over E."""

    def __init__(self, x, r):
        self.x = np.asarray(x, dtype=np.float64)
        r = np.asarray(r, dtype=np.float64)
        self.mu = np.where(r > 0, 1.0 - r, -r)
        self.g = float(np.sum(self.x * r))
        with np.errstate(divide="ignore"):
            self.lm, self.l1m = np.log(self.mu), np.log1p(-self.mu)

    def pi_q(self, beta):
        """pi and 1 - pi, each without cancellation."""
        a = self.lm - self.l1m + self.x * beta
        e = np.exp(-np.abs(a))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        return np.where(a >= 0, big, small), np.where(a >= 0, small, big)

    def k(self, beta):
        """(K, K', K'', K''', K'''')"""
        x, mu = self.x, self.mu
        pi, q = self.pi_q(beta)
        v = pi * q
        k0 = np.sum(np.logaddexp(self.l1m, self.lm + x * beta) - mu * x * beta)
        return (float(k0), float(np.sum(x * (pi - mu))), float(np.sum(x ** 2 * v)),
                float(np.sum(x ** 3 * v * (q - pi))), float(np.sum(x ** 4 * v * (1.0 - 6.0 * v))))

    def at(self, beta):
        """(l*, F, H, K'', H was replaced by K'') at beta; K'' not > 0: (NaN, NaN, NaN, K'', False)."""
        k0, k1, k2, k3, k4 = self.k(beta)
        if not k2 > 0:
            return NAN, NAN, NAN, k2, False
        ls = beta * self.g - k0 + 0.5 * math.log(k2)
        f = self.g - k1 + 0.5 * k3 / k2
        h = k2 - 0.5 * (k4 / k2 - (k3 / k2) ** 2)
        replaced = not h > 0
        return ls, f, (k2 if replaced else h), k2, replaced

    def lstar(self, beta):
        return self.at(beta)[0]

    def solve(self):
        """(beta, se, p, evaluations) by the contract's iteration, or (None, None, None, evaluations): state 2."""
        sgn, u, lo, hi, grow, tol, l0 = 0.0, 0.0, 0.0, math.inf, 0.0, 0.0, 0.0
        for ev in range(1, MAX_EVAL + 1):
            beta = sgn * u
            ls, f, h, k2, _ = self.at(beta)
            if not (math.isfinite(ls) and math.isfinite(f) and math.isfinite(h)):
                return None, None, None, ev
            if ev == 1:
                sgn, l0 = (1.0 if f > 0 else -1.0), ls
                grow = 1.0 / math.sqrt(k2)
                tol = STOP * grow
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
                done = d <= tol or hi - lo <= tol or d <= ULPS * u
            if done:
                dev = max(2.0 * (ls - l0), 0.0)
                return beta, 1.0 / math.sqrt(k2), math.erfc(math.sqrt(dev) / math.sqrt(2.0)), ev
            u = un
        return None, None, None, MAX_EVAL


def cgf_of(x, codes, nul):
    """The Cgf of a row and whether E is separated (its samples all cases or all controls)."""
    in_e = (codes != 3) & (codes != 0) & nul.in_s
    assert np.array_equal(x[in_e], codes[in_e].astype(np.float64))
    r = nul.r[in_e]
    return Cgf(x[in_e], r), bool(len(r) and ((r > 0).all() or (r < 0).all()))


def firth_row(x, codes, nul, cutoff):
    """(row, beta, se, p, state, info) of one variant: the row is glm_score_oracle's.  info: evals, separated."""
    row = O.oracle_row(x, nul)
    info = dict(evals=0, separated=False)
    if row["errcode"] is not None:
        return row, NAN, NAN, NAN, 0, info
    assert abs(abs(row["stat"]) - cutoff) > UNDECIDED, ("|stat| is too near the cutoff to decide", row["stat"])
    if not abs(row["stat"]) > cutoff:
        return row, row["beta"], row["se"], row["p"], 0, info
    cgf, info["separated"] = cgf_of(x, codes, nul)
    beta, se, p, info["evals"] = cgf.solve()
    if beta is None:
        return row, row["beta"], row["se"], row["p"], 2, info
    return row, beta, se, p, 1, info
