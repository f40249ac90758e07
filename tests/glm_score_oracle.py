"""FP64 numpy oracle of pgh_glm_score_sparse: the logistic score test of a variant given the covariates.

The rules are the header's (include/pgenhip.h); the numbers are computed another way than the device computes them.
The used samples N of a variant come straight from its dense calls, with no base code; x is residualised on the
covariates by a Householder QR of sqrt(w) [1, z] rather than through the normal equations and their Cholesky factor,
so that the oracle does not lose the digits the kernels could lose; p is erfc(|stat| / sqrt 2)."""

import math

import numpy as np

NAN = float("nan")
PIVOT = 1e-10  # the pivot rule of every Cholesky factor of the contract


def chol_ok(a, rel=PIVOT):
    """Cholesky pivots of a, in order: False when one is not positive or at most rel x its diagonal entry."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    low = np.zeros_like(a)
    for j in range(n):
        d = a[j, j] - low[j, :j] @ low[j, :j]
        if not d > 0 or d <= rel * abs(a[j, j]):
            return False
        low[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            low[i, j] = (a[i, j] - low[i, :j] @ low[j, :j]) / low[j, j]
    return True


def _sigmoid(eta):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-eta))


class Null:
    """The covariates-only fit over S = the samples with a phenotype.  status: None (fitted), "SINGULAR_MATRIX",
    "NO_CONVERGENCE" or "skipped" (n_y < k + 3).  zt, w, r: per sample of the call (r NaN outside S)."""

    def __init__(self, y, Z, tol=1e-12):
        y = np.asarray(y, dtype=np.float64)
        n = len(y)
        self.k = k = Z.shape[0]
        self.in_s = s = ~np.isnan(y)
        self.n_y = int(s.sum())
        zc = Z - Z[:, s].mean(axis=1, keepdims=True) if k else Z
        self.zt = zt = np.column_stack([np.ones(n), zc.T])
        self.beta = np.zeros(k + 1)
        self.status = None
        self.steps = 0
        if self.n_y < k + 3:
            self.status = "skipped"
        X, ys = zt[s], y[s]
        while self.status is None:
            mu = _sigmoid(X @ self.beta)
            h = (X * (mu * (1 - mu))[:, None]).T @ X
            if not chol_ok(h):
                self.status = "SINGULAR_MATRIX" if self.steps == 0 else "NO_CONVERGENCE"
                break
            if self.steps == 25:
                self.status = "NO_CONVERGENCE"
                break
            with np.errstate(all="ignore"):
                delta = np.linalg.solve(h, X.T @ (ys - mu))
            if not np.all(np.isfinite(delta)) or not np.all(np.isfinite(self.beta + delta)):
                self.status = "NO_CONVERGENCE"
                break
            self.beta = self.beta + delta
            self.steps += 1
            if np.max(np.abs(delta)) <= tol:
                break
        mu = _sigmoid(zt @ self.beta)
        self.w = np.where(s, mu * (1 - mu), 0.0)
        self.r = np.where(s, y - mu, NAN)


def score_parts(x, nul):
    """(U, V, A, used) of one variant: x holds values with -9 = missing.  A is sum_N w x^2."""
    use = (x != -9.0) & nul.in_s
    xs, w, r, zt = x[use], nul.w[use], nul.r[use], nul.zt[use]
    sw = np.sqrt(w)
    q, rr = np.linalg.qr(zt * sw[:, None])
    t = np.linalg.solve(rr, q.T @ (sw * xs))
    res = xs - zt @ t
    return float(res @ r), float((sw * res) @ (sw * res)), float(w @ (xs * xs)), use


def oracle_row(x, nul):
    k = nul.k
    use = (x != -9.0) & nul.in_s
    n = int(use.sum())
    row = dict(beta=NAN, se=NAN, stat=NAN, p=NAN, a1_freq=NAN, obs_ct=n, errcode=None, firth=False)
    if n < k + 3:
        row["errcode"] = "TOO_FEW_SAMPLES"
        return row
    xs = x[use]
    row["a1_freq"] = xs.sum() / (2.0 * n)
    if np.all(xs == xs[0]):
        row["errcode"] = "CONST_ALLELE"
        return row
    if nul.status is not None:
        assert nul.status != "skipped"
        row["errcode"] = nul.status
        return row
    zt, w = nul.zt[use], nul.w[use]
    if not chol_ok((zt * w[:, None]).T @ zt):
        row["errcode"] = "SINGULAR_MATRIX"
        return row
    u, v, _, _ = score_parts(x, nul)
    # the last pivot V against A = sum_N w d^2, d = x - b: whatever base code b the dataset holds the row with, the
    # rule must decide alike, or the case is not one the contract decides
    ratios = [v / a for a in (float(w @ ((xs - b) ** 2)) for b in (0.0, 1.0, 2.0)) if a > 0]
    singular = [not v > 0 or ratio <= PIVOT for ratio in ratios]
    assert all(singular) or not any(singular), ("V / A straddles the pivot rule", v, ratios)
    assert all(singular) or min(ratios) > 100 * PIVOT, ("V / A is too close to the pivot rule", v, ratios)
    if all(singular):
        row["errcode"] = "SINGULAR_MATRIX"
        return row
    row["beta"] = u / v
    row["se"] = 1.0 / math.sqrt(v)
    row["stat"] = u / math.sqrt(v)
    row["p"] = math.erfc(abs(row["stat"]) / math.sqrt(2.0))
    return row


def check_rows(got, xs, nul, rel=1e-9, idx=None, got_idx=None):
    """got: Dataset.glm_score_sparse's dict; xs: one value row (-9 = missing) per variant; nul: Null(y, Z).  Asserts
    on glm_oracle.check_rows' scale: beta relative to |beta| + se, stat to |stat| + 1, se and p to their value.
    Returns (rows fitted, the worst relative difference seen)."""
    fitted, worst = 0, 0.0
    for i in (range(len(xs)) if idx is None else idx):
        gi = i if got_idx is None else got_idx(i)
        exp = oracle_row(xs[i], nul)
        ctx = (i, exp, {key: got[key][gi] for key in got})
        assert got["errcode"][gi] == exp["errcode"], ctx
        assert got["obs_ct"][gi] == exp["obs_ct"], ctx
        assert not got["firth"][gi], ctx
        for key in ("beta", "se", "stat", "p", "a1_freq"):
            g, e = got[key][gi], exp[key]
            if math.isnan(e):
                assert math.isnan(g), (key, ctx)
            else:
                scale = abs(e) + (exp["se"] if key == "beta" else 1.0 if key == "stat" else 0.0)
                diff = abs(g - e) / scale if scale > 0 else abs(g - e)
                worst = max(worst, diff)
                assert abs(g - e) <= rel * scale + 1e-300, (key, diff, ctx)
        fitted += exp["errcode"] is None
    return fitted, worst


def pheno(rng, n, Z, case_rate=0.2, missing=0.03):
    """A Bernoulli 0/1 phenotype with about case_rate cases that depends on the covariates, NaN at `missing`."""
    zs = Z / np.maximum(Z.std(axis=1, keepdims=True), 1e-300) if Z.shape[0] else Z
    eta = math.log(case_rate / (1 - case_rate)) + (0.3 * zs.sum(axis=0) if Z.shape[0] else 0.0)
    y = (rng.random(n) < _sigmoid(eta)).astype(np.float64)
    y[rng.random(n) < missing] = NAN
    return y
