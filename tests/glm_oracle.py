"""FP64 numpy oracle of plink_glm's per-variant fits (the reference's ComputeLinearRegression /
ComputeLogisticRegression rules), shared by the pgh_glm device tests.

Where the reference's rules and the numerics can be separated, the oracle follows the rule and computes the numbers
another way than the device does: linear fits come from a QR factorisation of the design rather than from its normal
equations, so that the oracle does not lose the digits the kernels could lose."""

import math

import numpy as np
import pytest

scipy_stats = pytest.importorskip("scipy.stats")

NAN = float("nan")


def _chol_ok(a, rel):
    """Cholesky pivots of a (in order); False when one is not positive or below rel x its diagonal."""
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


def _ref_chol_solve(h, g):
    """The reference's Newton Cholesky: a negative pivot becomes 1e-6 instead of failing."""
    p = h.shape[0]
    low = np.zeros_like(h)
    for j in range(p):
        d = h[j, j] - low[j, :j] @ low[j, :j]
        low[j, j] = math.sqrt(d) if d >= 0 else 1e-6
        for i in range(j + 1, p):
            low[i, j] = (h[i, j] - low[i, :j] @ low[j, :j]) / low[j, j]
    with np.errstate(all="ignore"):
        w = np.linalg.solve(low, g) if np.all(np.diag(low) != 0) else np.full(p, np.nan)
        return np.linalg.solve(low.T, w) if np.all(np.isfinite(w)) else np.full(p, np.nan)


def _sigmoid(eta):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-eta))


def _newton(X, y):
    p = X.shape[1]
    b = np.zeros(p)
    min_delta = 1e9
    h = None
    for it in range(1000):
        mu = _sigmoid(X @ b)
        h = (X * (mu * (1 - mu))[:, None]).T @ X
        d = _ref_chol_solve(h, X.T @ (mu - y))
        delta = float(np.sum(np.abs(d)))
        b = b - d
        min_delta = min(min_delta, delta)
        if delta != delta:
            return "failed", b, h
        if it > 3:
            if (delta > 20 and delta > 2 * min_delta) or (it > 6 and abs(1 - delta) < 1e-3):
                return "failed", b, h
            if it > 13:
                return ("failed" if np.any(np.abs(b) > 8e3) else "unfinished"), b, h
        if delta < 1e-4:
            return ("failed" if np.any(np.abs(b) > 6e4) else "converged"), b, h
    raise AssertionError("unreachable")


def _firth(X, y):
    p = X.shape[1]
    b = np.zeros(p)
    delta_max, ll_old, hinv = 0.0, 0.0, None
    for it in range(1000):
        mu = _sigmoid(X @ b)
        if np.any((mu == 0) | (mu == 1)):
            return "failed", b, hinv
        ll = float(np.sum(np.where(y != 0, np.log(mu), np.log1p(-mu))))
        v = mu * (1 - mu)
        h0 = (X * v[:, None]).T @ X
        if not _chol_ok(h0, 1e-13):
            return "failed", b, hinv
        ll += 0.5 * np.linalg.slogdet(h0)[1]
        h0i = np.linalg.inv(h0)
        hd = v * np.einsum("ij,jk,ik->i", X, h0i, X)
        ustar = X.T @ ((y - mu) + hd * (0.5 - mu))
        if it > 0:
            if delta_max <= 1e-4 and np.max(np.abs(ustar)) < 1e-4 and ll - ll_old < 1e-4:
                return "converged", b, hinv
            if it > 25:
                return "unfinished", b, hinv
        ll_old = ll
        hh = (X * ((1 + hd) * v)[:, None]).T @ X
        if not _chol_ok(hh, 1e-13):
            return "failed", b, hinv
        hinv = np.linalg.inv(hh)
        d = hinv @ ustar
        delta_max = float(np.max(np.abs(d)))
        if delta_max > 5:
            d *= 5 / delta_max
            delta_max = 5.0
        b = b + d
    raise AssertionError("unreachable")


def one_pass_sxx(xs):
    """sum x^2 - (sum x)^2 / n: the reference's no-covariate linear closed form (its CONST_ALLELE test)."""
    sx = float(xs.sum())
    return float(np.sum(xs * xs)) - sx * sx / len(xs)


def two_pass_sxx(xs):
    """sum (x - mean)^2: the reference's CONST_ALLELE test on its multivariate linear and its logistic paths."""
    return float(np.sum((xs - float(xs.sum()) / len(xs)) ** 2))


def _linear_lstsq(Zu, xs, ys):
    """Least squares of ys on [1, covariates, x] (genotype last): (beta, rss, (R^T R)^-1 at the genotype).

    The covariate and genotype columns are centred first and the intercept is kept, so the fit is the same model
    whatever the centring's rounding; Householder QR then works on the data's spread rather than its offset."""
    n = len(ys)
    A = np.column_stack([Zu.T, xs]) if Zu.shape[0] else xs[:, None]
    A = A - A.mean(axis=0)
    X = np.column_stack([np.ones(n), A])
    q, r = np.linalg.qr(X)
    coef = np.linalg.solve(r, q.T @ ys)
    resid = ys - X @ coef
    # R is upper triangular with the genotype last: the last row of R^-1 is (0, .., 0, 1 / r_xx)
    return coef[-1], float(resid @ resid), 1.0 / (r[-1, -1] * r[-1, -1])


def oracle_row(x, y, Z, model, firth=True):
    """x: values with -9 = missing; y: NaN = missing; Z: k x n covariates."""
    k = Z.shape[0]
    p = k + 2
    use = (x != -9.0) & ~np.isnan(y)
    n = int(use.sum())
    row = dict(beta=NAN, se=NAN, stat=NAN, p=NAN, a1_freq=NAN, obs_ct=n, errcode=None, firth=False)
    if n < p + 1:
        row["errcode"] = "TOO_FEW_SAMPLES"
        return row
    xs, ys = x[use], y[use]
    row["a1_freq"] = xs.sum() / (2.0 * n)
    sxx = one_pass_sxx(xs) if model == "linear" and k == 0 else two_pass_sxx(xs)
    if sxx < 1e-20:
        row["errcode"] = "CONST_ALLELE"
        return row
    Zu = Z[:, use]
    if model == "linear":
        X = np.column_stack([np.ones(n), Zu.T, xs])
        if not _chol_ok(X.T @ X, 1e-10 if k else 0.0):
            row["errcode"] = "SINGULAR_MATRIX"
            return row
        beta, rss, inv_xx = _linear_lstsq(Zu, xs, ys)
        df = n - p
        se2 = max(0.0, rss) / df * inv_xx
        row["beta"] = beta
        row["rss"], row["tss"] = rss, float(np.sum((ys - ys.mean()) ** 2))
        if se2 < 1e-30:
            row["errcode"] = "ZERO_VARIANCE"
            return row
        row["se"] = math.sqrt(se2)
        row["stat"] = row["beta"] / row["se"]
        row["p"] = 2 * scipy_stats.t.sf(abs(row["stat"]), df)
        return row
    X = np.column_stack([np.ones(n), xs, Zu.T])
    status, b, h = _newton(X, ys)
    if status == "converged":
        if not _chol_ok(h, 1e-13):
            row["errcode"] = "SINGULAR_MATRIX"
            return row
        se2 = np.linalg.inv(h)[1, 1]
    elif firth:
        status, b, hinv = _firth(X, ys)
        if status == "failed":
            row["errcode"] = "NO_CONVERGENCE"
            return row
        row["firth"] = True
        se2 = hinv[1, 1]
    else:
        row["errcode"] = "SEPARATION" if status == "failed" else "NO_CONVERGENCE"
        return row
    row["beta"] = b[1]
    if se2 < 1e-30:
        row["errcode"] = "ZERO_VARIANCE"
        return row
    row["se"] = math.sqrt(se2)
    row["stat"] = row["beta"] / row["se"]
    row["p"] = 2 * scipy_stats.norm.sf(abs(row["stat"]))
    return row


def check_rows(got, xs, y, Z, model, firth=True, rel=1e-9, idx=None, got_idx=None, seen=None, rel_of=None):
    """got: Dataset.glm output; xs: one value row per variant.  got_idx: maps a row of xs to its row of got (default:
    the same index).  seen: a dict that receives the oracle row of every index checked.  rel_of: the tolerance of SE,
    statistic and p for an oracle row (default: rel).  Returns the rows fitted."""
    fitted = 0
    for i in (range(len(xs)) if idx is None else idx):
        gi = i if got_idx is None else got_idx(i)
        exp = oracle_row(xs[i], y, Z, model, firth)
        ctx = (i, exp, {k: got[k][gi] for k in got})
        assert got["errcode"][gi] == exp["errcode"], ctx
        assert got["obs_ct"][gi] == exp["obs_ct"], ctx
        assert bool(got["firth"][gi]) == exp["firth"], ctx
        for key in ("beta", "se", "stat", "p", "a1_freq"):
            g, e = got[key][gi], exp[key]
            if math.isnan(e):
                assert math.isnan(g), (key, ctx)
            else:
                # relative to the value, or for an estimate close to zero to its standard error (the scale of beta)
                scale = abs(e) + (exp["se"] if key == "beta" else 1.0 if key == "stat" else 0.0)
                tol = rel_of(exp) if rel_of is not None and key in ("se", "stat", "p") else rel
                assert abs(g - e) <= tol * scale + 1e-300, (key, ctx)
        fitted += exp["errcode"] is None
        if seen is not None:
            seen[i] = exp
    return fitted


def _pheno(rng, n, kind, Z):
    y = 0.3 * (Z.sum(axis=0) if Z.shape[0] else 0) + rng.normal(size=n)
    if kind == "logistic":
        y = (rng.random(n) < 1 / (1 + np.exp(-0.2 * y))).astype(np.float64)
    y[rng.random(n) < 0.03] = NAN
    return y


def _same_rows(a, b):
    for key in ("beta", "se", "stat", "p", "a1_freq"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for key in ("obs_ct", "errcode", "firth"):
        assert list(a[key]) == list(b[key]), key


def rows_2bit(geno):
    """int8 calls [M][N] (-9 = missing) as 2-bit records (00 hom-ref, 01 het, 10 hom-alt, 11 missing)."""
    m, n = geno.shape
    codes = np.where(geno < 0, 3, geno).astype(np.uint8)
    pad = (-n) % 4
    codes = np.concatenate([codes, np.zeros((m, pad), np.uint8)], axis=1).reshape(m, -1, 4)
    return (codes[:, :, 0] | (codes[:, :, 1] << 2) | (codes[:, :, 2] << 4) | (codes[:, :, 3] << 6)).astype(np.uint8)


def calls_of_rows(rows, n):
    """The inverse of rows_2bit, as float64 values with -9 = missing."""
    m = rows.shape[0]
    codes = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(m, -1)[:, :n]
    return np.where(codes == 3, -9.0, codes.astype(np.float64))
