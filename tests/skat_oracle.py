"""Dense FP64 numpy oracle of pgh_skat_sparse: per variant set, the SKAT statistic, its eigenvalues and p-value and the
burden score test, under the null model of tests/glm_score_oracle.py.

The rules are the header's (include/pgenhip.h); the numbers are computed another way than the library computes them:
the genotype values of a set are a dense matrix G over S, residualised on the covariates as a whole
(G~ = G - Zt H^-1 Zt' W G), U = G~' r, Phi = G~' W G~, and the eigenvalues are numpy.linalg.eigvalsh's.  The only thing
taken from the resident form (forms: the _Forms of tests/test_burden_sparse.py) is what the header defines by it:
n_carriers and the "every d is zero" rule.  p_from_lambda is a line-for-line transcription of the p-value definition."""

import math

import numpy as np

import glm_score_oracle as O

NAN = float("nan")
VAL = np.array([0.0, 1.0, 2.0, 0.0])  # a missing call is imputed hom-ref
USED = 1e-10                          # an eigenvalue is used iff it is above USED x the largest
NONE, EXACT, SADDLE, NEAR_MEAN, FAILED = range(5)


def phibar(x):
    return 0.5 * math.erfc(x * 0.70710678118654752440)


def _derivs(lam, s):
    a = b = 0.0
    for l in lam:
        t = l / (1.0 - 2.0 * s * l)
        a += t
        b += 2.0 * t * t
    return a, b


def p_from_lambda(q, lam):
    """(p, state) of pgh_skat_p_from_lambda for the used eigenvalues lam."""
    lam = [float(l) for l in lam]
    n = len(lam)
    if n == 0 or not math.isfinite(q):
        return NAN, FAILED
    mu = s2 = s3 = lmax = 0.0
    for l in lam:
        if not math.isfinite(l) or not l > 0.0:
            return NAN, FAILED
        mu += l
        s2 += l * l
        s3 += l * l * l
        lmax = max(lmax, l)
    if q <= 0.0:
        return (1.0 if q == 0.0 else NAN), FAILED
    if n == 1:
        return math.erfc(abs(math.sqrt(q / lam[0])) * 0.70710678118654752440), EXACT
    k2, k3 = 2.0 * s2, 8.0 * s3
    if not (math.isfinite(mu) and math.isfinite(k2) and math.isfinite(k3)):
        return NAN, FAILED
    if abs(q - mu) <= 1e-3 * math.sqrt(k2):
        p = phibar(k3 / (6.0 * k2 * math.sqrt(k2)))
        return (p, NEAR_MEAN) if math.isfinite(p) else (NAN, FAILED)
    up = q > mu
    lo, hi = (0.0, 0.5 / lmax) if up else (-math.inf, 0.0)
    limit = 1.0 / math.sqrt(k2)
    s = (q - mu) / k2
    if up:
        if s >= hi:
            s = 0.5 * hi
    elif -s > limit:
        s = -limit
        limit *= 2.0
    found = False
    for _ in range(100):
        try:
            kd1, kd2 = _derivs(lam, s)
        except ZeroDivisionError:
            return NAN, FAILED
        f = kd1 - q
        if not math.isfinite(f) or not math.isfinite(kd2) or not kd2 > 0.0:
            return NAN, FAILED
        if f > 0.0:
            hi = s
        else:
            lo = s
        nxt = s - f / kd2
        if lo == -math.inf:
            if s - nxt > limit:
                nxt = s - limit
                limit *= 2.0
        elif nxt <= lo:
            nxt = 0.5 * (s + lo)
        elif nxt >= hi:
            nxt = 0.5 * (s + hi)
        step = abs(nxt - s)
        s = nxt
        if step <= 1e-12 * abs(s):
            found = True
            break
    if not found or not math.isfinite(s) or s == 0.0:
        return NAN, FAILED
    try:
        cgf = -0.5 * _sum(math.log1p(-2.0 * s * l) for l in lam)
        kd1, kd2 = _derivs(lam, s)
    except (ValueError, ZeroDivisionError):
        return NAN, FAILED
    w2 = 2.0 * (s * q - cgf)
    if not math.isfinite(w2) or not w2 > 0.0 or not math.isfinite(kd2) or not kd2 > 0.0:
        return NAN, FAILED
    omega = math.sqrt(w2) if s > 0.0 else -math.sqrt(w2)
    nu = s * math.sqrt(kd2)
    ratio = nu / omega
    if not math.isfinite(ratio) or not ratio > 0.0:
        return NAN, FAILED
    p = phibar(omega + math.log(ratio) / omega)
    return (p, SADDLE) if math.isfinite(p) else (NAN, FAILED)


def _sum(values):
    total = 0.0
    for v in values:  # in order, as the library sums
        total += v
    return total


def imhof_sf(q, lam):
    """P(sum lam_k chi^2_1 > q) by Imhof's (1961) inversion integral
        1/2 + 1/pi int_0^inf sin(theta(u)) / (u rho(u)) du,
        theta = 1/2 sum atan(lam_k u) - q u / 2,   rho = prod (1 + lam_k^2 u^2)^(1/4),
    by 16-point Gauss-Legendre panels no wider than half an oscillation (|theta'| <= (sum lam + q) / 2), up to the U at
    which the envelope 1 / (u rho) has fallen to 1e-9.  Returns (p, bound on the truncated tail): the tail of an
    oscillating integrand under a decreasing envelope is at most the envelope at U times one half-period."""
    lam = np.asarray(lam, dtype=np.float64)
    scale = lam.max()
    lam, q = lam / scale, q / scale

    def envelope(u):
        return math.exp(-0.25 * float(np.sum(np.log1p((lam * u) ** 2)))) / u

    top = 1.0
    while envelope(top) > 1e-9:
        top *= 2.0
    h = math.pi / (lam.sum() + q)
    panels = int(math.ceil(top / h))
    assert panels <= 4_000_000, ("the envelope decays too slowly for this quadrature", lam, panels)
    x, wt = np.polynomial.legendre.leggauss(16)
    total = 0.0
    for p0 in range(0, panels, 4096):  # in blocks, to bound the memory
        left = h * np.arange(p0, min(panels, p0 + 4096))
        u = (left[:, None] + 0.5 * h * (x[None, :] + 1.0)).ravel()
        lu = lam[None, :] * u[:, None]
        theta = 0.5 * np.arctan(lu).sum(axis=1) - 0.5 * q * u
        rho = np.exp(0.25 * np.log1p(lu * lu).sum(axis=1))
        total += float(np.sum(np.tile(0.5 * h * wt, len(left)) * np.sin(theta) / (u * rho)))
    return 0.5 + total / math.pi, envelope(h * panels) * h / math.pi


class Null(O.Null):
    """glm_score_oracle.Null, with H and g_S of the fitted model."""

    def __init__(self, y, Z):
        super().__init__(y, Z)
        s = self.in_s
        self.h = (self.zt[s] * self.w[s][:, None]).T @ self.zt[s]
        self.errcode = None if self.status in (None, "skipped") else self.status


def carriers(codes, forms, members, in_s):
    """(n_carriers, any d != 0) of a set: codes over the call's samples, forms the resident form of every variant."""
    if len(members) == 0:
        return 0, False
    touched = np.zeros(codes.shape[1], dtype=bool)
    nonzero = False
    for v in members:
        g = codes[v]
        if forms.dense[v]:
            b, hit = 0, ((g == 1) | (g == 2)) & in_s
        else:
            b = int(forms.major[v])
            hit = (g != b) & in_s
        touched |= hit
        nonzero = nonzero or bool((VAL[g[hit]] != VAL[b]).any())
    return int(touched.sum()), nonzero


def oracle_row(codes, forms, members, omega, nul):
    """(row dict, eigenvalues descending or None) of one set.  codes: (V, n) codes over the call's samples (the
    subsetted matrix); members: variant indices; omega: one weight per membership; nul: Null(y, Z)."""
    m, k = len(members), nul.k
    n_car, nonzero = carriers(codes, forms, members, nul.in_s)
    row = dict(q=NAN, p_skat=NAN, beta=NAN, se=NAN, stat=NAN, p=NAN, lambda_sum=NAN, lambda_max=NAN, obs_ct=nul.n_y,
               n_carriers=n_car, n_lambda=0, errcode=None, p_state=NONE)
    if nul.n_y < k + 3:
        row["errcode"] = "TOO_FEW_SAMPLES"
        return row, None
    if n_car == 0 or not nonzero:
        row["errcode"] = "CONST_ALLELE"
        return row, None
    if nul.errcode is not None:
        row["errcode"] = nul.errcode
        return row, None
    s = nul.in_s
    omega = np.asarray(omega, dtype=np.float64)
    g = VAL[codes[np.asarray(members, dtype=np.int64)]][:, s].T  # n_y x m
    zt, w, r = nul.zt[s], nul.w[s], nul.r[s]
    gt = g - zt @ np.linalg.solve(nul.h, zt.T @ (w[:, None] * g))
    u = gt.T @ r
    phi = gt.T @ (w[:, None] * gt)
    kmat = omega[:, None] * phi * omega[None, :]
    lam = np.linalg.eigvalsh(0.5 * (kmat + kmat.T))[::-1].copy()
    if not np.isfinite(lam[0]) or not lam[0] > 0.0:
        row["errcode"] = "ZERO_VARIANCE"
        return row, None
    # the fixture must not put an eigenvalue near the threshold of use, where rounding decides n_lambda
    near = (np.abs(lam) > USED * lam[0] / 100.0) & (np.abs(lam) < USED * lam[0] * 100.0)
    assert not near.any(), ("an eigenvalue within a factor 100 of the threshold of use", lam)
    used = lam[lam > USED * lam[0]]
    row["q"] = float(np.sum(omega ** 2 * u ** 2))
    # nor a score that cancels to rounding: q == 0 exactly is a state of its own
    assert row["q"] > 1e-20 * abs(np.trace(kmat)), ("the set's scores cancel", row["q"])
    row["lambda_sum"] = float(np.trace(kmat))
    row["lambda_max"] = float(lam[0])
    row["n_lambda"] = len(used)
    row["p_skat"], row["p_state"] = p_from_lambda(row["q"], used)
    ub, vb = float(omega @ u), float(omega @ phi @ omega)
    base = np.array([0.0 if forms.dense[v] else VAL[int(forms.major[v])] for v in members])
    d = g - base[None, :]  # A is defined with d = val(code) - val(base)
    a = d.T @ (w[:, None] * d)
    ab = float(omega @ a @ omega)
    # V_B against omega' A omega: the rule must not be a matter of rounding either
    assert not (1e-12 * ab < abs(vb) < 1e-8 * ab), ("V_B is too close to its pivot rule", vb, ab)
    if vb > 1e-10 * ab:
        row["beta"] = ub / vb
        row["se"] = 1.0 / math.sqrt(vb)
        row["stat"] = ub / math.sqrt(vb)
        row["p"] = math.erfc(abs(row["stat"]) / math.sqrt(2.0))
    return row, lam
