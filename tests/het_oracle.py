"""The yardstick of pgh_het, written from the contract in include/pgenhip.h with no call into the library.

Per variant the counts are Python integers and e comes from the header's statements in Python floats (one correctly
rounded IEEE operation each); q_v = int(np.rint(np.float64(e) * 2.0**k)) (the scaling is exact, rint rounds half to
even as llrint does); the per-sample sums are Python integers; e_hom = math.ldexp(float(e_sum), -k) and f in Python
floats.  Every operation is an integer one or one IEEE operation, so the library's rows must equal these BIT FOR BIT:
same_rows compares every field of every row with tobytes() and there is no tolerance anywhere."""

import math

import numpy as np

ROW_DTYPE = np.dtype([("e_hom", "<f8"), ("f", "<f8"), ("e_sum", "<i8"), ("hom_ct", "<u4"), ("obs_ct", "<u4")])
FIELDS = ("e_hom", "f", "e_sum", "hom_ct", "obs_ct")
NAN = float("nan")


def scale(n_var):
    """k = 62 - L, L the smallest integer with 2^L >= max(n_var, 1)."""
    big, l = max(int(n_var), 1), 0
    while (1 << l) < big:
        l += 1
    return 62 - l


def expected(het, alt, called, freq=None, small_sample=True):
    """e of one variant, or None when it is skipped.  freq=None: p from the counts."""
    if called == 0:
        return None
    p = (het + 2 * alt) / (2 * called) if freq is None else float(freq)  # int / int: correctly rounded
    if not (math.isfinite(p) and 0.0 < p < 1.0):
        return None
    q = 1.0 - p
    tp = 2.0 * p
    u = tp * q
    if small_sample:
        r = float(2 * called) / float(2 * called - 1)
        u = u * r
    return 1.0 - u


def fixed(e, k):
    return int(np.rint(np.float64(e) * 2.0 ** k))


def rows_of(codes, n_var=None, sel=None, freq=None, small_sample=True):
    """(rows, used, n_used) of pgh_het over the variants codes[0], codes[1], .. (one entry of the call each, repeats
    included) and the output samples sel (all when None).  n_var: the caller's count when the codes are only a part of
    the call (never here: len(codes))."""
    codes = np.asarray(codes)
    if sel is not None:
        codes = codes[:, sel]
    v, n = codes.shape
    k = scale(v if n_var is None else n_var)
    e_sum, hom, obs = [0] * n, [0] * n, [0] * n
    used = np.zeros(v, dtype=np.uint8)
    for i in range(v):
        c = codes[i]
        het, alt, called = int((c == 1).sum()), int((c == 2).sum()), int((c != 3).sum())
        e = expected(het, alt, called, None if freq is None else float(freq[i]), small_sample and freq is None)
        if e is None:
            continue
        used[i] = 1
        q = fixed(e, k)
        for s in np.flatnonzero(c != 3):
            e_sum[s] += q
            obs[s] += 1
        for s in np.flatnonzero((c == 0) | (c == 2)):
            hom[s] += 1
    rows = np.zeros(n, dtype=ROW_DTYPE)
    for s in range(n):
        e_hom = math.ldexp(float(e_sum[s]), -k)
        den = float(obs[s]) - e_hom
        f = NAN if obs[s] == 0 or den == 0.0 else (float(hom[s]) - e_hom) / den
        rows[s] = (e_hom, f, e_sum[s], hom[s], obs[s])
    return rows, used, int(used.sum())


def empty_rows(n):
    """What n_var == 0 and a call without a used variant give: {0.0, NaN, 0, 0, 0}."""
    rows = np.zeros(n, dtype=ROW_DTYPE)
    rows["f"] = NAN
    return rows


def same_rows(got, want):
    """Every field of every row, bit for bit."""
    if got.shape != want.shape:
        return False
    return all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).astype(ROW_DTYPE[f]).tobytes()
               for f in FIELDS)
