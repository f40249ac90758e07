"""pgh_ld_scores / pgh_ld_r2 (Dataset.ld_scores, lib.ld_r2): windowed LD scores from the int8 band kernel.

The yardstick is brute force written here, from the 2-bit codes the test itself wrote with pgen_writer: the C / G / Q
planes multiplied as int64, the header's term formula one IEEE operation at a time, and math.fsum over each variant's
terms.  n_partners must be equal to the brute force; a score must be within the summation bound

    |got - fsum(terms)| <= T * 2^-52 * sum |term|        (T terms, the self term included)

which the test computes per variant: every term is bit-identical to the formula, so only the order of the T additions
differs (any order is within (T - 1) 2^-53 sum |term| to first order, and fsum is within 2^-53 of the true sum)."""

import ctypes as C
import math
import os
import threading

import numpy as np
import pytest

from conftest import ROOT, data_path

import pgen_writer as W

C_OF = np.array([1, 1, 1, 0], dtype=np.int64)
G_OF = np.array([0, 1, 2, 0], dtype=np.int64)
Q_OF = np.array([0, 1, 4, 0], dtype=np.int64)

# ---- the yardstick -----------------------------------------------------------------------------------------------


def py_term(sums, unbiased):
    """The header's formula in Python integers and floats; None when the pair is not defined."""
    n, sa, sb, sab, sa2, sb2 = (int(x) for x in sums)
    if n < (3 if unbiased else 2):
        return None
    num, va, vb = n * sab - sa * sb, n * sa2 - sa * sa, n * sb2 - sb * sb
    if va <= 0 or vb <= 0:
        return None
    dn = float(num)
    top = dn * dn
    bottom = float(va) * float(vb)
    r2 = top / bottom
    if not unbiased:
        return r2
    rest = 1.0 - r2
    adj = rest / float(n - 2)
    return r2 - adj


def brute_sums(codes):
    """(6, V, V) int64 from (V, N) codes: n, sum_a, sum_b, sum_ab, sum_a2, sum_b2 of every pair."""
    c, g, q = C_OF[codes], G_OF[codes], Q_OF[codes]
    return np.stack([c @ c.T, g @ c.T, c @ g.T, g @ g.T, q @ c.T, c @ q.T])


def term_matrix(s, unbiased):
    """(defined, term) of every pair of a brute_sums block; the formula, elementwise, one operation a statement."""
    n, sa, sb, sab, sa2, sb2 = s
    num, va, vb = n * sab - sa * sb, n * sa2 - sa * sa, n * sb2 - sb * sb
    ok = (n >= (3 if unbiased else 2)) & (va > 0) & (vb > 0)
    with np.errstate(all="ignore"):
        dn = num.astype(np.float64)
        top = dn * dn
        bottom = va.astype(np.float64) * vb.astype(np.float64)
        term = top / bottom
        if unbiased:
            rest = 1.0 - term
            adj = rest / (n - 2).astype(np.float64)
            term = term - adj
    term[~ok] = 0.0
    return ok, term


def self_terms(codes, unbiased):
    called = (codes != 3).sum(axis=1)
    het, alt = (codes == 1).sum(axis=1), (codes == 2).sum(axis=1)
    out = np.zeros(len(codes))
    for k in range(len(codes)):
        s1, s2 = het[k] + 2 * alt[k], het[k] + 4 * alt[k]
        out[k] = 0.0 if py_term((called[k], s1, s1, s2, s2, s2), unbiased) is None else 1.0
    return out


def band_mask(win_end):
    v = len(win_end)
    u = np.arange(v)
    return (u[None, :] > u[:, None]) & (u[None, :] < np.asarray(win_end, dtype=np.int64)[:, None])


def brute_scores(codes, win_end, unbiased):
    """(fsum score, bound, n_partners) per variant, exactly the definition."""
    ok, term = term_matrix(brute_sums(codes), unbiased)
    use = band_mask(win_end) & ok
    use = use | use.T  # a band pair counts for both of its variants
    selfs = self_terms(codes, unbiased)
    v = len(codes)
    score, bound = np.zeros(v), np.zeros(v)
    for k in range(v):
        # term(j, k) for j < k is read at [j, k]: the anchor is the row
        terms = [selfs[k]] + term[k, use[k] & (np.arange(v) > k)].tolist() + term[use[:, k] & (np.arange(v) < k), k].tolist()
        score[k] = math.fsum(terms)
        bound[k] = len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
    return score, bound, use.sum(axis=1).astype(np.uint32)


def check_against_brute(got, codes, win_end, unbiased):
    score, partners = got
    exp, bound, exp_n = brute_scores(codes, win_end, unbiased)
    assert score.dtype == np.float64 and partners.dtype == np.uint32
    assert score.shape == exp.shape and partners.shape == exp_n.shape
    assert np.array_equal(partners, exp_n)
    err = np.abs(score - exp)
    worst = int(np.argmax(err - bound))
    print(f"largest error {err.max():.3e}; variant {worst}: error {err[worst]:.3e}, bound {bound[worst]:.3e}, "
          f"score {exp[worst]:.6f}, partners {exp_n[worst]}")
    assert (err <= bound).all(), (worst, score[worst], exp[worst], bound[worst])
    return exp, exp_n


def windows(n_var, w):
    return np.minimum(np.arange(n_var) + w, n_var).astype(np.uint32)


def ld_codes(rng, v, n, missing):
    """Genotypes with LD structure: two haplotypes per sample, each with a latent uniform that is redrawn with
    probability 0.1 per variant; the allele of variant k is u < p_k, p_k ~ U(0.05, 0.5); independent missingness."""
    p = rng.uniform(0.05, 0.5, v)
    u = rng.random(2 * n)
    codes = np.zeros((v, n), dtype=np.uint8)
    for k in range(v):
        redraw = rng.random(2 * n) < 0.1
        u = np.where(redraw, rng.random(2 * n), u)
        allele = (u < p[k]).astype(np.uint8)
        codes[k] = allele[:n] + allele[n:]
    if missing:
        codes[rng.random((v, n)) < missing] = 3
    return codes


def pack_rows(codes):
    """codes: (V, N) uint8 in 0..3 -> the 2-bit rows Dataset.from_host_rows takes."""
    v, n = codes.shape
    padded = np.zeros((v, (n + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def open_codes(L, tmp, name, codes):
    path = str(tmp / (name + ".pgen"))
    W.write_pgen(path, codes, [0] * len(codes))
    return L.Dataset.open(path)


# ---- no device ---------------------------------------------------------------------------------------------------

LD_SCORE_SYMBOLS = ("pgh_ld_scores", "pgh_ld_r2")


def test_header_declares_and_library_exports_ld_scores(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in LD_SCORE_SYMBOLS:
        assert name + "(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "PGH_LDSCORE_UNBIASED = 1" in header and lib.LDSCORE_UNBIASED == 1
    assert lib.LD_SCORE_CHUNK_ENV in header
    assert "ldsc --l2" in header  # says that the definition has not been compared with ldsc's output


def test_ld_r2_is_the_formula(lib):
    same = (6, 6, 6, 10, 10, 10)   # two identical variants 0,0,1,1,2,2: r = 1
    flip = (6, 6, 6, 2, 10, 10)    # 0,0,1,1,2,2 against 2,2,1,1,0,0: r = -1
    edge = [
        (0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 1, 1),          # n = 0, 1: never
        (2, 1, 1, 1, 1, 1), (2, 1, 1, 0, 1, 1),          # n = 2: r2 = 1 plain, undefined unbiased
        (3, 1, 1, 1, 1, 1), (3, 2, 1, 1, 2, 1), (3, 3, 1, 1, 5, 1),  # n = 3
        (10, 10, 7, 7, 10, 9), (10, 7, 20, 14, 9, 40),  # va = 0; vb = 0
        same, flip, (8, 4, 4, 3, 4, 4), (8, 4, 4, 1, 4, 4),
    ]
    for s in edge:
        for unbiased in (False, True):
            assert lib.ld_r2(s, unbiased) == py_term(s, unbiased), (s, unbiased)
    assert lib.ld_r2((0, 0, 0, 0, 0, 0)) is None and lib.ld_r2((1, 1, 1, 1, 1, 1)) is None
    assert lib.ld_r2((10, 10, 7, 7, 10, 9)) is None and lib.ld_r2((10, 7, 20, 14, 9, 40), True) is None
    assert lib.ld_r2((2, 1, 1, 1, 1, 1)) == 1.0 and lib.ld_r2((2, 1, 1, 1, 1, 1), True) is None
    assert lib.ld_r2((3, 1, 1, 1, 1, 1), True) == 1.0
    assert lib.ld_r2(same) == 1.0 and lib.ld_r2(flip) == 1.0 and lib.ld_r2(same, True) == 1.0
    assert lib.ld_r2((8, 4, 4, 3, 4, 4)) == 0.25 and lib.ld_r2((8, 4, 4, 3, 4, 4), True) == 0.125
    # random consistent sums up to the largest the entry points can return (n = 2^29 - 1)
    rng = np.random.default_rng(12)
    checked = defined = 0
    for n in (2, 3, 4, 17, 1000, 2 ** 20 + 1, 2 ** 29 - 1):
        for _ in range(400):
            ga = rng.integers(0, 3, size=min(n, 64))
            gb = np.where(rng.random(len(ga)) < 0.7, ga, rng.integers(0, 3, size=len(ga)))
            scale = n // len(ga)
            s = (scale * len(ga), scale * int(ga.sum()), scale * int(gb.sum()), scale * int((ga * gb).sum()),
                 scale * int((ga * ga).sum()), scale * int((gb * gb).sum()))
            for unbiased in (False, True):
                got, exp = lib.ld_r2(s, unbiased), py_term(s, unbiased)
                assert got == exp, (s, unbiased, got, exp)
                checked += 1
                defined += exp is not None
    assert checked == 7 * 400 * 2 and defined > checked // 2
    # the raw entry point: NULL term is allowed, unknown flag bits are "not defined"
    raw = lib.raw()
    s = np.array(same, dtype=np.uint32)
    assert raw.pgh_ld_r2(s.ctypes.data_as(C.c_void_p), 0, None) == 1
    assert raw.pgh_ld_r2(s.ctypes.data_as(C.c_void_p), 2, None) == 0
    assert raw.pgh_ld_r2(None, 0, None) == 0
    with pytest.raises(ValueError):
        lib.ld_r2((1, 2, 3))
    with pytest.raises(ValueError):
        lib.ld_r2(np.zeros((2, 6), dtype=np.uint32))


def test_brute_force_of_this_file_on_a_hand_case():
    """The yardstick itself, on four variants worked by hand (needs neither the device nor the new symbols)."""
    a = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint8)
    codes = np.stack([a, a, 2 - a, np.zeros(6, dtype=np.uint8)])
    score, bound, n = brute_scores(codes, windows(4, 4), False)
    assert score.tolist() == [3.0, 3.0, 3.0, 0.0] and n.tolist() == [2, 2, 2, 0]
    score, bound, n = brute_scores(codes, windows(4, 2), False)
    assert score.tolist() == [2.0, 3.0, 2.0, 0.0] and n.tolist() == [1, 2, 1, 0]
    assert (bound[:3] > 0).all() and bound[3] == 0.0


# ---- on the GPU --------------------------------------------------------------------------------------------------

V, N = 300, 130
BREAKS = (96, 128, 192, 256)


@pytest.fixture(scope="module")
def small(gpu_lib, tmp_path_factory):
    """130 samples (two K-steps and a 2-sample tail) x 300 variants (more than three anchor tile rows of 96 and two
    partner tiles of 128, neither ending on a tile edge), 10 % missing, with the special variants on tile edges."""
    L = gpu_lib
    assert V > 3 * L.LD_TILE_A and V > 2 * L.LD_TILE_B and V % L.LD_TILE_A and V % L.LD_TILE_B and N % 64 == 2
    rng = np.random.default_rng(20261018)
    codes = ld_codes(rng, V, N, 0.10)
    codes[96] = codes[95]                                   # a duplicate across an anchor tile edge: r2 = 1
    codes[128] = np.where(codes[127] == 3, 3, 2 - codes[127])  # a complement across a partner tile edge: r = -1
    codes[191] = np.where(codes[191] == 3, 3, 0)            # monomorphic
    codes[256] = 3                                          # all missing
    ds = open_codes(L, tmp_path_factory.mktemp("ld_scores"), "small", codes)
    assert ds.n_samples == N and ds.v_end == V
    mask = rng.random(N) < 0.6
    vidx = np.union1d(rng.permutation(V)[:207], [95, 96, 127, 128]).astype(np.uint32)  # sorted, the special pairs in
    assert 2 * L.LD_TILE_A < len(vidx) < V
    chrom = np.searchsorted(np.array(BREAKS), np.arange(V), side="right")
    pos = np.concatenate([np.sort(rng.integers(0, 400_000, int((chrom == c).sum()))) for c in range(len(BREAKS) + 1)])
    ss = ds.subset(mask)
    yield {"ds": ds, "codes": codes, "mask": mask, "ss": ss, "vidx": vidx, "chrom": chrom, "pos": pos}
    ss.close()
    ds.close()


def route(small, how):
    """(the codes the call sees, its keyword arguments)"""
    codes, kw = small["codes"], {}
    if how in ("subset", "both"):
        codes, kw["subset"] = codes[:, small["mask"]], small["ss"]
    if how in ("vidx", "both"):
        codes, kw["vidx"] = codes[small["vidx"]], small["vidx"]
    return codes, kw


def window_of(L, small, how, which):
    sel = small["vidx"] if how in ("vidx", "both") else np.arange(V)
    n = len(sel)
    if which == "ragged":
        win = L.ld_windows(small["chrom"][sel], small["pos"][sel], 60)
        assert len(set((win - np.arange(n)).tolist())) > 10  # ragged
        if n == V:
            assert all(win[b - 1] == b for b in BREAKS)      # the breaks sit exactly on 96, 128, 192 and 256
        return win
    return windows(n, {"one": 1, "fifty": 50, "full": n}[which])


@pytest.mark.gpu
@pytest.mark.parametrize("unbiased", [False, True])
@pytest.mark.parametrize("how", ["plain", "subset", "vidx", "both"])
@pytest.mark.parametrize("which", ["one", "fifty", "full", "ragged"])
def test_scores_equal_brute_force(small, gpu_lib, which, how, unbiased):
    ds = small["ds"]
    codes, kw = route(small, how)
    win = window_of(gpu_lib, small, how, which)
    got = ds.ld_scores(win_end=win, unbiased=unbiased, want_counts=True, **kw)
    exp, exp_n = check_against_brute(got, codes, win, unbiased)
    selfs = self_terms(codes, unbiased)
    if which == "one":
        assert not exp_n.any() and np.array_equal(got[0], selfs)  # no partners: the score is the self term
    else:
        assert exp_n.max() > 0 and (exp != selfs).any()
    if how == "plain":
        assert selfs[191] == 0.0 and selfs[256] == 0.0 and got[0][191] == 0.0 and got[0][256] == 0.0
        assert got[1][191] == 0 and got[1][256] == 0
        if which != "one" and not unbiased:
            # the duplicate and the complement each add exactly 1 to both of their variants
            _, term = term_matrix(brute_sums(codes), False)
            assert term[95, 96] == 1.0 and term[127, 128] == 1.0
    # the plain scores alone, and window= instead of win_end=
    assert np.array_equal(ds.ld_scores(win_end=win, unbiased=unbiased, **kw), got[0])
    if which != "ragged":
        w = {"one": 1, "fifty": 50, "full": len(win)}[which]
        again = ds.ld_scores(window=w, unbiased=unbiased, want_counts=True, **kw)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


@pytest.mark.gpu
def test_chunk_size_does_not_change_a_byte(small, gpu_lib, monkeypatch):
    ds = small["ds"]
    env = gpu_lib.LD_SCORE_CHUNK_ENV
    monkeypatch.delenv(env, raising=False)
    for kw in ({"window": 50}, {"window": V}, {"window": V, "unbiased": True, "subset": small["ss"]}):
        first = ds.ld_scores(want_counts=True, **kw)
        for chunk in ("1", "2", "7"):
            monkeypatch.setenv(env, chunk)
            got = ds.ld_scores(want_counts=True, **kw)
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), (kw, chunk)
        monkeypatch.delenv(env)


@pytest.mark.gpu
def test_determinism_threads_and_routes(small):
    ds = small["ds"]
    first = ds.ld_scores(window=V, want_counts=True)
    again = ds.ld_scores(window=V, want_counts=True)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    out, errors = [], []

    def worker():
        try:
            out.append(ds.ld_scores(window=V, want_counts=True))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=worker)
    th.start()
    th.join()
    assert not errors, errors
    assert out[0][0].tobytes() == first[0].tobytes() and out[0][1].tobytes() == first[1].tobytes()
    # the range form and the list form of the same variants
    listed = ds.ld_scores(window=V, want_counts=True, vidx=np.arange(V, dtype=np.uint32))
    assert listed[0].tobytes() == first[0].tobytes() and listed[1].tobytes() == first[1].tobytes()
    part = ds.ld_scores(window=40, want_counts=True, v_begin=37, v_end=260)
    listed = ds.ld_scores(window=40, want_counts=True, vidx=np.arange(37, 260, dtype=np.uint32))
    assert listed[0].tobytes() == part[0].tobytes() and listed[1].tobytes() == part[1].tobytes()
    check_against_brute(part, small["codes"][37:260], windows(223, 40), False)


def tile_order_scores(L, terms, selfs, win_end):
    """The documented order of the sum, on the host: terms[k, u] is the term of the band pair (k, u), 0.0 elsewhere.
    Tiles of 96 x 128 by anchor tile row, then partner tile; each adds its row sums, then its column sums."""
    v = len(selfs)
    ta_n, tb_n = L.LD_TILE_A, L.LD_TILE_B
    score = selfs.astype(np.float64).copy()
    for k0 in range(0, v, ta_n):
        k_last = min(k0 + ta_n, v) - 1
        lo, hi = k0 + 1, int(win_end[k_last])
        if lo >= hi:
            continue
        for tb in range(lo // tb_n, (hi - 1) // tb_n + 1):
            b0 = tb * tb_n
            m = np.zeros((ta_n, tb_n))
            blk = terms[k0:k0 + ta_n, b0:b0 + tb_n]
            m[:blk.shape[0], :blk.shape[1]] = blk
            # rows: per wave column wc its two 16-column blocks, a butterfly over 16 lanes, then the waves in order
            w = m.reshape(ta_n, 4, 2, 16)
            x = w[:, :, 0, :] + w[:, :, 1, :]
            while x.shape[-1] > 1:
                x = x[..., 0::2] + x[..., 1::2]
            x = x[..., 0]
            rows = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
            # columns: per wave row wr (48 anchors) and row group q the 12 rows 16 x + 4 q + reg in (x, reg) order,
            # then (q0 + q1) + (q2 + q3), then the two waves
            c = m.reshape(2, 3, 4, 4, tb_n)  # wr, x, q, reg, column
            acc = np.zeros((2, 4, tb_n))
            for xb in range(3):
                for reg in range(4):
                    acc = acc + c[:, xb, :, reg, :]
            per_wave = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
            cols = per_wave[0] + per_wave[1]
            na, nb = min(ta_n, v - k0), min(tb_n, v - b0)
            score[k0:k0 + na] += rows[:na]
            score[b0:b0 + nb] += cols[:nb]
    return score


@pytest.mark.gpu
@pytest.mark.parametrize("unbiased", [False, True])
def test_documented_order_of_the_sum_from_window_sums(small, gpu_lib, unbiased):
    """ld_window_sums' planes through lib.ld_r2, added on the host in the documented order: bit equality."""
    L = gpu_lib
    ds, codes = small["ds"], small["codes"]
    planes = ds.ld_window_sums()
    win = windows(V, V)
    terms = np.zeros((V, V))
    count = np.zeros(V, dtype=np.uint32)
    for k in range(V):
        for u in range(k + 1, int(win[k])):
            t = L.ld_r2(planes[:, k, u], unbiased)
            if t is not None:
                terms[k, u] = t
                count[k] += 1
                count[u] += 1
    selfs = np.array([0.0 if L.ld_r2([planes[p, k, k] for p in range(6)], unbiased) is None else 1.0 for k in range(V)])
    assert np.array_equal(selfs, self_terms(codes, unbiased))
    exp = tile_order_scores(L, terms, selfs, win)
    got = ds.ld_scores(win_end=win, unbiased=unbiased, want_counts=True)
    assert np.array_equal(got[1], count)
    assert got[0].tobytes() == exp.tobytes()
    assert len(set(np.round(got[0], 9).tolist())) > V // 2  # scores with structure, not a constant


@pytest.mark.gpu
def test_wider_case(gpu_lib, tmp_path):
    v, n, window = 200, 1000, 64
    codes = ld_codes(np.random.default_rng(9), v, n, 0.05)
    ds = open_codes(gpu_lib, tmp_path, "wide", codes)
    for unbiased in (False, True):
        got = ds.ld_scores(window=window, unbiased=unbiased, want_counts=True)
        exp, exp_n = check_against_brute(got, codes, windows(v, window), unbiased)
        assert exp_n.min() >= window - 1 and exp.max() > 2.0
    ds.close()


@pytest.mark.gpu
def test_unbiased_needs_three_samples(small):
    ds = small["ds"]
    mask = np.zeros(N, dtype=bool)
    mask[[3, 77]] = True
    ss = ds.subset(mask)
    score, partners = ds.ld_scores(window=V, unbiased=True, want_counts=True, subset=ss)
    assert not score.any() and not partners.any()
    ss.close()


@pytest.mark.gpu
def test_refusals(small, gpu_lib):
    L = gpu_lib
    ds, codes = small["ds"], small["codes"]
    ok = windows(V, 10)
    bad = ok.copy()
    bad[5] = bad[4] - 1  # decreasing (and still > 5)
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_scores(win_end=bad)
    bad = ok.copy()
    bad[:8] = 7  # win_end[7] <= 7
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_scores(win_end=bad)
    bad = ok.copy()
    bad[-1] = V + 1
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_scores(win_end=bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        ds.ld_scores(window=3, vidx=np.array([1, 5, 5, 9], dtype=np.uint32))
    with pytest.raises(ValueError, match="strictly increasing"):
        ds.ld_scores(window=3, vidx=np.array([1, 9, 5], dtype=np.uint32))
    with pytest.raises(ValueError, match="exactly one"):
        ds.ld_scores()
    with pytest.raises(ValueError, match="exactly one"):
        ds.ld_scores(win_end=ok, window=10)
    with pytest.raises(ValueError, match="one unsigned 32-bit value per variant"):
        ds.ld_scores(win_end=ok[:-1])
    with pytest.raises(ValueError, match="n_var"):
        ds.ld_scores(window=3, v_begin=5, v_end=5)
    with pytest.raises(ValueError, match="variant index"):
        ds.ld_scores(window=3, vidx=np.array([0, V], dtype=np.uint32))
    # a flag bit that is not defined, through the raw entry point (the binding only knows `unbiased`)
    score = np.zeros(V)
    eb = C.create_string_buffer(512)
    for flags in (2, 3, 1 << 31):
        rc = L.raw().pgh_ld_scores(ds._h, None, 0, V, None, ok.ctypes.data_as(C.c_void_p), flags,
                                   score.ctypes.data_as(C.c_void_p), None, eb)
        assert rc == L.PGH_ERR_ARG and b"flag" in eb.value
    assert not score.any()
    sp = L.Dataset.open(data_path("rare_small.pgen"), sparse=True)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.ld_scores(window=3)
    sp.close()
    group = L.Dataset.group([L.Dataset.from_host_rows(pack_rows(codes[:10]), N)])
    with pytest.raises(ValueError, match="one device's dataset"):
        group.ld_scores(window=3)
    group.close()
