"""pgh_ld_window_sums / pgh_ld_prune / pgh_ld_exceeds (Dataset.ld_window_sums, Dataset.ld_prune, lib.ld_exceeds,
lib.ld_windows): the six r2 sums of variant pairs on the int8 matrix cores, and greedy LD pruning over a band.

The yardstick is brute force written here: the C / G / Q planes of the 2-bit codes the dataset was made from,
multiplied as int64, then the header's formula and its sequential loop exactly as written.  Sums and keep arrays are
compared with np.array_equal, never with a tolerance."""

import ctypes as C
import math
import os
import threading

import numpy as np
import pytest

from conftest import ROOT, data_path

# ---- the yardstick -----------------------------------------------------------------------------------------------


def pack_rows(codes):
    """codes: (V, N) uint8 in 0..3 -> the 2-bit rows Dataset.from_host_rows takes (sample s in bits 2 (s % 4) of byte
    s // 4)."""
    v, n = codes.shape
    padded = np.zeros((v, (n + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def unpack_rows(rows, n):
    shifts = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((rows[:, :, None] >> shifts) & 3).reshape(rows.shape[0], -1)[:, :n].astype(np.uint8)


C_OF = np.array([1, 1, 1, 0], dtype=np.int64)
G_OF = np.array([0, 1, 2, 0], dtype=np.int64)
Q_OF = np.array([0, 1, 4, 0], dtype=np.int64)


def brute_sums(codes, a=None, b=None):
    """(6, na, nb) int64 from (V, N) codes: n, sum_a, sum_b, sum_ab, sum_a2, sum_b2 of variants a x b."""
    v = codes.shape[0]
    a = np.arange(v) if a is None else np.asarray(a)
    b = np.arange(v) if b is None else np.asarray(b)
    ca, ga, qa = C_OF[codes[a]], G_OF[codes[a]], Q_OF[codes[a]]
    cb, gb, qb = C_OF[codes[b]].T, G_OF[codes[b]].T, Q_OF[codes[b]].T
    return np.stack([ca @ cb, ga @ cb, ca @ gb, ga @ gb, qa @ cb, ca @ qb])


def py_exceeds(sums, t):
    """The issue's formula in Python integers and floats."""
    n, sa, sb, sab, sa2, sb2 = (int(x) for x in sums)
    num, va, vb = n * sab - sa * sb, n * sa2 - sa * sa, n * sb2 - sb * sb
    if n < 2 or va <= 0 or vb <= 0:
        return False
    return (float(num) * float(num)) / (float(va) * float(vb)) > t


def r2_matrix(s):
    """float64 r2 of every pair of a brute_sums block by the formula, NaN where the pair never exceeds."""
    n, sa, sb, sab, sa2, sb2 = s
    num, va, vb = n * sab - sa * sb, n * sa2 - sa * sa, n * sb2 - sb * sb
    ok = (n >= 2) & (va > 0) & (vb > 0)
    with np.errstate(all="ignore"):
        r2 = (num.astype(np.float64) * num.astype(np.float64)) / (va.astype(np.float64) * vb.astype(np.float64))
    r2[~ok] = np.nan
    return r2


def maf_keys(codes):
    """(mc, obs) per variant as Python-int friendly int64 arrays."""
    alt = (codes == 1).sum(axis=1).astype(np.int64) + 2 * (codes == 2).sum(axis=1).astype(np.int64)
    obs = 2 * (codes != 3).sum(axis=1).astype(np.int64)
    return np.minimum(alt, obs - alt), obs


def prune_loop(exc, win_end, mc, obs):
    """The header's sequential rule.  exc[k, u]: the pair exceeds."""
    n_var = len(win_end)
    keep = np.ones(n_var, dtype=bool)
    for k in range(n_var):
        if not keep[k]:
            continue
        for u in range(k + 1, int(win_end[k])):
            if keep[u] and exc[k, u]:
                if int(mc[k]) * int(obs[u]) < int(mc[u]) * int(obs[k]):
                    keep[k] = False
                    break
                keep[u] = False  # ties remove the later variant
    return keep


def brute_prune(codes, win_end, t, near=None):
    r2 = r2_matrix(brute_sums(codes))
    if near is not None:
        band = np.zeros_like(r2, dtype=bool)
        for k in range(len(win_end)):
            band[k, k + 1:int(win_end[k])] = True
        assert not (np.abs(r2[band & ~np.isnan(r2)] - t) <= near).any(), "a band pair sits on the threshold: reseed"
    with np.errstate(invalid="ignore"):
        exc = r2 > t  # NaN: never
    mc, obs = maf_keys(codes)
    return prune_loop(exc, win_end, mc, obs)


def windows(n_var, w):
    return np.minimum(np.arange(n_var) + w, n_var).astype(np.uint32)


def random_codes(rng, v, n, missing):
    p = rng.uniform(0.05, 0.5, v)[:, None]
    codes = rng.binomial(2, p, size=(v, n)).astype(np.uint8)
    if missing:
        codes[rng.random((v, n)) < missing] = 3
    return codes


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


def pairs_from_planes(planes, a, b):
    """(len(a), 6) rows in ld_pairs' layout from (6, na, nb) planes."""
    return np.stack([planes[p][a, b] for p in range(6)], axis=1)


# ---- no device ---------------------------------------------------------------------------------------------------

LD_SYMBOLS = ("pgh_ld_window_sums", "pgh_ld_prune", "pgh_ld_exceeds")


def test_header_declares_and_library_exports_ld_band(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in LD_SYMBOLS:
        assert name + "(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert (lib.LD_N, lib.LD_SUM_A, lib.LD_SUM_B, lib.LD_SUM_AB, lib.LD_SUM_A2, lib.LD_SUM_B2, lib.LD_PLANES) == \
        (0, 1, 2, 3, 4, 5, 6)
    assert lib.LD_PRUNE_CHUNK_ENV in header
    assert "indep-pairwise" in header  # says that the rule has not been compared with plink2's


def test_ld_exceeds_is_the_formula(lib):
    # n < 2: never, whatever the rest
    assert not lib.ld_exceeds((0, 0, 0, 0, 0, 0), 0.0)
    assert not lib.ld_exceeds((1, 1, 1, 1, 1, 1), 0.0)
    # va = 0 (a monomorphic over the pair's samples) and vb = 0
    assert not lib.ld_exceeds((10, 10, 7, 7, 10, 9), 0.0)
    assert not lib.ld_exceeds((10, 7, 20, 14, 9, 40), 0.0)
    # two identical variants 0,0,1,1,2,2: r2 = 1 exactly
    same = (6, 6, 6, 10, 10, 10)
    assert py_exceeds(same, 0.999999) and lib.ld_exceeds(same, 0.999999)
    assert not lib.ld_exceeds(same, 1.0)
    # exactly at the threshold is not "exceeds"
    exact = (8, 4, 4, 3, 4, 4)  # num = 8, va = 16, vb = 16: r2 = 64 / 256 = 0.25
    assert (8 * 3 - 16, 8 * 4 - 16) == (8, 16)
    assert not py_exceeds(exact, 0.25) and not lib.ld_exceeds(exact, 0.25)
    assert py_exceeds(exact, math.nextafter(0.25, 0.0)) and lib.ld_exceeds(exact, math.nextafter(0.25, 0.0))
    # a negative correlation exceeds like a positive one
    neg = (8, 4, 4, 1, 4, 4)
    assert py_exceeds(neg, 0.2) and lib.ld_exceeds(neg, 0.2)
    # a grid up to the largest sums the entry points can return (n = 2^29 - 1)
    top = 2 ** 29 - 1
    rng = np.random.default_rng(11)
    checked = 0
    for n in (2, 3, 17, 1000, 2 ** 20 + 1, top):
        for _ in range(300):
            ga = rng.integers(0, 3, size=min(n, 64))
            gb = np.where(rng.random(len(ga)) < 0.7, ga, rng.integers(0, 3, size=len(ga)))
            scale = n // len(ga)
            s = (scale * len(ga), scale * int(ga.sum()), scale * int(gb.sum()), scale * int((ga * gb).sum()),
                 scale * int((ga * ga).sum()), scale * int((gb * gb).sum()))
            for t in (0.0, 0.1, 0.5, 0.999, 1.0):
                assert lib.ld_exceeds(s, t) == py_exceeds(s, t), (s, t)
                checked += 1
    assert checked == 6 * 300 * 5
    with pytest.raises(ValueError):
        lib.ld_exceeds((1, 2, 3), 0.5)


def test_ld_windows_on_a_two_chromosome_map(lib):
    chrom = np.array(["1"] * 5 + ["2"] * 4)
    pos = np.array([100, 1100, 1101, 5000, 9000, 50, 60, 1050, 1051])
    got = lib.ld_windows(chrom, pos, 1)  # 1 kb: pos[u] - pos[k] <= 1000
    assert got.dtype == np.uint32
    assert got.tolist() == [2, 3, 3, 4, 5, 8, 9, 9, 9]
    # a window never crosses the boundary, however wide
    assert lib.ld_windows(chrom, pos, 1e6).tolist() == [5, 5, 5, 5, 5, 9, 9, 9, 9]
    # kb = 0: only variants at the same position
    assert lib.ld_windows(["1", "1", "1"], [7, 7, 8], 0).tolist() == [2, 2, 3]
    assert lib.ld_windows([], [], 5).tolist() == []
    # every window is valid input for ld_prune: k < win_end[k] <= n, not decreasing
    assert all(k < w <= len(got) for k, w in enumerate(got)) and (np.diff(got.astype(np.int64)) >= 0).all()
    with pytest.raises(ValueError, match="decrease"):
        lib.ld_windows(chrom, np.array([100, 99, 1101, 5000, 9000, 50, 60, 1050, 1051]), 1)
    with pytest.raises(ValueError, match="contiguous"):
        lib.ld_windows(["1", "2", "1"], [1, 2, 3], 1)
    with pytest.raises(ValueError):
        lib.ld_windows(["1", "1"], [1, 2, 3], 1)


def test_ld_generator_has_structure():
    """A sanity check of this file's own generator and brute force, not of the library (it needs neither the device nor
    the new symbols): the pruning inputs are not trivial -- the rule prunes some and keeps some, no pair on a cut."""
    codes = ld_codes(np.random.default_rng(20261017), 400, 70, 0.2)
    keep = brute_prune(codes, windows(400, 400), 0.8, near=1e-12)
    assert 0 < keep.sum() < 400


# ---- on the GPU: sums --------------------------------------------------------------------------------------------


def check_sums(ds, codes, **kw):
    got = ds.ld_window_sums(**kw)
    exp = brute_sums(codes)
    assert got.dtype == np.uint32 and got.shape == exp.shape
    assert np.array_equal(got, exp)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pgen_example", "pca_example", "rare_small", "large_example"])
def test_fixture_files_sums(gpu_lib, name):
    ds = gpu_lib.Dataset.open(data_path(name + ".pgen"))
    n = ds.n_samples
    m = min(ds.v_end, 400)
    codes = unpack_rows(ds.copy_rows_to_host(0, m), n)
    got = check_sums(ds, codes, v_begin=0, v_end=m)
    a, b = np.triu_indices(m, 0)
    assert np.array_equal(ds.ld_pairs(a, b), pairs_from_planes(got, a, b))
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("missing", [0.0, 0.2])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 4099])
@pytest.mark.parametrize("v", [1, 15, 16, 127, 128, 129, 300])
def test_sums_at_tile_and_padding_edges(gpu_lib, v, n, missing):
    assert 300 > 2 * gpu_lib.LD_TILE_B and 300 > 3 * gpu_lib.LD_TILE_A
    rng = np.random.default_rng(100000 * v + 10 * n + int(missing * 5))
    codes = random_codes(rng, v, n, missing)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    check_sums(ds, codes)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 255, 257])
def test_padding_is_not_called_not_hom_ref(gpu_lib, n):
    """All hom-ref: n is the sample count, not the count rounded up to the K-step or the row's padding."""
    v = 131
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(np.zeros((v, n), dtype=np.uint8)), n)
    got = ds.ld_window_sums()
    assert np.array_equal(got[gpu_lib.LD_N], np.full((v, v), n, dtype=np.uint32))
    assert not got[1:].any()
    ds.close()


@pytest.fixture(scope="module")
def square(gpu_lib):
    v, n = 700, 333
    codes = ld_codes(np.random.default_rng(77), v, n, 0.03)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    yield ds, codes, brute_sums(codes)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ar,br", [((0, 100), (400, 700)), ((100, 300), (200, 400)), ((5, 6), (0, 700)),
                                   ((699, 700), (699, 700)), ((130, 131), (17, 18)), ((95, 289), (1, 129)),
                                   ((300, 700), (0, 50)), ((0, 700), (0, 700))])
def test_rectangles_and_the_diagonal(square, gpu_lib, ar, br):
    ds, codes, full = square
    got = ds.ld_window_sums(a_range=ar, b_range=br)
    assert got.shape == (6, ar[1] - ar[0], br[1] - br[0])
    assert np.array_equal(got, full[:, ar[0]:ar[1], br[0]:br[1]])
    if ar == br == (0, 700):
        L = gpu_lib
        assert np.array_equal(got[L.LD_N], got[L.LD_N].T) and np.array_equal(got[L.LD_SUM_AB], got[L.LD_SUM_AB].T)
        assert np.array_equal(got[L.LD_SUM_A], got[L.LD_SUM_B].T) and np.array_equal(got[L.LD_SUM_A2], got[L.LD_SUM_B2].T)
        assert np.array_equal(np.diagonal(got[L.LD_N]), (codes != 3).sum(axis=1))
        assert np.array_equal(np.diagonal(got[L.LD_SUM_AB]), np.diagonal(got[L.LD_SUM_A2]))


@pytest.mark.gpu
def test_sums_variant_list_subset_and_ld_pairs(square):
    ds, codes, full = square
    v, n = codes.shape
    rng = np.random.default_rng(5)
    vidx = rng.permutation(v)[:150].astype(np.uint32)  # unsorted on purpose: sums do not care
    assert np.array_equal(ds.ld_window_sums(vidx=vidx), full[:, vidx][:, :, vidx])
    assert np.array_equal(ds.ld_window_sums(v_begin=37, v_end=201), full[:, 37:201, 37:201])
    mask = rng.random(n) < 0.6
    ss = ds.subset(mask)
    sub = codes[:, mask]
    assert np.array_equal(ds.ld_window_sums(subset=ss), brute_sums(sub))
    got = ds.ld_window_sums(vidx=vidx, subset=ss, a_range=(3, 120), b_range=(10, 150))
    assert np.array_equal(got, brute_sums(sub, vidx[3:120], vidx[10:150]))
    # the same pairs through pgh_ld_pairs, with and without the subset
    a = rng.integers(0, v, 3000).astype(np.uint32)
    b = rng.integers(0, v, 3000).astype(np.uint32)
    assert np.array_equal(ds.ld_pairs(a, b), pairs_from_planes(full, a, b))
    assert np.array_equal(ds.ld_pairs(a, b, subset=ss), pairs_from_planes(brute_sums(sub), a, b))
    ss.close()


# ---- on the GPU: pruning -----------------------------------------------------------------------------------------

PRUNE_CASES = [(700, 333, 0.03, 50, 0.2), (700, 333, 0.03, 200, 0.5), (1500, 1001, 0.0, 300, 0.1),
               (400, 70, 0.2, 400, 0.8)]


@pytest.mark.gpu
@pytest.mark.parametrize("v,n,missing,window,t", PRUNE_CASES)
def test_prune_equals_brute_force(gpu_lib, v, n, missing, window, t):
    codes = ld_codes(np.random.default_rng(20261017), v, n, missing)
    exp = brute_prune(codes, windows(v, window), t, near=1e-12)
    print(f"{v} x {n}, window {window}, r2 {t}: brute force prunes {100 * (1 - exp.mean()):.1f} %")
    assert 0 < exp.sum() < v
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    got = ds.ld_prune(t, window=window)
    assert got.dtype == bool and np.array_equal(got, exp)
    assert np.array_equal(ds.ld_prune(t, win_end=windows(v, window)), exp)
    ds.close()


@pytest.fixture(scope="module")
def pruned(gpu_lib):
    v, n = 900, 210
    codes = ld_codes(np.random.default_rng(20261017), v, n, 0.03)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    yield ds, codes
    ds.close()


@pytest.mark.gpu
def test_prune_windows_from_a_map(pruned, gpu_lib):
    ds, codes = pruned
    v = codes.shape[0]
    rng = np.random.default_rng(8)
    chrom = np.array([1] * 500 + [2] * (v - 500))
    pos = np.concatenate([np.sort(rng.integers(0, 400_000, 500)), np.sort(rng.integers(0, 300_000, v - 500))])
    win = gpu_lib.ld_windows(chrom, pos, 100)
    assert win[499] == 500 and win.max() == v and (win - np.arange(v)).max() > gpu_lib.LD_TILE_A
    exp = brute_prune(codes, win, 0.3, near=1e-12)
    assert 0 < exp.sum() < v
    assert np.array_equal(ds.ld_prune(0.3, win_end=win), exp)


@pytest.mark.gpu
def test_prune_window_and_threshold_extremes(pruned):
    ds, codes = pruned
    v = codes.shape[0]
    assert ds.ld_prune(0.2, window=1).all()  # a window of 1 holds no partner
    for window, t in [(v, 0.2), (v + 1000, 0.5), (2, 0.2), (60, 0.0), (60, 1.0)]:
        exp = brute_prune(codes, windows(v, window), t)
        assert np.array_equal(ds.ld_prune(t, window=window), exp), (window, t)
        if t == 1.0:
            assert exp.all()  # r2 > 1 never happens with 3 % of the calls missing at random
        else:
            assert 0 < exp.sum() < v


@pytest.mark.gpu
def test_prune_subset_and_variant_list(pruned):
    ds, codes = pruned
    v, n = codes.shape
    rng = np.random.default_rng(4)
    mask = rng.random(n) < 0.6
    ss = ds.subset(mask)
    sub = codes[:, mask]
    exp = brute_prune(sub, windows(v, 80), 0.3)
    assert 0 < exp.sum() < v
    assert np.array_equal(ds.ld_prune(0.3, window=80, subset=ss), exp)
    vidx = np.sort(rng.permutation(v)[:611]).astype(np.uint32)
    exp = brute_prune(codes[vidx], windows(611, 80), 0.3)
    assert 0 < exp.sum() < 611
    assert np.array_equal(ds.ld_prune(0.3, window=80, vidx=vidx), exp)
    exp = brute_prune(sub[vidx], windows(611, 80), 0.3)
    assert np.array_equal(ds.ld_prune(0.3, window=80, vidx=vidx, subset=ss), exp)
    exp = brute_prune(codes[100:433], windows(333, 80), 0.3)
    assert np.array_equal(ds.ld_prune(0.3, window=80, v_begin=100, v_end=433), exp)
    ss.close()


@pytest.mark.gpu
def test_monomorphic_all_missing_and_maf_ties(gpu_lib):
    rng = np.random.default_rng(21)
    n = 120
    base = rng.binomial(2, 0.3, n).astype(np.uint8)
    rarer = base.copy()
    rarer[np.flatnonzero(base == 2)[:1]] = 1  # one ALT copy fewer, still r2 far above 0.5 with base
    assert rarer.sum() == base.sum() - 1 and base.sum() < n  # ALT is the minor allele of both
    mono = np.zeros(n, dtype=np.uint8)
    gone = np.full(n, 3, dtype=np.uint8)
    flipped = (2 - base).astype(np.uint8)  # the same minor-allele count on the other allele: a tie, r2 = 1
    codes = np.stack([base, mono, base, gone, flipped, rarer, base])
    exp = brute_prune(codes, windows(7, 7), 0.5)
    # 0 against 2: tie, the later goes; 0 against 4: tie; 0 against 5: 5 has the lower MAF and is the LATER one
    # here, so the anchor 0 is not the lower one and 5 goes; 6: tie
    assert exp.tolist() == [True, True, False, True, False, False, False]
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    assert np.array_equal(ds.ld_prune(0.5, window=7), exp)
    ds.close()
    # the anchor has the lower MAF: it is the one removed, and its later partners are then left alone
    codes = np.stack([rarer, base, mono, gone, base])
    exp = brute_prune(codes, windows(5, 5), 0.5)
    assert exp.tolist() == [False, True, True, True, False]
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    assert np.array_equal(ds.ld_prune(0.5, window=5), exp)
    ds.close()


@pytest.mark.gpu
def test_chunk_size_determinism_and_threads(pruned, gpu_lib):
    ds, codes = pruned
    v = codes.shape[0]
    exp = brute_prune(codes, windows(v, 300), 0.2)
    assert 0 < exp.sum() < v
    env = gpu_lib.LD_PRUNE_CHUNK_ENV
    assert env not in os.environ
    first = ds.ld_prune(0.2, window=300)
    assert np.array_equal(first, exp)
    try:
        for chunk in ("1", "2", "7"):
            os.environ[env] = chunk
            assert np.array_equal(ds.ld_prune(0.2, window=300), first), chunk
    finally:
        del os.environ[env]
    for _ in range(2):
        assert ds.ld_prune(0.2, window=300).tobytes() == first.tobytes()
    sums = ds.ld_window_sums().tobytes()
    assert ds.ld_window_sums().tobytes() == sums
    # four threads at once, each on its own stream
    results, errors = [None] * 4, []

    def worker(i):
        try:
            results[i] = (ds.ld_prune(0.2, window=300).tobytes(), ds.ld_window_sums().tobytes())
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert all(r == (first.tobytes(), sums) for r in results)


@pytest.mark.gpu
def test_refusals(pruned, gpu_lib):
    ds, codes = pruned
    v, n = codes.shape
    ok = windows(v, 10)
    bad = ok.copy()
    bad[5] = bad[4] - 1  # decreasing (and still > 5)
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_prune(0.2, win_end=bad)
    bad = ok.copy()
    bad[:8] = 7  # win_end[7] <= 7
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_prune(0.2, win_end=bad)
    bad = ok.copy()
    bad[-1] = v + 1
    with pytest.raises(ValueError, match="win_end"):
        ds.ld_prune(0.2, win_end=bad)
    with pytest.raises(ValueError, match="strictly increasing"):
        ds.ld_prune(0.2, window=3, vidx=np.array([1, 5, 5, 9], dtype=np.uint32))
    with pytest.raises(ValueError, match="strictly increasing"):
        ds.ld_prune(0.2, window=3, vidx=np.array([1, 9, 5], dtype=np.uint32))
    for t in (math.nan, 1.0000001, -0.1, math.inf):
        with pytest.raises(ValueError, match="r2_threshold"):
            ds.ld_prune(t, window=3)
    with pytest.raises(ValueError, match="exactly one"):
        ds.ld_prune(0.2)
    with pytest.raises(ValueError, match="exactly one"):
        ds.ld_prune(0.2, win_end=ok, window=10)
    with pytest.raises(ValueError, match="n_var"):
        ds.ld_prune(0.2, window=3, v_begin=5, v_end=5)
    with pytest.raises(ValueError, match="variant index"):
        ds.ld_prune(0.2, window=3, vidx=np.array([0, v], dtype=np.uint32))
    for ar, br in [((5, 5), (0, 3)), ((6, 5), (0, 3)), ((0, 3), (9, 2)), ((0, v + 1), (0, 3)), ((0, 3), (v, v + 1))]:
        with pytest.raises(ValueError, match="rectangle"):
            ds.ld_window_sums(a_range=ar, b_range=br)
    with pytest.raises(ValueError, match="range"):
        ds.ld_window_sums(v_begin=v - 2, v_end=v + 1)
    other = gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)
    ss = other.subset(np.ones(n, dtype=bool))
    with pytest.raises(ValueError, match="different dataset"):
        ds.ld_prune(0.2, window=3, subset=ss)
    ss.close()
    other.close()
    sp = gpu_lib.Dataset.open(data_path("rare_small.pgen"), sparse=True)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.ld_window_sums()
    with pytest.raises(ValueError, match="dense-resident"):
        sp.ld_prune(0.2, window=3)
    sp.close()
    group = gpu_lib.Dataset.group([gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)])
    with pytest.raises(ValueError, match="one device's dataset"):
        group.ld_window_sums()
    with pytest.raises(ValueError, match="one device's dataset"):
        group.ld_prune(0.2, window=3)
    group.close()


@pytest.mark.gpu
def test_wide_case_against_ld_pairs(gpu_lib):
    """500,000 samples: sums equal pgh_ld_pairs on a sample of pairs, and the keep array equals the rule run here
    from pgh_ld_pairs' sums over the band."""
    v, n, window = 260, 500_000, 30
    ds = gpu_lib.Dataset.synth(0, v, n, 20261017, 0.02)
    rng = np.random.default_rng(1)
    got = ds.ld_window_sums(a_range=(0, 200), b_range=(60, v))
    a = rng.integers(0, 200, 2000).astype(np.uint32)
    b = rng.integers(60, v, 2000).astype(np.uint32)
    assert np.array_equal(ds.ld_pairs(a, b), pairs_from_planes(got, a, b - 60))
    assert got[gpu_lib.LD_N].min() > 0.9 * n
    # unrelated synthetic variants: r2 is of the order of 1 / n, so the cut sits there
    t = 2e-6
    win = windows(v, window)
    ka = np.concatenate([np.full(int(win[k]) - k - 1, k) for k in range(v)]).astype(np.uint32)
    ub = np.concatenate([np.arange(k + 1, int(win[k])) for k in range(v)]).astype(np.uint32)
    sums = ds.ld_pairs(ka, ub)
    exc = np.zeros((v, v), dtype=bool)
    exc[ka, ub] = [py_exceeds(s, t) for s in sums]
    counts = ds.counts_range().astype(np.int64)
    alt, obs = counts[:, 1] + 2 * counts[:, 2], 2 * counts[:, :3].sum(axis=1)
    exp = prune_loop(exc, win, np.minimum(alt, obs - alt), obs)
    assert 0 < exp.sum() < v
    assert np.array_equal(ds.ld_prune(t, win_end=win), exp)
    ds.close()
