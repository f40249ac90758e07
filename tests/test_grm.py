"""pgh_grm / pgh_grm_standardize (Dataset.grm, lib.grm_standardize): the variance-standardised relationship matrix on
the FP64 matrix cores.

The yardstick is written here.  The codes the dataset was made from are unpacked; per variant, p = (het + 2 alt) /
(2 called) in Python integers and z[c] = (c - 2 p) / math.sqrt((2 p) (1 - p)), one variant at a time; Z is the
variants x samples matrix of those z (0 at a missing call), num = Z.T @ Z in float64, and nobs comes from boolean
planes as in test_king.py.

nobs is compared with np.array_equal.  rel is compared per entry with a derived bound, not a fitted one:

    |got * div - num| <= 2 (n_used + 16) 2^-53 S_ij + 2^-52 |num|        S = |Z|.T @ |Z|,  div the divisor

The first term is the classical bound for two sums of n_used products in any order (gamma_n ~ n 2^-53 each), the z a
few ulps from the exact ones; the second is the final division (and the product got * div taken here).

all-het padding case: the definition gives p = 0.5 and z[1] = (1 - 1) / s = 0 for a matrix of het calls, so rel is
exactly 0 there, not 1; rel == 1 exactly for every pair needs z[1] == 1, which the supplied frequency
P_Z1_IS_ONE gives ((1 - 2 p) and sqrt(2 p (1 - p)) round to the same double).  Both are asserted."""

import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT, data_path

# ---- the yardstick -----------------------------------------------------------------------------------------------


def pack_rows(codes):
    v, n = codes.shape
    padded = np.zeros((v, (n + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def unpack_rows(rows, n):
    shifts = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((rows[:, :, None] >> shifts) & 3).reshape(rows.shape[0], -1)[:, :n].astype(np.uint8)


def py_standardize(het, alt, called, p=None):
    """(p, [z0, z1, z2]) by the formula above, or (nan, None) for a skipped variant: nothing called, p not finite,
    p <= 0 or p >= 1."""
    if called == 0:
        return math.nan, None
    if p is None:
        p = (het + 2 * alt) / (2 * called)  # int / int: correctly rounded
    if not (math.isfinite(p) and 0.0 < p < 1.0):
        return math.nan, None
    q = 1.0 - p
    s = math.sqrt((2.0 * p) * q)
    return p, [(c - 2.0 * p) / s for c in (0.0, 1.0, 2.0)]


class Yardstick:
    """Z, num, S, nobs and n_used of (V, N) codes over the output samples `sel` (all when None)."""

    def __init__(self, codes, sel=None, freq=None):
        if sel is not None:
            codes = codes[:, sel]
        rows, used = [], []
        for k in range(codes.shape[0]):
            c = codes[k]
            het, alt, called = int((c == 1).sum()), int((c == 2).sum()), int((c != 3).sum())
            _, z = py_standardize(het, alt, called, None if freq is None else float(freq[k]))
            if z is not None:
                rows.append(np.array(z + [0.0])[c])
                used.append(k)
        n = codes.shape[1]
        self.used = np.array(used, dtype=np.int64)
        self.n_used = len(used)
        self.Z = np.array(rows, dtype=np.float64).reshape(self.n_used, n)
        self.num = self.Z.T @ self.Z
        self.S = np.abs(self.Z).T @ np.abs(self.Z)
        called = (codes[self.used] != 3).astype(np.float64).reshape(self.n_used, n)
        self.nobs = (called.T @ called).astype(np.uint32)


def bound(y):
    return 2.0 * (y.n_used + 16) * 2.0 ** -53 * y.S + 2.0 ** -52 * np.abs(y.num)


def check(rel, nobs, n_used, y, rows=None, cols=None, meanimpute=False):
    n = y.num.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    ix = np.ix_(rows, cols)
    assert n_used == y.n_used
    assert rel.dtype == np.float64 and nobs.dtype == np.uint32 and rel.shape == nobs.shape == (len(rows), len(cols))
    assert np.array_equal(nobs, y.nobs[ix])
    div = np.full(nobs.shape, float(y.n_used)) if meanimpute else nobs.astype(np.float64)
    nan = div == 0
    assert np.array_equal(np.isnan(rel), nan)
    err = np.abs(np.where(nan, 0.0, rel) * div - y.num[ix])
    lim = bound(y)[ix]
    worst = float((err / np.maximum(lim, 1e-300))[~nan].max(initial=0.0))
    print(f"grm check: n_used={y.n_used} pairs={rel.size} worst error / bound = {worst:.3f}")
    assert (err[~nan] <= lim[~nan]).all(), worst


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def random_codes(rng, v, n, missing):
    p = rng.uniform(0.05, 0.5, v)[:, None]
    codes = rng.binomial(2, p, size=(v, n)).astype(np.uint8)
    codes[rng.random((v, n)) < missing] = 3
    return codes


# (1 - 2 p) and sqrt((2 p) (1 - p)) are the same double: z[1] == 1.0 exactly
P_Z1_IS_ONE = float.fromhex("0x1.b0cb174df99c7p-3")

# ---- no device ---------------------------------------------------------------------------------------------------


def test_header_declares_and_library_exports_grm(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in ("pgh_grm", "pgh_grm_standardize"):
        assert name + "(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "PGH_GRM_MEANIMPUTE" in header
    assert lib.GRM_MEANIMPUTE == 1 and lib.GRM_TILE == 128 and lib.GRM_BAND_ENV == "PGH_GRM_BAND_BYTES"


def test_grm_standardize_is_the_formula_bit_for_bit(lib):
    top = 2 ** 31 - 1
    cases = []
    for called in (1, 2, 3, 7, 100, 12345, 2 ** 20 + 1, top - 1, top):
        hets = {0, 1, 2, called // 3, called // 2, called - 1, called}
        for het in sorted(h for h in hets if 0 <= h <= called):
            alts = {0, 1, (called - het) // 2, called - het - 1, called - het}
            for alt in sorted(a for a in alts if 0 <= a <= called - het):
                cases.append((het, alt, called))
    cases += [(1, 0, top), (0, 1, top), (0, top // 2, top - 1), (top - 1, 0, top - 1), (500, 250, 1000)]
    seen_half = seen_used = seen_skipped = 0
    for het, alt, called in cases:
        p, z = lib.grm_standardize(het, alt, called)
        ep, ez = py_standardize(het, alt, called)
        if ez is None:
            assert math.isnan(p) and z is None, (het, alt, called)
            seen_skipped += 1
            continue
        assert np.float64(p).tobytes() == np.float64(ep).tobytes(), (het, alt, called)
        assert z.tobytes() == np.array(ez, dtype=np.float64).tobytes(), (het, alt, called)
        seen_used += 1
        seen_half += p == 0.5
    assert seen_used > 100 and seen_skipped > 10 and seen_half > 5
    # singletons and all-het
    p, z = lib.grm_standardize(1, 0, top)
    assert p == 1 / (2 * top) and z[0] < 0 < z[1] < z[2]
    p, z = lib.grm_standardize(77, 0, 77)
    assert p == 0.5 and z[1] == 0.0 and z[0] == -z[2]
    assert py_standardize(5, 0, 5, P_Z1_IS_ONE)[1][1] == 1.0


def test_grm_standardize_skips(lib):
    for het, alt, called in [(0, 0, 0), (3, 4, 0), (0, 0, 5), (0, 0, 2 ** 31 - 1), (0, 5, 5), (0, 2 ** 31 - 1, 2 ** 31 - 1)]:
        z = np.full(3, 7.0)
        p = lib.raw().pgh_grm_standardize(het, alt, called, z.ctypes.data)
        assert math.isnan(p) and (z == 7.0).all(), (het, alt, called)


def test_bound_holds_for_a_permuted_float64_recomputation():
    """The bound is about summation order: numpy's own product over the variants in another order stays inside it."""
    for n, v, seed in [(300, 1000, 1), (257, 257, 2), (1000, 65, 3)]:
        rng = np.random.default_rng(seed)
        y = Yardstick(random_codes(rng, v, n, 0.03))
        perm = rng.permutation(y.n_used)
        again = y.Z[perm].T @ y.Z[perm]
        assert (np.abs(again - y.num) <= bound(y)).all()
        # and a sum taken one variant at a time, as a kernel's accumulator takes it
        serial = np.zeros_like(y.num[:40, :40])
        for k in range(y.n_used):
            serial += np.outer(y.Z[k, :40], y.Z[k, :40])
        assert (np.abs(serial - y.num[:40, :40]) <= bound(y)[:40, :40]).all()


# ---- on the GPU --------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pgen_example", "pca_example", "rare_small", "large_example"])
def test_fixture_files_full_square(gpu_lib, name):
    ds = gpu_lib.Dataset.open(data_path(name + ".pgen"))
    n = ds.n_samples
    codes = unpack_rows(ds.copy_rows_to_host(ds.v_begin, ds.v_end), n)
    y = Yardstick(codes)
    check(*ds.grm(), y)
    ds.close()


@pytest.mark.gpu
def test_fixture_file_subset_and_unsorted_list(gpu_lib):
    ds = gpu_lib.Dataset.open(data_path("pca_example.pgen"))
    n, m = ds.n_samples, ds.v_end
    codes = unpack_rows(ds.copy_rows_to_host(0, m), n)
    rng = np.random.default_rng(5)
    vidx = rng.permutation(m)[:133].astype(np.uint32)
    mask = rng.random(n) < 0.6
    ss = ds.subset(mask)
    sel = np.flatnonzero(mask)
    check(*ds.grm(vidx=vidx, subset=ss), Yardstick(codes[vidx], sel))
    y = Yardstick(codes[37:201], sel)
    check(*ds.grm(v_begin=37, v_end=201, subset=ss), y)
    k = len(sel)
    rel, nobs, used = ds.grm(v_begin=37, v_end=201, subset=ss, i_range=(3, 20), j_range=(10, k))
    check(rel, nobs, used, y, np.arange(3, 20), np.arange(10, k))
    ss.close()
    ds.close()


T = 128
SHAPES = [(1, 1), (1, 65), (2, 3), (2, 1000), (17, 4), (17, 257), (257, 5), (257, 63), (300, 65), (300, 1),
          (1000, 63), (1000, 1000), (2 * T + 3, 257), (2 * T + 3, 1000), (2 * T + 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", SHAPES)
def test_shapes_off_every_grid(gpu_lib, n, v):
    assert gpu_lib.GRM_TILE == T
    rng = np.random.default_rng(1000 * n + v)
    codes = random_codes(rng, v, n, rng.uniform(0.02, 0.05))
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    check(*ds.grm(), Yardstick(codes))
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("v", [1, 3, 5, 63, 65])
def test_padding_all_het(gpu_lib, v):
    """All het.  The counted p is 0.5 and z[1] = 0: rel is exactly 0.  With the supplied frequency at which z[1] is
    exactly 1, every product is 1: rel == 1 exactly for every pair, the diagonal included.  nobs == v both times: the
    codes past the end of the list, the K-step and the row's padding are not calls."""
    n = 131
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(np.ones((v, n), dtype=np.uint8)), n)
    rel, nobs, used = ds.grm()
    assert used == v and np.array_equal(nobs, np.full((n, n), v, dtype=np.uint32))
    assert same_bytes(rel, np.zeros((n, n)))
    rel, nobs, used = ds.grm(freq=np.full(v, P_Z1_IS_ONE))
    assert used == v and np.array_equal(nobs, np.full((n, n), v, dtype=np.uint32))
    assert same_bytes(rel, np.ones((n, n)))
    ds.close()


@pytest.mark.gpu
def test_skipped_variants(gpu_lib):
    rng = np.random.default_rng(11)
    n, v = 150, 200
    codes = random_codes(rng, v, n, 0.03)
    codes[[0, 64, 199], :] = 3                      # all missing
    codes[[5, 63], :] = 0                           # all hom-ref
    codes[[128], :] = 2                             # all hom-alt
    codes[17, :] = np.where(rng.random(n) < 0.2, 3, 0)  # hom-ref or missing
    y = Yardstick(codes)
    assert y.n_used == v - 7
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    rel, nobs, used = ds.grm()
    check(rel, nobs, used, y)
    rel2, nobs2, used2 = ds.grm(vidx=y.used.astype(np.uint32))
    assert used2 == used and same_bytes(rel, rel2) and same_bytes(nobs, nobs2)
    # nothing but skipped variants
    rel, nobs, used = ds.grm(vidx=np.array([0, 5, 128, 17], dtype=np.uint32))
    assert used == 0 and np.isnan(rel).all() and not nobs.any()
    rel, nobs, used = ds.grm(vidx=np.array([5], dtype=np.uint32), meanimpute=True, i_range=(3, 9), j_range=(0, 150))
    assert used == 0 and rel.shape == (6, 150) and np.isnan(rel).all() and not nobs.any()
    ds.close()


@pytest.fixture(scope="module")
def square(gpu_lib):
    n, v = 700, 500
    codes = random_codes(np.random.default_rng(77), v, n, 0.03)
    codes[:, 650] = codes[:, 9]  # a duplicated sample across distant tiles
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    y = Yardstick(codes)
    whole = ds.grm()
    yield ds, codes, y, whole
    ds.close()


@pytest.mark.gpu
def test_whole_square_symmetry_determinism_and_king_nobs(square, gpu_lib):
    ds, codes, y, (rel, nobs, used) = square
    check(rel, nobs, used, y)
    assert used == codes.shape[0]  # nothing skipped
    assert np.array_equal(nobs, ds.king_counts()[gpu_lib.KING_NSNP])
    assert same_bytes(rel, np.ascontiguousarray(rel.T)) and same_bytes(nobs, np.ascontiguousarray(nobs.T))
    again = ds.grm()
    assert same_bytes(again[0], rel) and same_bytes(again[1], nobs) and again[2] == used
    # the duplicated sample: every sum it takes part in is its original's
    assert np.float64(rel[9, 650]).tobytes() == np.float64(rel[9, 9]).tobytes() == np.float64(rel[650, 650]).tobytes()
    assert same_bytes(rel[650], rel[9])


@pytest.mark.gpu
@pytest.mark.parametrize("ir,jr", [((0, 100), (400, 700)), ((100, 300), (200, 400)), ((5, 6), (0, 700)),
                                   ((699, 700), (699, 700)), ((130, 131), (17, 18)), ((127, 385), (1, 129)),
                                   ((300, 700), (0, 50))])
def test_rectangles(square, ir, jr):
    ds, _, _, (rel, nobs, used) = square
    r, c, u = ds.grm(i_range=ir, j_range=jr)
    assert u == used
    assert same_bytes(r, np.ascontiguousarray(rel[ir[0]:ir[1], jr[0]:jr[1]]))
    assert same_bytes(c, np.ascontiguousarray(nobs[ir[0]:ir[1], jr[0]:jr[1]]))
    # the other way round: the row sample becomes the column sample
    r2, c2, _ = ds.grm(i_range=jr, j_range=ir)
    assert same_bytes(np.ascontiguousarray(r2.T), r) and same_bytes(np.ascontiguousarray(c2.T), c)


@pytest.mark.gpu
def test_full_square_in_several_bands(gpu_lib):
    """3,500 samples: rel and nobs of a band and its mirror strip are 2 x 12 B a pair, so the default 256 MB budget
    cuts the square into two bands (3,072 rows and 428).  The second band's rows left of the diagonal come from the
    first band's mirror strip."""
    n, v = 3500, 64
    assert 2 * 12 * n * n > 256 << 20 and (256 << 20) // (2 * 12 * n) // T * T == 3072
    rng = np.random.default_rng(3500)
    codes = random_codes(rng, v, n, 0.03)
    codes[:, 3400] = codes[:, 11]  # a duplicate across the two bands
    y = Yardstick(codes)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    rel, nobs, used = ds.grm()
    check(rel, nobs, used, y)
    assert same_bytes(rel, np.ascontiguousarray(rel.T)) and same_bytes(nobs, np.ascontiguousarray(nobs.T))
    assert same_bytes(rel[3400], rel[11])
    # rectangles across the cut, one band each, are the same bits
    for ir, jr in [((3000, 3500), (0, 300)), ((2900, 3200), (2900, 3200)), ((0, 200), (3072, 3500))]:
        r, c, _ = ds.grm(i_range=ir, j_range=jr)
        assert same_bytes(r, np.ascontiguousarray(rel[ir[0]:ir[1], jr[0]:jr[1]]))
        assert same_bytes(c, np.ascontiguousarray(nobs[ir[0]:ir[1], jr[0]:jr[1]]))
    ds.close()


@pytest.mark.gpu
def test_band_size_does_not_change_the_result(square, gpu_lib, monkeypatch):
    """The byte budget of a band lowered until a band is one tile row: six bands for the 700 x 700 square (triangle
    launches, mirror strips), for a square on the diagonal that does not start at 0, for rectangles (every tile, plain
    copies), with and without nobs."""
    ds, _, _, (rel, nobs, used) = square
    n = rel.shape[0]
    monkeypatch.setenv(gpu_lib.GRM_BAND_ENV, str(2 * 12 * n * T))      # full square: T rows a band
    r, c, u = ds.grm()
    assert u == used and same_bytes(r, rel) and same_bytes(c, nobs)
    monkeypatch.setenv(gpu_lib.GRM_BAND_ENV, str(2 * 12 * n * 2 * T))  # 2 T rows: bands of 256, 256, 188
    r, c, _ = ds.grm()
    assert same_bytes(r, rel) and same_bytes(c, nobs)
    r, c, _ = ds.grm(want_nobs=False)                                  # 8 B a pair: 384 rows, then 316
    assert c is None and same_bytes(r, rel)
    monkeypatch.setenv(gpu_lib.GRM_BAND_ENV, "1")                      # never less than one tile row
    for ir, jr in [((130, 600), (130, 600)), ((100, 700), (0, 650)), ((0, 700), (5, 6)), ((3, 645), (300, 700))]:
        for want in (True, False):
            r, c, _ = ds.grm(i_range=ir, j_range=jr, want_nobs=want)
            assert same_bytes(r, np.ascontiguousarray(rel[ir[0]:ir[1], jr[0]:jr[1]])), (ir, jr, want)
            assert c is None if not want else same_bytes(c, np.ascontiguousarray(nobs[ir[0]:ir[1], jr[0]:jr[1]]))
    relm = ds.grm(meanimpute=True)[0]
    monkeypatch.delenv(gpu_lib.GRM_BAND_ENV)
    assert same_bytes(relm, ds.grm(meanimpute=True)[0])


@pytest.mark.gpu
def test_supplied_freq(gpu_lib):
    rng = np.random.default_rng(21)
    n, v = 150, 130
    codes = random_codes(rng, v, n, 0.03)
    codes[40, :] = 3
    freq = rng.uniform(0.01, 0.99, v)
    freq[[3, 64, 65, 129]] = [math.nan, 0.0, 1.0, -0.1]
    freq[100] = math.inf
    y = Yardstick(codes, freq=freq)
    assert y.n_used == v - 6  # five frequencies and the variant nobody is called at
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    check(*ds.grm(freq=freq), y)
    # the counted frequencies handed back in give the same bytes as the call without freq
    p = np.array([py_standardize(int((c == 1).sum()), int((c == 2).sum()), int((c != 3).sum()))[0] for c in codes])
    a, b = ds.grm(), ds.grm(freq=p)
    assert a[2] == b[2] == v - 1 and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    with pytest.raises(ValueError, match="freq"):
        ds.grm(freq=freq[:-1])
    ds.close()


@pytest.mark.gpu
def test_meanimpute(gpu_lib):
    rng = np.random.default_rng(31)
    n, v = 2 * T + 3, 300
    codes = random_codes(rng, v, n, 0.05)
    codes[7, :] = 0
    y = Yardstick(codes)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    rel, nobs, used = ds.grm()
    relm, nobsm, usedm = ds.grm(meanimpute=True)
    assert usedm == used == v - 1 and same_bytes(nobs, nobsm)
    check(relm, nobsm, usedm, y, meanimpute=True)
    r, c, _ = ds.grm(meanimpute=True, i_range=(100, 259), j_range=(0, 130))
    assert same_bytes(r, np.ascontiguousarray(relm[100:259, :130]))
    ds.close()


@pytest.mark.gpu
def test_refusals(gpu_lib):
    n, v = 60, 40
    codes = random_codes(np.random.default_rng(41), v, n, 0.02)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    for ir, jr in [((5, 5), (0, 3)), ((6, 5), (0, 3)), ((0, 3), (9, 2)), ((0, n + 1), (0, 3)), ((0, 3), (n, n + 1)),
                   ((n, n), (0, 1))]:
        with pytest.raises(ValueError, match="rectangle"):
            ds.grm(i_range=ir, j_range=jr)
    with pytest.raises(ValueError, match="n_var"):
        ds.grm(v_begin=5, v_end=5)
    with pytest.raises(ValueError, match="n_var"):
        ds.grm(vidx=np.zeros(0, dtype=np.uint32))
    with pytest.raises(ValueError, match="range"):
        ds.grm(v_begin=v - 2, v_end=v + 1)
    with pytest.raises(ValueError, match="variant index"):
        ds.grm(vidx=np.array([0, v], dtype=np.uint32))
    rel = np.zeros((n, n))
    eb = C.create_string_buffer(gpu_lib.ERRBUF_LEN)
    rc = gpu_lib.raw().pgh_grm(ds._h, None, 0, v, None, None, 0, n, 0, n, 2, rel.ctypes.data, None, None, eb)
    assert rc != 0 and b"flag" in eb.value
    rc = gpu_lib.raw().pgh_grm(ds._h, None, 0, v, None, None, 0, n, 0, n, 0, rel.ctypes.data, None, None, eb)
    assert rc == 0 and same_bytes(rel, ds.grm()[0])  # nobs and n_used may be NULL
    other = gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)
    ss = other.subset(np.ones(n, dtype=bool))
    with pytest.raises(ValueError, match="different dataset"):
        ds.grm(subset=ss)
    ss.close()
    other.close()
    sp = gpu_lib.Dataset.open(data_path("rare_small.pgen"), sparse=True)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.grm()
    sp.close()
    group = gpu_lib.Dataset.group([gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)])
    with pytest.raises(ValueError, match="one device's dataset"):
        group.grm()
    group.close()
    ds.close()
