"""pgh_king_counts / pgh_king_table / pgh_king_kinship (Dataset.king_counts, Dataset.king_table, lib.king_kinship):
KING-robust pair counts and kinship on the int8 matrix cores.

The yardstick is brute force written here: boolean planes of the 2-bit codes the dataset was made from, multiplied as
float64 (BLAS; exact, every sum is far below 2^53) and converted back.  Counts are compared with np.array_equal,
never with a tolerance; a table's kinship column is compared bit for bit with king_kinship of its own counts."""

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
    """The inverse: (V, N) codes out of packed rows."""
    shifts = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((rows[:, :, None] >> shifts) & 3).reshape(rows.shape[0], -1)[:, :n].astype(np.uint8)


def brute_counts(codes, rows=None, cols=None):
    """(5, ni, nj) uint32 from (V, N) codes: NSNP, HETHET, IBS0, HET1HOM2, HET2HOM1 of samples rows x cols."""
    n = codes.shape[1]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    a, b = codes[:, rows], codes[:, cols]

    def planes(c):
        return [(c == k).astype(np.float64) for k in (0, 1, 2)]

    ref_a, het_a, alt_a = planes(a)
    ref_b, het_b, alt_b = planes(b)
    called_a, called_b = ref_a + het_a + alt_a, ref_b + het_b + alt_b
    hom_a, hom_b = ref_a + alt_a, ref_b + alt_b
    out = np.stack([called_a.T @ called_b, het_a.T @ het_b, ref_a.T @ alt_b + alt_a.T @ ref_b, het_a.T @ hom_b,
                    hom_a.T @ het_b])
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


def py_kinship(hethet, ibs0, h1, h2):
    """The issue's formula in Python integers and floats (int / int is correctly rounded)."""
    min_het = int(hethet) + min(int(h1), int(h2))
    if min_het == 0:
        return math.nan
    return 0.5 - (4 * int(ibs0) + int(h1) + int(h2)) / (4 * min_het)


def brute_table(codes, min_kinship):
    """[(i, j, nsnp, hethet, ibs0, h1, h2, kinship)] for i < j passing the filter, in (i, j) order."""
    c = brute_counts(codes)
    n = codes.shape[1]
    no_filter = math.isnan(min_kinship) or min_kinship == -math.inf
    out = []
    for i in range(n):
        for j in range(i + 1, n):
            k = py_kinship(c[1, i, j], c[2, i, j], c[3, i, j], c[4, i, j])
            if no_filter or k >= min_kinship:
                out.append((i, j, int(c[0, i, j]), int(c[1, i, j]), int(c[2, i, j]), int(c[3, i, j]), int(c[4, i, j]), k))
    return out


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def random_codes(rng, v, n, missing):
    p = rng.uniform(0.05, 0.5, v)[:, None]
    codes = rng.binomial(2, p, size=(v, n)).astype(np.uint8)
    codes[rng.random((v, n)) < missing] = 3
    return codes


def check_table(table, expect):
    assert len(table) == len(expect)
    for row, e in zip(table, expect):
        got = (int(row["i"]), int(row["j"]), int(row["nsnp"]), int(row["hethet"]), int(row["ibs0"]),
               int(row["het1hom2"]), int(row["het2hom1"]))
        assert got == e[:7]
        assert same_bits(row["kinship"], e[7]), (got, row["kinship"], e[7])


# ---- no device ---------------------------------------------------------------------------------------------------

KING_SYMBOLS = ("pgh_king_counts", "pgh_king_table", "pgh_king_kinship")


def test_header_declares_and_library_exports_king(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in KING_SYMBOLS:
        assert name + "(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert (lib.KING_NSNP, lib.KING_HETHET, lib.KING_IBS0, lib.KING_HET1HOM2, lib.KING_HET2HOM1,
            lib.KING_PLANES) == (0, 1, 2, 3, 4, 5)
    assert lib.KING_PAIR_DTYPE.itemsize == 40


def test_king_kinship_is_the_formula_bit_for_bit(lib):
    top = 2 ** 31 - 1
    grid = [0, 1, 2, 3, 7, 100, 12345, 2 ** 20 + 1, top - 1, top]
    n = 0
    for hethet in grid:
        for ibs0 in grid:
            for h1 in grid:
                for h2 in grid:
                    got, exp = lib.king_kinship(hethet, ibs0, h1, h2), py_kinship(hethet, ibs0, h1, h2)
                    assert same_bits(got, exp) or (math.isnan(got) and math.isnan(exp)), (hethet, ibs0, h1, h2)
                    n += 1
    assert n == 10 ** 4
    # min_het == 0: NaN, whatever the numerator
    assert math.isnan(lib.king_kinship(0, 0, 0, 0))
    assert math.isnan(lib.king_kinship(0, 5, 0, 9))
    assert math.isnan(lib.king_kinship(0, 5, 9, 0))
    # duplicates: no IBS0, no het against hom
    for hethet in (1, 977, top):
        assert lib.king_kinship(hethet, 0, 0, 0) == 0.5
    # the smaller het count is the denominator's, both ways round
    assert lib.king_kinship(10, 1, 2, 6) == 0.5 - 12 / 48 == lib.king_kinship(10, 1, 6, 2)
    assert lib.king_kinship(10, 1, 2, 6) != 0.5 - 12 / (4 * 16)
    # the largest counts the entry points can return
    assert same_bits(lib.king_kinship(top, top, top, top - 1), 0.5 - (4 * top + top + top - 1) / (4 * (2 * top - 1)))


# ---- on the GPU --------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pgen_example", "pca_example", "rare_small", "large_example"])
def test_fixture_files_full_square(gpu_lib, name):
    ds = gpu_lib.Dataset.open(data_path(name + ".pgen"))
    n = ds.n_samples
    codes = unpack_rows(ds.copy_rows_to_host(ds.v_begin, ds.v_end), n)
    got = ds.king_counts()
    assert got.shape == (5, n, n) and got.dtype == np.uint32
    assert np.array_equal(got, brute_counts(codes))
    ds.close()


@pytest.mark.gpu
def test_fixture_file_codes_are_the_oracles(gpu_lib, oracle):
    """The rows the brute force reads are the file's calls as the CPU decoder sees them."""
    path = data_path("pca_example.pgen")
    ds = gpu_lib.Dataset.open(path)
    pg = oracle.Pgen(path)
    codes = np.stack([pg.raw(v) for v in range(pg.M)])
    assert np.array_equal(ds.king_counts(), brute_counts(codes))
    ds.close()


@pytest.mark.gpu
def test_fixture_file_variant_list_with_subset(gpu_lib):
    ds = gpu_lib.Dataset.open(data_path("pca_example.pgen"))
    n, m = ds.n_samples, ds.v_end
    codes = unpack_rows(ds.copy_rows_to_host(0, m), n)
    rng = np.random.default_rng(5)
    vidx = rng.permutation(m)[:133].astype(np.uint32)  # unsorted on purpose: a sum does not care
    mask = rng.random(n) < 0.6
    ss = ds.subset(mask)
    sel = np.flatnonzero(mask)
    assert np.array_equal(ds.king_counts(vidx=vidx, subset=ss), brute_counts(codes[vidx], sel, sel))
    assert np.array_equal(ds.king_counts(v_begin=37, v_end=201, subset=ss), brute_counts(codes[37:201], sel, sel))
    ss.close()
    ds.close()


# large sample counts with small variant counts and the reverse: the float64 brute force stays in seconds
SHAPES = [(1, 4097), (2, 1000), (17, 65), (257, 64), (1000, 63), (4099, 1), (4099, 65), (17, 1), (257, 1000),
          (1000, 4097), (300, 63), (2, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", SHAPES)
def test_shapes_off_the_tile_grid(gpu_lib, n, v):
    assert 4099 > 2 * gpu_lib.KING_TILE and 4099 % gpu_lib.KING_TILE  # beyond two tiles, with a remainder
    rng = np.random.default_rng(1000 * n + v)
    codes = random_codes(rng, v, n, rng.uniform(0.02, 0.05))
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    assert np.array_equal(ds.king_counts(), brute_counts(codes))
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("v", [1, 63, 65, 255, 257])
def test_padding_is_not_called_not_hom_ref(gpu_lib, v):
    """All hom-ref: NSNP is the variant count, not the count rounded up to the kernel's K-step or the row's padding."""
    n = 131
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(np.zeros((v, n), dtype=np.uint8)), n)
    got = ds.king_counts()
    assert np.array_equal(got[gpu_lib.KING_NSNP], np.full((n, n), v, dtype=np.uint32))
    assert not got[1:].any()
    ds.close()


@pytest.fixture(scope="module")
def square(gpu_lib):
    n, v = 700, 500
    codes = random_codes(np.random.default_rng(77), v, n, 0.03)
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    yield ds, codes, brute_counts(codes)
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ir,jr", [((0, 100), (400, 700)), ((100, 300), (200, 400)), ((5, 6), (0, 700)),
                                   ((699, 700), (699, 700)), ((130, 131), (17, 18)), ((127, 385), (1, 129)),
                                   ((300, 700), (0, 50))])
def test_rectangles(square, ir, jr):
    ds, _, full = square
    got = ds.king_counts(i_range=ir, j_range=jr)
    assert got.shape == (5, ir[1] - ir[0], jr[1] - jr[0])
    assert np.array_equal(got, full[:, ir[0]:ir[1], jr[0]:jr[1]])


@pytest.mark.gpu
def test_quadrants_and_symmetry(square, gpu_lib):
    ds, codes, full = square
    n, cut = codes.shape[1], 333
    whole = ds.king_counts()
    assert np.array_equal(whole, full)
    for ir in ((0, cut), (cut, n)):
        for jr in ((0, cut), (cut, n)):
            assert np.array_equal(ds.king_counts(i_range=ir, j_range=jr), whole[:, ir[0]:ir[1], jr[0]:jr[1]])
    for p in (gpu_lib.KING_NSNP, gpu_lib.KING_HETHET, gpu_lib.KING_IBS0):
        assert np.array_equal(whole[p], whole[p].T)
    assert np.array_equal(whole[gpu_lib.KING_HET1HOM2], whole[gpu_lib.KING_HET2HOM1].T)
    # the diagonal: a sample against itself
    het = (codes == 1).sum(axis=0)
    assert np.array_equal(np.diagonal(whole[gpu_lib.KING_HETHET]), het)
    assert np.array_equal(np.diagonal(whole[gpu_lib.KING_NSNP]), (codes != 3).sum(axis=0))
    assert not np.diagonal(whole[gpu_lib.KING_IBS0]).any()


@pytest.mark.gpu
def test_all_missing_samples_and_variants(gpu_lib):
    ds = gpu_lib.Dataset.open(data_path("all_missing.pgen"))
    n = ds.n_samples
    codes = unpack_rows(ds.copy_rows_to_host(0, ds.v_end), n)
    assert (codes == 3).all()
    assert not ds.king_counts().any()
    table = ds.king_table()
    assert len(table) == n * (n - 1) // 2 and np.isnan(table["kinship"]).all() and not table["nsnp"].any()
    assert len(ds.king_table(min_kinship=-1e300)) == 0  # NaN never passes a filter
    ds.close()
    # rows of missing samples and one missing variant inside an ordinary matrix
    rng = np.random.default_rng(9)
    codes = random_codes(rng, 200, 150, 0.02)
    codes[:, [0, 77, 149]] = 3
    codes[50, :] = 3
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), 150)
    got = ds.king_counts()
    assert np.array_equal(got, brute_counts(codes))
    assert not got[:, 77, :].any() and not got[:, :, 149].any()
    table = ds.king_table()
    check_table(table, brute_table(codes, -math.inf))
    assert np.isnan(table["kinship"][table["i"] == 0]).all()
    ds.close()


CUTOFFS = [0.354, 0.177, 0.0884, -math.inf]


def pedigree_codes(seed=7):
    """60 samples x 3,000 variants: 40 founders, 8 children of the couples (0,1), (2,3), ..., 4 second children of the
    first four couples, 4 copies of samples 0-3, 4 more children of founders 0 and 2; 2 % of the calls missing."""
    rng = np.random.default_rng(seed)
    v, n, founders = 3000, 60, 40
    p = rng.uniform(0.05, 0.5, v)
    h1, h2 = [], []
    g = np.zeros((v, n), dtype=np.uint8)

    def hap():
        return (rng.random(v) < p).astype(np.uint8)

    def child(a, b):
        x = np.where(rng.random(v) < 0.5, h1[a], h2[a])
        y = np.where(rng.random(v) < 0.5, h1[b], h2[b])
        h1.append(x)
        h2.append(y)
        return x + y

    for s in range(founders):
        h1.append(hap())
        h2.append(hap())
        g[:, s] = h1[s] + h2[s]
    s = founders
    for k in range(8):
        g[:, s] = child(2 * k, 2 * k + 1)
        s += 1
    for k in range(4):
        g[:, s] = child(2 * k, 2 * k + 1)
        s += 1
    for k in range(4):
        g[:, s] = g[:, k]
        h1.append(h1[k])
        h2.append(h2[k])
        s += 1
    while s < n:
        g[:, s] = child(0, 2)
        s += 1
    g[rng.random((v, n)) < 0.02] = 3
    return g


@pytest.fixture(scope="module")
def pedigree(gpu_lib):
    codes = pedigree_codes()
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), codes.shape[1])
    yield ds, codes
    ds.close()


def test_pedigree_fixture_is_not_trivial():
    codes = pedigree_codes()
    n = codes.shape[1]
    every = brute_table(codes, -math.inf)
    assert len(every) == n * (n - 1) // 2
    kin = np.array([e[7] for e in every])
    assert not np.isnan(kin).any()
    found = []
    for cut in CUTOFFS[:3]:
        assert not (np.abs(kin - cut) <= 1e-12).any(), "a pair sits on a cut-off: reseed the fixture"
        found.append(int((kin >= cut).sum()))
        assert 0 < found[-1] < len(every)
    assert found[0] < found[1] < found[2]
    # a copy differs from its original only in which calls are missing: exactly 0.5 over the calls both have
    by_pair = {(e[0], e[1]): e[7] for e in every}
    assert all(by_pair[(k, 52 + k)] == 0.5 for k in range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTOFFS + [math.nan])
def test_table_equals_brute_force(pedigree, gpu_lib, cut):
    ds, codes = pedigree
    table = ds.king_table(min_kinship=cut)
    assert table.dtype == gpu_lib.KING_PAIR_DTYPE
    check_table(table, brute_table(codes, cut))
    for row in table:
        k = gpu_lib.king_kinship(row["hethet"], row["ibs0"], row["het1hom2"], row["het2hom1"])
        assert same_bits(row["kinship"], k)
    assert not table["pad"].any()


@pytest.mark.gpu
def test_table_over_many_tiles_and_a_grown_list(gpu_lib):
    """1,500 samples: 12 x 12 tiles, and 1,124,250 unfiltered pairs -- more than the first device list holds."""
    n, v = 1500, 96
    codes = random_codes(np.random.default_rng(31), v, n, 0.03)
    codes[:, 1400] = codes[:, 3]  # a duplicate across distant tiles
    ds = gpu_lib.Dataset.from_host_rows(pack_rows(codes), n)
    c = brute_counts(codes)
    table = ds.king_table()
    assert len(table) == n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    assert np.array_equal(table["i"], iu[0]) and np.array_equal(table["j"], iu[1])
    for p, name in enumerate(("nsnp", "hethet", "ibs0", "het1hom2", "het2hom1")):
        assert np.array_equal(table[name], c[p][iu])
    with np.errstate(all="ignore"):
        min_het = c[1].astype(np.int64) + np.minimum(c[3], c[4])
        kin = 0.5 - (4 * c[2].astype(np.int64) + c[3] + c[4]) / (4 * min_het).astype(np.float64)
    kin[min_het == 0] = np.nan
    assert np.array_equal(table["kinship"].view(np.uint64) << 1, kin[iu].view(np.uint64) << 1)  # NaN sign aside
    some = ds.king_table(min_kinship=0.2)
    keep = kin[iu] >= 0.2
    assert 0 < keep.sum() < len(table) and (3, 1400) in set(zip(some["i"].tolist(), some["j"].tolist()))
    assert some.tobytes() == table[keep].tobytes()
    ds.close()


@pytest.mark.gpu
def test_capacity(pedigree, gpu_lib):
    ds, codes = pedigree
    L = gpu_lib
    full = ds.king_table(min_kinship=0.0884)
    rows, found = ds.king_table_capped(0.0884, 0)
    assert len(rows) == 0 and found == len(full) > 10
    rows, found = ds.king_table_capped(0.0884, 10)
    assert found == len(full) and rows.tobytes() == full[:10].tobytes()
    rows, found = ds.king_table_capped(0.0884, len(full) + 5)
    assert found == len(full) and rows.tobytes() == full.tobytes()
    # nothing is written past what the call reports: the buffer behind a short table keeps its bytes
    buf = np.full(len(full) + 3, 0xAB, dtype=np.uint8).repeat(40).view(L.KING_PAIR_DTYPE)
    n_found = C.c_uint64(0)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    rc = L.raw().pgh_king_table(ds._h, None, 0, codes.shape[0], None, 0.0884, buf.ctypes.data_as(C.c_void_p), 4,
                                C.byref(n_found), eb)
    assert rc == 0 and n_found.value == len(full)
    assert buf[:4].tobytes() == full[:4].tobytes()
    assert (buf[4:].view(np.uint8) == 0xAB).all()


@pytest.mark.gpu
def test_determinism_subset_and_threads(pedigree, gpu_lib):
    ds, codes = pedigree
    first = ds.king_table(min_kinship=0.0884).tobytes()
    for _ in range(2):
        assert ds.king_table(min_kinship=0.0884).tobytes() == first
    every = ds.king_table().tobytes()
    for _ in range(2):
        assert ds.king_table().tobytes() == every
    mask = np.random.default_rng(3).random(codes.shape[1]) < 0.7
    mask[[0, 1, 40, 52]] = True
    ss = ds.subset(mask)
    sel = np.flatnonzero(mask)
    assert np.array_equal(ds.king_counts(subset=ss), brute_counts(codes, sel, sel))
    check_table(ds.king_table(min_kinship=0.177, subset=ss), brute_table(codes[:, sel], 0.177))
    assert np.array_equal(ds.king_counts(subset=ss, i_range=(3, 20), j_range=(10, len(sel))),
                          brute_counts(codes, sel[3:20], sel[10:]))
    # a call from a second thread next to calls on this one: each on its own stream, same results
    results = {}

    def worker():
        try:
            results["table"] = [ds.king_table(min_kinship=0.0884).tobytes() for _ in range(3)]
            results["counts"] = ds.king_counts()
        except Exception as e:  # noqa: BLE001
            results["error"] = e

    th = threading.Thread(target=worker)
    th.start()
    mine = [ds.king_table(min_kinship=0.0884).tobytes() for _ in range(3)]
    mine_counts = ds.king_counts()
    th.join()
    assert "error" not in results, results.get("error")
    assert all(t == first for t in mine + results["table"])
    assert np.array_equal(mine_counts, results["counts"]) and np.array_equal(mine_counts, brute_counts(codes))
    ss.close()


@pytest.mark.gpu
def test_refusals(pedigree, gpu_lib):
    ds, codes = pedigree
    v, n = codes.shape
    for ir, jr in [((5, 5), (0, 3)), ((6, 5), (0, 3)), ((0, 3), (9, 2)), ((0, n + 1), (0, 3)), ((0, 3), (n, n + 1)),
                   ((n, n), (0, 1))]:
        with pytest.raises(ValueError, match="rectangle"):
            ds.king_counts(i_range=ir, j_range=jr)
    with pytest.raises(ValueError, match="n_var"):
        ds.king_counts(v_begin=5, v_end=5)
    with pytest.raises(ValueError, match="n_var"):
        ds.king_table(v_begin=5, v_end=5)
    with pytest.raises(ValueError, match="n_var"):
        ds.king_counts(vidx=np.zeros(0, dtype=np.uint32))
    with pytest.raises(ValueError, match="range"):
        ds.king_counts(v_begin=v - 2, v_end=v + 1)
    with pytest.raises(ValueError, match="range"):
        ds.king_table(v_begin=v, v_end=v + 1)
    with pytest.raises(ValueError, match="variant index"):
        ds.king_counts(vidx=np.array([0, v], dtype=np.uint32))
    with pytest.raises(ValueError, match="variant index"):
        ds.king_table(vidx=np.array([v + 7], dtype=np.uint32))
    other = gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)
    ss = other.subset(np.ones(n, dtype=bool))
    with pytest.raises(ValueError, match="different dataset"):
        ds.king_counts(subset=ss)
    ss.close()
    other.close()
    sp = gpu_lib.Dataset.open(data_path("rare_small.pgen"), sparse=True)
    with pytest.raises(ValueError, match="dense-resident"):
        sp.king_counts()
    with pytest.raises(ValueError, match="dense-resident"):
        sp.king_table()
    sp.close()
    group = gpu_lib.Dataset.group([gpu_lib.Dataset.from_host_rows(pack_rows(codes[:10]), n)])
    with pytest.raises(ValueError, match="one device's dataset"):
        group.king_counts()
    with pytest.raises(ValueError, match="one device's dataset"):
        group.king_table()
    group.close()
