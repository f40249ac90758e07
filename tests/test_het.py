"""pgh_het (Dataset.het) on the GPU against the yardstick of tests/het_oracle.py: every field of every row bit for
bit, no tolerance (every operation of the contract is an integer one or one correctly rounded IEEE operation).

T = lib.HET_TILE samples are one workgroup tile of k_het_missing_sum; a lane of it holds 64 samples of a row."""

import ctypes as C
import threading

import numpy as np
import pytest

import het_oracle as H
import subset_shapes as S
from conftest import data_path

pytestmark = pytest.mark.gpu

SEED = 20261021


def pack_rows(codes):
    v, n = codes.shape
    padded = np.zeros((v, (n + 3) // 4 * 4), dtype=np.uint8)
    padded[:, :n] = codes
    q = padded.reshape(v, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def unpack_rows(rows, n):
    shifts = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((rows[:, :, None] >> shifts) & 3).reshape(rows.shape[0], -1)[:, :n].astype(np.uint8)


def random_codes(rng, v, n, missing):
    p = rng.uniform(0.05, 0.5, v)[:, None]
    codes = rng.binomial(2, p, size=(v, n)).astype(np.uint8)
    codes[rng.random((v, n)) < missing] = 3
    return codes


def resident(L, codes):
    return L.Dataset.from_host_rows(pack_rows(codes), codes.shape[1])


def synth_codes(L, v0, v1, n, seed, missing):
    return unpack_rows(np.stack([L.synth_record_host(v, n, seed, missing) for v in range(v0, v1)]), n)


def check(got, want):
    rows, used, n_used = got
    w_rows, w_used, w_n = want
    assert rows.dtype == H.ROW_DTYPE and used.dtype == np.uint8
    assert n_used == w_n and np.array_equal(used, w_used)
    for f in H.FIELDS:
        assert rows[f].tobytes() == w_rows[f].tobytes(), f
    assert H.same_rows(rows, w_rows)


def same(a, b):
    return H.same_rows(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def raw_het(L, ds, subset, v0, n, vidx, freq, flags, n_out):
    """pgh_het itself with prefilled outputs: (rc, message, outputs untouched?)."""
    out = np.full(32 * max(n_out, 1), 0x5A, dtype=np.uint8)
    used = np.full(max(n, 1), 9, dtype=np.uint8)
    n_used = C.c_uint32(77)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    v = None if vidx is None else np.ascontiguousarray(vidx, dtype=np.uint32)
    f = None if freq is None else np.ascontiguousarray(freq, dtype=np.float64)
    rc = L.raw().pgh_het(ds._h, subset._h if subset else None, v0, n, None if v is None else v.ctypes.data_as(C.c_void_p),
                         None if f is None else f.ctypes.data_as(C.c_void_p), flags, out.ctypes.data_as(C.c_void_p),
                         used.ctypes.data_as(C.c_void_p), C.byref(n_used), eb)
    untouched = bool((out == 0x5A).all() and (used == 9).all() and n_used.value == 77)
    return rc, eb.value.decode(), untouched


# ---- edges of the sample tile and of the variant walk ---------------------------------------------------------------


def sample_edges():
    from plinking_duck_amd.lib import HET_TILE as T
    return [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]


@pytest.mark.parametrize("n", sample_edges())
def test_sample_edges(gpu_lib, n):
    codes = random_codes(np.random.default_rng(SEED + n), 37, n, 0.10)
    ds = resident(gpu_lib, codes)
    for small in (True, False):
        check(ds.het(small_sample=small), H.rows_of(codes, small_sample=small))


@pytest.mark.parametrize("v", [1, 2, 1025])
def test_variant_edges(gpu_lib, v):
    codes = random_codes(np.random.default_rng(SEED + v), v, 130, 0.10)
    check(resident(gpu_lib, codes).het(), H.rows_of(codes))


def test_slices_do_not_change_a_byte(gpu_lib, monkeypatch):
    v, n = 150, gpu_lib.HET_TILE + 77
    codes = random_codes(np.random.default_rng(SEED), v, n, 0.10)
    ds = resident(gpu_lib, codes)
    want = H.rows_of(codes)
    check(ds.het(), want)  # the default choice
    for slices in (1, 2, 7, v + 50, 10 ** 9):
        monkeypatch.setenv(gpu_lib.HET_SLICES_ENV, str(slices))
        check(ds.het(), want)
    monkeypatch.setenv(gpu_lib.HET_SLICES_ENV, "seven")  # not a number: the default
    check(ds.het(), want)


# ---- structured rows and columns --------------------------------------------------------------------------------------


def test_structured_rows_and_columns(gpu_lib):
    rng = np.random.default_rng(SEED + 1)
    v, n = 41, 300
    codes = random_codes(rng, v, n, 0.15)
    codes[:, 5] = 3                       # a sample missing at every variant
    codes[:, 6] = np.where(codes[:, 6] == 3, 0, codes[:, 6])  # a sample missing nowhere
    codes[7] = 3                          # an all-missing variant
    codes[8] = 0                          # a monomorphic one ...
    codes[8, 5] = 3
    codes[9] = 2                          # ... either way
    codes[9, 5] = 3
    codes[10] = 3                         # a variant with one call, which is het
    codes[10, 6] = 1
    ds = resident(gpu_lib, codes)
    for small in (True, False):
        rows, used, n_used = got = ds.het(small_sample=small)
        check(got, H.rows_of(codes, small_sample=small))
        assert list(used[7:10]) == [0, 0, 0] and used[10] == 1 and n_used == v - 3
        assert rows[5]["obs_ct"] == 0 and rows[5]["e_sum"] == 0 and rows[5]["e_hom"] == 0.0 and np.isnan(rows[5]["f"])
        assert rows[6]["obs_ct"] == n_used
    # the lone het call: e = 0 with the correction, 0.5 without -- the only variant at which sample 6 differs
    only = resident(gpu_lib, codes[10:11])
    assert only.het(small_sample=True)[0][6]["e_hom"] == 0.0 and only.het(small_sample=False)[0][6]["e_hom"] == 0.5
    assert only.het(small_sample=True)[0][6]["f"] == 0.0  # (0 - 0) / (1 - 0)
    # a fully missing matrix: nothing is used, every row is the empty row
    gone = np.full((9, 130), 3, dtype=np.uint8)
    rows, used, n_used = resident(gpu_lib, gone).het()
    assert n_used == 0 and not used.any() and H.same_rows(rows, H.empty_rows(130))
    # 100 % het: p = 0.5 everywhere, nobody homozygous
    hets = np.ones((12, 200), dtype=np.uint8)
    got = resident(gpu_lib, hets).het()
    check(got, H.rows_of(hets))
    assert (got[0]["hom_ct"] == 0).all() and (got[0]["obs_ct"] == 12).all() and (got[0]["f"] < 0).all()


def test_no_variants_is_ok_with_empty_rows(gpu_lib):
    codes = random_codes(np.random.default_rng(3), 5, 70, 0.1)
    ds = resident(gpu_lib, codes)
    for kw in (dict(v_begin=2, v_end=2), dict(vidx=np.zeros(0, dtype=np.uint32))):
        rows, used, n_used = ds.het(**kw)
        assert n_used == 0 and len(used) == 0 and H.same_rows(rows, H.empty_rows(70))


# ---- subsets -----------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def subset_matrix():
    return S.hard_codes(S.N_SMALL)


@pytest.mark.parametrize("name", ["word_block", "stride4", "last_word", "empty"])
def test_subsets(gpu_lib, subset_matrix, name):
    codes = subset_matrix
    n = codes.shape[1]
    mask = S.shapes(n)[name]
    ds = resident(gpu_lib, codes)
    sub = ds.subset(mask)
    got = ds.het(subset=sub)
    want = H.rows_of(codes, sel=np.flatnonzero(mask))  # the frequencies are the subset's
    check(got, want)
    assert len(got[0]) == int(mask.sum())
    if name == "empty":
        assert got[2] == 0 and not got[1].any()
        return
    assert got[1][S.ROW_ALL_MISSING] == 0 and got[1][S.ROW_MONO] == 0
    if name == "word_block":
        assert got[1][S.ROW_BLOCK] == 0  # monomorphic among the kept samples only
        assert ds.het()[1][S.ROW_BLOCK] == 1
    # a sample outside the subset that is missing everywhere changes nothing
    other = codes.copy()
    other[:, int(np.flatnonzero(~mask)[0])] = 3
    ds2 = resident(gpu_lib, other)
    assert same(ds2.het(subset=ds2.subset(mask)), got)


# ---- supplied frequencies ------------------------------------------------------------------------------------------


def test_supplied_frequencies(gpu_lib):
    rng = np.random.default_rng(SEED + 2)
    v, n = 60, 257
    codes = random_codes(rng, v, n, 0.10)
    codes[4] = 0    # the counts would skip it; a frequency keeps it
    codes[5] = 3    # nothing called: skipped whatever the frequency
    freq = rng.uniform(0.01, 0.99, v)
    freq[[0, 11]] = [0.0, 1.0]                     # skip variants the counts would keep
    freq[[12, 13, 14]] = [np.nan, np.inf, -0.25]   # and these
    freq[15] = 5e-324
    ds = resident(gpu_lib, codes)
    got = ds.het(freq=freq, small_sample=False)
    check(got, H.rows_of(codes, freq=freq, small_sample=False))
    assert not got[1][[0, 5, 11, 12, 13, 14]].any() and got[1][[4, 15, 1, 2]].all()
    assert H.same_rows(ds.het(small_sample=False)[0], got[0]) is False
    sub_mask = S.shapes(n)["stride4"]
    check(ds.het(freq=freq, small_sample=False, subset=ds.subset(sub_mask)),
          H.rows_of(codes, sel=np.flatnonzero(sub_mask), freq=freq, small_sample=False))


# ---- ranges, lists, windows and shard groups ---------------------------------------------------------------------------


def test_range_list_shuffle_and_repeats(gpu_lib):
    rng = np.random.default_rng(SEED + 3)
    v, n = 90, 515
    codes = random_codes(rng, v, n, 0.10)
    ds = resident(gpu_lib, codes)
    ranged = ds.het(v_begin=10, v_end=80)
    check(ranged, H.rows_of(codes[10:80]))
    listed = ds.het(vidx=np.arange(10, 80))
    assert same(listed, ranged)
    perm = rng.permutation(np.arange(10, 80))
    shuffled = ds.het(vidx=perm)
    assert H.same_rows(shuffled[0], ranged[0]) and shuffled[2] == ranged[2]
    assert np.array_equal(shuffled[1], ranged[1][perm - 10])
    # a repeated entry counts twice (and makes the call one entry longer: its own scale)
    rep = np.array([3, 17, 3, 44, 44, 44, 89, 0], dtype=np.uint32)
    check(ds.het(vidx=rep), H.rows_of(codes[rep]))
    freq = rng.uniform(0.05, 0.95, len(rep))  # the freq of each of its entries
    check(ds.het(vidx=rep, freq=freq, small_sample=False), H.rows_of(codes[rep], freq=freq, small_sample=False))


def test_a_window_of_the_file_equals_the_whole_file(gpu_lib):
    path = data_path("pca_example.pgen")
    whole = gpu_lib.Dataset.open(path)
    window = gpu_lib.Dataset.open(path, variant_begin=37)
    assert window.v_begin == 37 and window.v_end == whole.v_end
    end = min(whole.v_end, 37 + 200)
    codes = unpack_rows(whole.copy_rows_to_host(37, end), whole.n_samples)
    a, b = whole.het(v_begin=37, v_end=end), window.het(v_begin=37, v_end=end)
    check(a, H.rows_of(codes))
    assert same(a, b)
    vidx = np.array([end - 1, 40, 37, 41, 40], dtype=np.uint32)
    assert same(whole.het(vidx=vidx), window.het(vidx=vidx))
    check(window.het(vidx=vidx), H.rows_of(codes[vidx - 37]))


def test_a_shard_group_equals_the_single_dataset(gpu_lib):
    L = gpu_lib
    m, n, seed, missing = 260, 700, SEED + 4, 0.06
    whole = L.Dataset.synth(0, m, n, seed, missing)
    group = L.Dataset.group([L.Dataset.synth(0, 101, n, seed, missing), L.Dataset.synth(101, m, n, seed, missing)])
    codes = synth_codes(L, 0, m, n, seed, missing)
    a = whole.het()
    check(a, H.rows_of(codes))
    assert same(group.het(), a)
    assert same(group.het(v_begin=90, v_end=130), whole.het(v_begin=90, v_end=130))
    assert same(group.het(v_begin=0, v_end=50), whole.het(v_begin=0, v_end=50))  # one shard has no share
    rng = np.random.default_rng(1)
    vidx = rng.permutation(m)[:120].astype(np.uint32)  # interleaves the shards
    vidx[5] = vidx[6]
    b = whole.het(vidx=vidx)
    check(b, H.rows_of(codes[vidx]))
    assert same(group.het(vidx=vidx), b)
    freq = rng.uniform(-0.05, 1.05, len(vidx))
    c = whole.het(vidx=vidx, freq=freq, small_sample=False)
    check(c, H.rows_of(codes[vidx], freq=freq, small_sample=False))
    assert same(group.het(vidx=vidx, freq=freq, small_sample=False), c)
    freq_r = rng.uniform(-0.05, 1.05, 40)
    assert same(group.het(v_begin=90, v_end=130, freq=freq_r, small_sample=False),
                whole.het(v_begin=90, v_end=130, freq=freq_r, small_sample=False))
    mask = S.shapes(n)["stride4"]
    d = whole.het(vidx=vidx, subset=whole.subset(mask))
    check(d, H.rows_of(codes[vidx], sel=np.flatnonzero(mask)))
    assert same(group.het(vidx=vidx, subset=group.subset(mask)), d)
    empty = group.het(subset=group.subset(np.zeros(n, dtype=bool)))
    assert len(empty[0]) == 0 and empty[2] == 0 and not empty[1].any()
    rc, msg, untouched = raw_het(L, group, None, 0, m + 1, None, None, 0, n)
    assert rc == L.PGH_ERR_ARG and "outside the resident range" in msg and untouched


# ---- repeatability ---------------------------------------------------------------------------------------------------


def test_repeated_calls_and_threads_give_the_same_bytes(gpu_lib):
    rng = np.random.default_rng(SEED + 5)
    codes_a = random_codes(rng, 80, 1500, 0.20)
    codes_b = random_codes(rng, 50, 1500, 0.40)
    a, b = resident(gpu_lib, codes_a), resident(gpu_lib, codes_b)
    first = a.het()
    check(first, H.rows_of(codes_a))
    second = b.het()  # other data through the same thread's buffers
    check(second, H.rows_of(codes_b))
    assert same(a.het(), first)  # sums that were not zeroed would show here
    got = {}

    def run(name, ds):
        got[name] = ds.het()

    threads = [threading.Thread(target=run, args=("a", a)), threading.Thread(target=run, args=("b", b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert same(got["a"], first) and same(got["b"], second)


# ---- refusals ---------------------------------------------------------------------------------------------------------


def test_refusals_leave_the_outputs_alone(gpu_lib):
    L = gpu_lib
    codes = random_codes(np.random.default_rng(9), 20, 100, 0.1)
    ds, other = resident(L, codes), resident(L, codes)
    freq = np.full(20, 0.3)
    cases = [
        ((ds, None, 0, 20, None, None, 2), "unknown flag bits"),
        ((ds, None, 0, 20, None, None, 0x80000001), "unknown flag bits"),
        ((ds, None, 0, 20, None, freq, L.HET_SMALL_SAMPLE), "freq"),
        ((ds, None, 0, 3, [1, 20, 2], None, 0), "outside the resident range"),
        ((ds, None, 5, 16, None, None, 0), "outside the resident range"),
        ((ds, other.subset(np.ones(100, dtype=bool)), 0, 20, None, None, 0), "different dataset"),
    ]
    for (d, sub, v0, n, vidx, f, flags), text in cases:
        rc, msg, untouched = raw_het(L, d, sub, v0, n, vidx, f, flags, 100)
        assert rc == L.PGH_ERR_ARG and text in msg and untouched, (text, msg)
    sparse = L.Dataset.open(data_path("pca_example.pgen"), sparse=True)
    rc, msg, untouched = raw_het(L, sparse, None, 0, 5, None, None, 0, sparse.n_samples)
    assert rc == L.PGH_ERR_ARG and "needs a dense-resident dataset" in msg and untouched
    with pytest.raises(ValueError):
        ds.het(freq=freq)  # small_sample defaults to True
    with pytest.raises(ValueError):
        ds.het(freq=freq[:3], small_sample=False)
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    assert L.raw().pgh_het(ds._h, None, 0, 20, None, None, 0, None, None, None, eb) == L.PGH_ERR_ARG
    assert "null argument" in eb.value.decode()


# ---- dosage tracks are not read -----------------------------------------------------------------------------------------


def test_dosage_tracks_are_not_read(gpu_lib):
    L = gpu_lib
    m, n, seed, missing = 70, 900, SEED + 6, 0.05
    plain = L.Dataset.synth(0, m, n, seed, missing)
    tracked = L.Dataset.synth(0, m, n, seed, missing)
    tracked.synth_add_dosage(0.3, seed + 1)
    assert tracked.info.dosage_variant_ct > 0
    got = tracked.het()
    check(got, H.rows_of(synth_codes(L, 0, m, n, seed, missing)))
    assert same(plain.het(), got)
