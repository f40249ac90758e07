"""The enqueue-only device entry points (include/pgenhip.h, "batched device calls"), called the way bench.py calls
them: a caller-owned device pointer, a caller-created stream, no host synchronisation between calls.

What belongs to the device forms alone -- and what the host-buffer forms, which call them at the minimal pitch on the
library's own stream and synchronise before they return, never show -- is pinned here:

  * the written extent: every output lives in the interior of a larger tensor filled with 0xA5 bytes (Guarded); the
    interior has exactly the extent the header documents, and at least 256 bytes of poison sit on each side.  After
    the final synchronise the interior must equal the reference and both guards must still be poison, byte for byte;
  * "zeroed by the call" / "overwritten": the interior starts as poison too, so a count that was only added onto
    what the buffer held, or an element the call skipped, shows;
  * out_pitch / out_stride wider than the row (the padding stays poison), NULL d_out / d_validity, the refusals;
  * back-to-back enqueues on caller streams, two buffer sets, a side stream behind an event (bench.py's step);
  * the library state keyed by (thread, device, stream): PghThreadScratch (one block per stream, growth after a
    drain, eviction of the oldest of more than eight) and pgh_ld_pairs_dev's per-thread task buffers.

References never pass through the code under test: the genotype matrices are NumPy code arrays written with
tests/pgen_writer.py, and every expected tally, unpack, validity word and LD sum is NumPy on those codes
(subset_shapes' references); dosages are test_dosage_tracks.make_dosage_file's own `want` matrix; plink_score's kept
rows are oracle.score's; Hardy-Weinberg ln p is held to test_hwe_exact's rational enumeration.

Every GPU test carries the gpu mark itself (not a module-wide pytestmark): test_references_and_guard_on_a_hand_case
runs the references and the guard helper without a device, wherever the suite runs.

Entry point -> its own test (each also appears in the calling-pattern tests at the end):
  pgh_counts_range_dev          test_counts_range_dev, test_counts_range_dev_sparse_resident
  pgh_freq_from_counts_dev      test_freq_from_counts_dev, test_benchmark_pipeline
  pgh_missing_per_sample_dev    test_missing_per_sample_dev (and the stream / thread tests)
  pgh_fused_tally_dev           test_fused_tally_dev, test_benchmark_pipeline
  pgh_hwe_lnp_batch_dev         test_hwe_lnp_batch_dev, test_benchmark_pipeline
  pgh_unpack_range_dev          test_unpack_range_dev
  pgh_sample_counts_dev         test_sample_counts_dev, test_sample_counts_dev_sparse_resident
  pgh_dosage_sums_dev           test_dosage_sums_dev
  pgh_dosage_unpack_dev         test_dosage_unpack_dev
  pgh_ld_pairs_dev, _status     test_ld_pairs_dev, test_ld_task_buffers_regrow_between_launches
  pgh_score_dev                 test_score_dev
  pgh_score_run_dev             test_score_run_dev
  pgh_probe_unpack_shape_dev    test_probe_unpack_shape_dev"""

import functools
import glob
import math
import os
import re
import threading

import numpy as np
import pytest

import pgen_writer as W
import subset_shapes as SS
from test_dosage_tracks import make_dosage_file
from test_hwe_exact import exact_tables

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5   # no count (0xA5A5A5A5 > any N x M here), call (-91), dosage or ln p (-1.9e-130) is made of these bytes
GUARD = 256     # bytes of poison on each side of an interior, at least
ALIGN = 256     # interiors start where hipMalloc's blocks do: every vector width the kernels store with is met
REL = 1e-6      # test_gpu_parity.test_score_matches_oracle's bound

# 63/64/65 straddle a validity word, 4099 is a ragged 16-byte lane, 16385 the first record of 4 KiB and more (the
# counts and LD kernels' workgroup forms, the wide unpack), 70001 a ragged wide row
WIDTHS = (1, 63, 64, 65, 1000, 4099, 16385, 70001)
VARIANTS = {1: 300, 63: 300, 64: 300, 65: 300, 1000: 200, 4099: 200, 16385: 96, 70001: 64}
DOSAGE_VARIANTS = {1: 60, 63: 60, 64: 60, 65: 60, 1000: 60, 4099: 60, 16385: 40, 70001: 40}
SPARSE_WIDTHS = (1, 65, 1000, 4099, 16385, 70001)
PATTERN_WIDTHS = (4099, 70001)  # the calling-pattern datasets: 200 x 4099 and 64 x 70001
SUBSETS = ("all_but_one", "last_word", "word_block", "stride4")
OFF = 17        # first variant of the dataset that is opened mid-file
MISSING_RATE = 0.06


def _cells(widths, names=SUBSETS):
    """(N, subset name or None) for every subset of the list that keeps somebody at N: no cell is ever skipped."""
    return [(n, s) for n in widths for s in (None,) + tuple(names) if s is None or SS.shapes(n)[s].any()]


CELLS = _cells(WIDTHS)
SPARSE_CELLS = _cells(SPARSE_WIDTHS, ("all_but_one", "stride4"))


def _id(cell):
    return f"{cell[0]}-{cell[1] or 'everyone'}"


# ---- the guarded output buffer -----------------------------------------------------------------------------------

class Guarded:
    """A tensor of POISON bytes with an interior of exactly `nbytes` that an entry point is handed (self.ptr): at
    least GUARD bytes of poison before and behind it, the interior ALIGN-aligned.  check() is the one place where
    this module looks at an output."""

    def __init__(self, nbytes, device="cuda"):
        import torch

        self.nbytes = int(nbytes)
        self.t = torch.full((GUARD + ALIGN + self.nbytes + GUARD,), POISON, dtype=torch.uint8, device=device)
        base = self.t.data_ptr()
        self.off = GUARD + (-(base + GUARD)) % ALIGN
        self.ptr = base + self.off
        assert self.off >= GUARD and self.t.numel() - self.off - self.nbytes >= GUARD and self.ptr % ALIGN == 0

    def image(self):
        """The interior as the call found it: what a byte the call must not touch still holds."""
        return np.full(self.nbytes, POISON, dtype=np.uint8)

    def _read(self):
        host = self.t.cpu().numpy()
        inner = host[self.off:self.off + self.nbytes]
        for name, g in (("front", host[:self.off]), ("back", host[self.off + self.nbytes:])):
            bad = np.flatnonzero(g != POISON)
            assert bad.size == 0, (f"{name} guard overwritten: {bad.size} bytes, the first {int(bad[0])} bytes into it "
                                   f"(interior of {self.nbytes} bytes)")
        return inner

    def check(self, expect, care=None):
        """(a) the interior equals `expect` byte for byte -- where `care` (bool per byte, default: everywhere) says
        the header specifies the byte -- and (b) both guards are poison."""
        inner = self._read()
        want = np.ascontiguousarray(expect).reshape(-1).view(np.uint8)
        assert want.size == self.nbytes, (want.size, self.nbytes)
        diff = inner != want
        if care is not None:
            diff &= np.asarray(care, dtype=bool).reshape(-1)
        bad = np.flatnonzero(diff)
        assert bad.size == 0, (f"{bad.size} of {self.nbytes} interior bytes differ; the first at byte {int(bad[0])}: "
                               f"got 0x{int(inner[bad[0]]):02x}, expected 0x{int(want[bad[0]]):02x}")

    def check_with(self, dtype, fn):
        """For outputs held to a tolerance: the guards as in check(), then fn(interior viewed as dtype)."""
        inner = self._read()
        fn(inner.copy().view(dtype))


def _sync():
    import torch

    torch.cuda.synchronize()


def _stream():
    import torch

    return torch.cuda.Stream()


def _upload(a):
    """A host array as a device tensor of its bytes (an INPUT of a call; outputs are Guarded)."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _in_fresh_thread(fn, timeout=120):
    """fn() on a thread the library has never seen (its PghThreadScratch list and LD task buffers start empty);
    joined with a time limit, its exception re-raised here."""
    box = []

    def run():
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 -- reported by the calling thread
            box.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join(timeout=timeout)
    assert not t.is_alive(), "the worker thread did not finish"
    if box:
        raise box[0]


# ---- references: NumPy on the codes, nothing of the library -------------------------------------------------------

def dense_codes(m, n):
    """(m, n) codes 0..3 (3 = missing, MISSING_RATE of the calls); row 3 all missing, row 4 monomorphic -- where
    subset_shapes.ld_pair_list expects them."""
    rng = np.random.default_rng(7000 + n)
    p = rng.uniform(0.05, 0.5, m)
    codes = rng.binomial(2, p[:, None], size=(m, n)).astype(np.uint8)
    codes[rng.random((m, n)) < MISSING_RATE] = 3
    codes[SS.ROW_ALL_MISSING] = 3
    codes[SS.ROW_MONO] = 0
    return codes


def missing_per_sample_ref(codes):
    return (codes == 3).sum(axis=0).astype(np.uint32)


def sample_classes_ref(codes):
    """uint32[3][ceil(n / 64) * 64]: het, hom-alt, missing per raw sample, the columns from n on zero."""
    n = codes.shape[1]
    out = np.zeros((3, (n + 63) // 64 * 64), dtype=np.uint32)
    for k, c in enumerate((1, 2, 3)):
        out[k, :n] = (codes == c).sum(axis=0)
    return out


def freq_ref(counts):
    """(alt_freq float64, obs_ct int32): (het + 2 hom_alt) / (2 obs) -- exact operands, one correctly rounded
    division, so the same bits as the device's -- NaN exactly where obs == 0; obs_ct = 2 obs."""
    c = np.asarray(counts, dtype=np.int64)
    obs = c[:, 0] + c[:, 1] + c[:, 2]
    af = np.full(len(c), np.nan)
    ok = obs > 0
    af[ok] = (c[ok, 1] + 2 * c[ok, 2]).astype(np.float64) / (2 * obs[ok]).astype(np.float64)
    return af, (2 * obs).astype(np.int32)


def unpack_image(g, codes, pitch, missing_code):
    """(expected bytes, care) of an unpack into Guarded g at row stride `pitch`: the calls, then -- unspecified by
    the header, so not compared -- the bytes up to the next multiple of 16, then poison up to the pitch."""
    rows, n_out = codes.shape
    img, care = g.image(), np.ones(g.nbytes, dtype=bool)
    c = codes.astype(np.int8)
    calls = np.where(c == 3, np.int8(missing_code), c).view(np.uint8)
    img2, care2 = img.reshape(rows, pitch), care.reshape(rows, pitch)
    img2[:, :n_out] = calls
    care2[:, n_out:(n_out + 15) // 16 * 16] = False
    return img, care


def ld_sums_ref(codes, a, b):
    """uint32[pairs][6] = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2} over the samples at which both calls are there."""
    planes = SS.ld_planes(codes)
    return planes[:, np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)].T.astype(np.uint32)


def ld_sums_loop(codes, a, b):
    """The same, pair by pair in integers (the self-check holds ld_sums_ref's BLAS form to it)."""
    out = np.zeros((len(a), 6), dtype=np.uint32)
    for i, (x, y) in enumerate(zip(a, b)):
        ga, gb = codes[x].astype(np.int64), codes[y].astype(np.int64)
        ok = (ga != 3) & (gb != 3)
        ga, gb = ga[ok], gb[ok]
        out[i] = (ok.sum(), ga.sum(), gb.sum(), (ga * gb).sum(), (ga * ga).sum(), (gb * gb).sum())
    return out


def score_ref_all(codes, vidx, weights, flip, mask, mean_impute=True):
    """plink_score phase 1 (oracle.score's "default" mode, or "no_mean_imputation") for EVERY raw sample, with the
    per-variant means and skips of the kept samples: what the device forms leave in their raw-order rows.  The kept
    rows are oracle.score's."""
    m, n = codes.shape
    keep = np.ones(n, dtype=bool) if mask is None else mask
    score, dos, ac = np.zeros((n, weights.shape[1])), np.zeros(n), np.zeros(n, dtype=np.uint32)
    for i, v in enumerate(vidx):
        d = codes[v].astype(np.float64)
        nm = codes[v] != 3
        sub = nm & keep
        if not sub.any():
            continue
        if mean_impute:
            alt = np.where(nm, d, float(d[sub].sum()) / int(sub.sum()))
            scored = (2.0 - alt) if flip[i] else alt
            ac += 2
        else:
            scored = np.where(nm, (2.0 - d) if flip[i] else d, 0.0)
            ac += 2 * nm.astype(np.uint32)
        score += np.outer(scored, weights[i])
        dos += scored
    return score, dos, ac


@functools.lru_cache(maxsize=None)
def hwe_exact(hom1, het, hom2):
    """(p, mid-p) of the exact test by test_hwe_exact's rational enumeration.  Without a single call there is no
    table to enumerate: the reference answers p = 1 before it asks plink2::HweLnP, mid-p or not
    (src/plink_hardy.cpp:73-75), and ln p = 0 is what pgenhip.h means by "the HWE ln p of zero counts"."""
    if hom1 + het + hom2 == 0:
        return 1.0, 1.0
    t = exact_tables(hom1 + het + hom2, 2 * hom1 + het)
    obs = t[het]
    total = sum(t.values())
    tail = sum(p for p in t.values() if p <= obs)
    eq = sum(p for p in t.values() if p == obs)
    return float(tail / total), float((tail - eq / 2) / total)


def hwe_float_ref(hom1, het, hom2, midp=False):
    """The same p in float64 for tables too large to enumerate in rationals: the ratio recurrence
    P(k + 2) / P(k) = 4 hr hc / ((k + 2)(k + 1)) run outwards from the mode.  Each table is a product of at most
    n / 2 correctly rounded factors (n = 70,001: 35,000 x 2^-53 = 4e-12 relative), far inside the 1e-9 the device is
    held to; tables within 1e-8 relative of the observed one count as equal to it (different tables are at least
    1e-6 apart, test_hwe_exact.test_no_two_different_tables_come_within_the_tie_band)."""
    n = hom1 + het + hom2
    if n == 0:
        return 1.0  # as hwe_exact
    a = 2 * hom1 + het
    rare, common = min(a, 2 * n - a), max(a, 2 * n - a)
    ks = np.arange(rare & 1, rare + 1, 2, dtype=np.float64)
    ratio = 4.0 * ((rare - ks[:-1]) / 2) * ((common - ks[:-1]) / 2) / ((ks[:-1] + 2) * (ks[:-1] + 1))
    mode = int(np.argmax(np.concatenate([[0.0], np.cumsum(np.log(ratio))])))
    t = np.ones(len(ks))
    t[mode + 1:] = np.cumprod(ratio[mode:])
    t[:mode] = np.cumprod((1.0 / ratio[:mode])[::-1])[::-1]
    obs = t[(het - (rare & 1)) // 2]
    tail = math.fsum(t[t <= obs * (1 + 1e-8)])
    if midp:
        tail -= 0.5 * math.fsum(t[np.abs(t - obs) <= 1e-8 * obs])
    return tail / math.fsum(t)


def hwe_order_min():
    """kHweOrderMin as the sources define it: from that many variants on the batch is tested in sorted order."""
    for path in sorted(glob.glob(os.path.join(ROOT, "plinking_duck_amd", "csrc", "*.h*"))):
        hit = re.search(r"constexpr\s+uint32_t\s+kHweOrderMin\s*=\s*(\d+)\s*;", open(path).read())
        if hit:
            return int(hit.group(1))
    raise AssertionError("kHweOrderMin is not defined in plinking_duck_amd/csrc")


def test_references_and_guard_on_a_hand_case():
    """Three variants, five samples, answers worked out by hand; and the guard helper catching what it is for."""
    codes = np.array([[0, 1, 2, 3, 1], [3, 3, 3, 3, 3], [0, 0, 0, 0, 0]], dtype=np.uint8)
    counts = SS.counts_ref(codes)
    assert counts.tolist() == [[1, 2, 1, 1], [0, 0, 0, 5], [5, 0, 0, 0]]
    assert SS.counts_ref(codes[:, [0, 2, 3]]).tolist() == [[1, 0, 1, 1], [0, 0, 0, 3], [3, 0, 0, 0]]
    assert missing_per_sample_ref(codes).tolist() == [1, 1, 1, 2, 1]
    cls = sample_classes_ref(codes)
    assert cls.shape == (3, 64) and cls[:, :5].tolist() == [[0, 1, 0, 0, 1], [0, 0, 1, 0, 0], [1, 1, 1, 2, 1]]
    assert not cls[:, 5:].any()
    af, obs = freq_ref(counts)
    assert af[0] == 0.5 and math.isnan(af[1]) and af[2] == 0.0 and obs.tolist() == [8, 0, 10] and obs.dtype == np.int32
    af, obs = freq_ref([[2 ** 29, 2 ** 28, 2 ** 28 - 1, 3]])
    assert obs[0] == 2 ** 31 - 2 and af[0] == (2 ** 28 + 2 * (2 ** 28 - 1)) / (2 ** 31 - 2)
    assert SS.validity_ref(codes).reshape(-1).tolist() == [0b10111, 0, 0b11111]
    pairs = ([0, 0, 0, 2], [2, 0, 1, 0])
    want = [[4, 4, 0, 0, 6, 0], [4, 4, 4, 6, 6, 6], [0, 0, 0, 0, 0, 0], [4, 0, 4, 0, 0, 6]]
    assert ld_sums_loop(codes, *pairs).tolist() == want and ld_sums_ref(codes, *pairs).tolist() == want
    rng = np.random.default_rng(1)
    big = dense_codes(12, 77)
    a, b = rng.integers(0, 12, 30), rng.integers(0, 12, 30)
    assert np.array_equal(ld_sums_ref(big, a, b), ld_sums_loop(big, a, b))
    assert (big[SS.ROW_ALL_MISSING] == 3).all() and not big[SS.ROW_MONO].any()
    assert SS.dosage_moments_ref([np.array([0.5, -9.0, 2.0])]).tolist() == [[40960, 8192 ** 2 + 32768 ** 2, 2]]
    # Hardy-Weinberg: 4 individuals, 4 copies: P(0 hets) : P(2) : P(4) = 1 : 8 : 8/3
    assert hwe_exact(1, 2, 1) == pytest.approx((1.0, 23 / 35), rel=1e-15)
    assert hwe_exact(2, 0, 2) == pytest.approx((3 / 35, 3 / 70), rel=1e-15)
    assert hwe_exact(0, 0, 0) == (1.0, 1.0) and hwe_exact(7, 0, 0) == (1.0, 0.5)
    for row in [(1, 2, 1), (2, 0, 2), (0, 0, 0), (7, 0, 0), (3, 1, 0), (40, 11, 9), (1200, 500, 300), (10, 1990, 0)]:
        for midp in (False, True):
            assert hwe_float_ref(*row, midp) == pytest.approx(hwe_exact(*row)[midp], rel=1e-11, abs=1e-300), row
    assert hwe_order_min() >= 2
    # plink_score: one variant, weight 1: the missing sample gets the mean of the kept ones (1 and 2 -> 1.5)
    s, d, ac = score_ref_all(codes, [0], np.ones((1, 1)), [0], np.array([False, True, True, True, False]))
    assert s[:, 0].tolist() == [0.0, 1.0, 2.0, 1.5, 1.0] and d.tolist() == s[:, 0].tolist() and ac.tolist() == [2] * 5
    s, _, ac = score_ref_all(codes, [1, 0], np.ones((2, 1)), [0, 1], None)  # all-missing variant skipped; flipped
    assert s[:, 0].tolist() == [2.0, 1.0, 0.0, 1.0, 1.0] and ac.tolist() == [2] * 5
    s, d, ac = score_ref_all(codes, [0, 2], np.ones((2, 1)), [0, 1], None, mean_impute=False)  # missing: no term
    assert s[:, 0].tolist() == [2.0, 3.0, 4.0, 2.0, 3.0] and d.tolist() == s[:, 0].tolist()
    assert ac.tolist() == [4, 4, 4, 2, 4]
    # the unpack image: 2 rows of 5 calls at pitch 32: calls, 11 unspecified bytes, 16 of poison
    g = Guarded(64, device="cpu")
    img, care = unpack_image(g, codes[:2], 32, -9)
    assert img.view(np.int8)[:5].tolist() == [0, 1, 2, -9, 1] and img.view(np.int8)[32:37].tolist() == [-9] * 5
    assert care[:5].all() and not care[5:16].any() and care[16:32].all() and (img[16:32] == POISON).all()
    # the guard helper: an untouched buffer is all poison; a written interior passes; every kind of damage is seen
    assert g.ptr % ALIGN == 0 and g.off >= GUARD and g.t.numel() - g.off - g.nbytes >= GUARD
    g.check(g.image())
    host = g.t.numpy()  # shares the tensor's memory
    host[g.off:g.off + 64] = img
    host[g.off + 7] = 0  # an unspecified byte
    g.check(img, care)
    with pytest.raises(AssertionError, match="interior bytes differ"):
        g.check(img)
    host[g.off + 20] = 0  # pitch padding that must stay poison
    with pytest.raises(AssertionError, match="interior bytes differ"):
        g.check(img, care)
    host[g.off + 20] = POISON
    for where, name in ((g.off - 1, "front"), (g.off + 64, "back"), (0, "front"), (g.t.numel() - 1, "back")):
        host[where] = 0
        with pytest.raises(AssertionError, match=name + " guard overwritten"):
            g.check(img, care)
        with pytest.raises(AssertionError, match=name + " guard overwritten"):
            g.check_with(np.uint8, lambda x: None)
        host[where] = POISON
    g.check(img, care)
    empty = Guarded(0, device="cpu")
    empty.check(np.zeros((0, 4), dtype=np.uint32))
    seen = []
    g.check_with(np.int8, lambda x: seen.append(x[:5].tolist()))
    assert seen == [[0, 1, 2, -9, 1]]


# ---- the datasets ------------------------------------------------------------------------------------------------

class DenseWorld:
    """VARIANTS[n] x n codes written as a .pgen of mixed record types, resident whole (ds) and from OFF on (ds_off)."""

    def __init__(self, L, root, n):
        self.L, self.n, self.m = L, n, VARIANTS[n]
        self.codes = dense_codes(self.m, n)
        self.path = os.path.join(root, f"dense_{n}.pgen")
        W.write_pgen(self.path, self.codes, W.choose_kinds(self.codes, np.random.default_rng(n)))
        self.ds = L.Dataset.open(self.path)
        assert (self.ds.v_begin, self.ds.v_end, self.ds.n_samples) == (0, self.m, n)
        self._off, self._subsets = None, {}

    @property
    def ds_off(self):
        if self._off is None:
            self._off = self.L.Dataset.open(self.path, variant_begin=OFF, variant_end=self.m - 3)
            assert (self._off.v_begin, self._off.v_end) == (OFF, self.m - 3)
        return self._off

    def subset(self, ds, shape):
        """(mask, Subset) of a shape name on one of the world's datasets; (None, None) for everyone."""
        if shape is None:
            return None, None
        key = (id(ds), shape)
        if key not in self._subsets:
            mask = SS.shapes(self.n)[shape]
            self._subsets[key] = (mask, ds.subset(mask))
        return self._subsets[key]

    def view(self, shape):
        return self.codes if shape is None else self.codes[:, SS.shapes(self.n)[shape]]


class RareWorld(DenseWorld):
    """120 x n rare-variant rows (pgen_writer.rare_matrix: every majority code), sparse-resident."""

    def __init__(self, L, root, n):  # noqa: super().__init__ not called -- another matrix, other datasets
        self.L, self.n, self.m = L, n, 120
        self.codes = W.rare_matrix(self.m, n, np.random.default_rng(9000 + n))
        self.path = os.path.join(root, f"rare_{n}.pgen")
        W.write_pgen(self.path, self.codes, W.choose_kinds(self.codes, np.random.default_rng(n)))
        self._subsets, self._sparse = {}, {}

    def sparse(self, max_minor):
        if max_minor not in self._sparse:
            ds = self.L.Dataset.open(self.path, sparse=True, max_minor=max_minor)
            assert ds.sparse_info().sparse_variant_ct + ds.sparse_info().dense_variant_ct == self.m
            self._sparse[max_minor] = ds
        return self._sparse[max_minor]


class DosageWorld(DenseWorld):
    """test_dosage_tracks.make_dosage_file: track kinds 0, 0x20, 0x40 and 0x60; `want` is the dosage matrix."""

    def __init__(self, L, root, n):  # noqa: super().__init__ not called
        self.L, self.n, self.m = L, n, DOSAGE_VARIANTS[n]
        self.path = os.path.join(root, f"dosage_{n}.pgen")
        _, _, kinds, self.want = make_dosage_file(self.path, self.m, n, 400 + n, False)
        assert set(kinds) == {0, 0x20, 0x40, 0x60}
        self.ds = L.Dataset.open(self.path)
        self._subsets = {}

    def view(self, shape):
        return self.want if shape is None else self.want[:, SS.shapes(self.n)[shape]]


class Worlds:
    def __init__(self, L, root):
        self.L, self.root, self._made = L, str(root), {}

    def _get(self, cls, n):
        if (cls, n) not in self._made:
            self._made[(cls, n)] = cls(self.L, self.root, n)
        return self._made[(cls, n)]

    def dense(self, n):
        return self._get(DenseWorld, n)

    def rare(self, n):
        return self._get(RareWorld, n)

    def dosage(self, n):
        return self._get(DosageWorld, n)


@pytest.fixture(scope="module")
def worlds(gpu_lib, tmp_path_factory):
    """Every matrix is made, written and opened once and shared by the tests that need it."""
    return Worlds(gpu_lib, tmp_path_factory.mktemp("device_entry_points"))


def _ranges(m):
    """Whole range, a sub-range that starts past the dataset's first variant, an empty range inside."""
    return [(0, m), (5, m - 7), (9, 9)]


# ---- 1: pgh_counts_range_dev ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_counts_range_dev(gpu_lib, worlds, cell):
    """uint32[v_end - v_begin][4], over the subset's samples when there is one; sub-ranges past v_begin; a dataset
    whose own first variant is OFF; v_begin == v_end writes nothing (an empty interior between two guards)."""
    n, shape = cell
    w = worlds.dense(n)
    st = _stream()
    jobs = [(w.ds, v0, v1) for v0, v1 in _ranges(w.m)] + [(w.ds_off, OFF, w.m - 3), (w.ds_off, OFF + 4, OFF + 30),
                                                             (w.ds_off, OFF + 9, OFF + 9)]
    bufs = [Guarded(16 * (v1 - v0)) for _, v0, v1 in jobs]
    _sync()
    for (ds, v0, v1), g in zip(jobs, bufs):
        ds.counts_range_dev(v0, v1, g.ptr, st.cuda_stream, subset=w.subset(ds, shape)[1])
    _sync()
    ref = SS.counts_ref(w.view(shape))
    for (ds, v0, v1), g in zip(jobs, bufs):
        g.check(ref[v0:v1])


@gpu
@pytest.mark.parametrize("cell", SPARSE_CELLS, ids=_id)
def test_counts_range_dev_sparse_resident(gpu_lib, worlds, cell):
    """The sparse branch of the device form (pgh_sparse::CountsRangeDev): rows kept as carrier lists, as pool rows
    (max_minor 0: whichever is smaller) or all as lists (max_minor = N)."""
    n, shape = cell
    w = worlds.rare(n)
    st = _stream()
    ref = SS.counts_ref(w.view(shape))
    for max_minor in (0, n):
        ds = w.sparse(max_minor)
        jobs = _ranges(w.m)
        bufs = [Guarded(16 * (v1 - v0)) for v0, v1 in jobs]
        _sync()
        for (v0, v1), g in zip(jobs, bufs):
            ds.counts_range_dev(v0, v1, g.ptr, st.cuda_stream, subset=w.subset(ds, shape)[1])
        _sync()
        for (v0, v1), g in zip(jobs, bufs):
            g.check(ref[v0:v1])


# ---- 2: pgh_freq_from_counts_dev -----------------------------------------------------------------------------------

HAND_COUNTS = np.array([
    [0, 0, 0, 0], [0, 0, 0, 77],                               # obs == 0: NaN, obs_ct 0
    [5, 0, 0, 0], [0, 0, 9, 1], [0, 12, 0, 0],                 # monomorphic REF / ALT, all het
    [2 ** 29, 2 ** 28, 2 ** 28 - 1, 3], [1, 2 ** 30 - 2, 0, 0], [0, 0, 2 ** 30 - 1, 5], [2 ** 30 - 1, 0, 0, 0],
    [1, 1, 1, 0], [3, 0, 1, 2 ** 31],                          # 2 obs = 2^31 - 2 still fits int32
], dtype=np.uint32)


@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_freq_from_counts_dev(gpu_lib, worlds, n):
    """From the counts a counts kernel has just left on the same stream, and from hand-made rows: ALT_FREQ bit for
    bit (NaN exactly where obs == 0), OBS_CT = 2 obs as int32; n == 0 with NULL pointers is PGH_OK."""
    L = gpu_lib
    w = worlds.dense(n)
    st = _stream()
    d_counts, d_freq, d_obs = Guarded(16 * w.m), Guarded(8 * w.m), Guarded(4 * w.m)
    hand = _upload(HAND_COUNTS)
    h_freq, h_obs = Guarded(8 * len(HAND_COUNTS)), Guarded(4 * len(HAND_COUNTS))
    _sync()
    w.ds.counts_range_dev(0, w.m, d_counts.ptr, st.cuda_stream)
    L.freq_from_counts_dev(d_counts.ptr, w.m, d_freq.ptr, d_obs.ptr, st.cuda_stream)
    L.freq_from_counts_dev(hand.data_ptr(), len(HAND_COUNTS), h_freq.ptr, h_obs.ptr, st.cuda_stream)
    L.freq_from_counts_dev(None, 0, None, None, st.cuda_stream)
    _sync()
    counts = SS.counts_ref(w.codes)
    d_counts.check(counts)
    for c, gf, go in ((counts, d_freq, d_obs), (HAND_COUNTS, h_freq, h_obs)):
        af, obs = freq_ref(c)
        assert np.array_equal(np.isnan(af), (c[:, :3].astype(np.int64).sum(axis=1) == 0))
        gf.check(af)
        go.check(obs)


# ---- 3 and 4: pgh_missing_per_sample_dev, pgh_fused_tally_dev ------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_missing_per_sample_dev(gpu_lib, worlds, n):
    """d_out: uint32[raw_sample_ct] -- N elements, not ceil(N / 64) * 64 -- zeroed by the call: the poison is replaced
    by the counts, zeros included; a zero-variant range leaves all zeros."""
    w = worlds.dense(n)
    st = _stream()
    jobs = [(w.ds, v0, v1) for v0, v1 in _ranges(w.m)] + [(w.ds_off, OFF, w.m - 3), (w.ds_off, OFF + 4, OFF + 30)]
    bufs = [Guarded(4 * n) for _ in jobs]
    _sync()
    for (ds, v0, v1), g in zip(jobs, bufs):
        ds.missing_per_sample_dev(v0, v1, g.ptr, st.cuda_stream)
    _sync()
    for (ds, v0, v1), g in zip(jobs, bufs):
        want = missing_per_sample_ref(w.codes[v0:v1])
        assert v1 > v0 or not want.any()
        g.check(want)


@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_fused_tally_dev(gpu_lib, worlds, n):
    """Both outputs guarded: d_counts as pgh_counts_range_dev (all samples), d_missing exactly N uint32 as
    pgh_missing_per_sample_dev, and both equal what those two calls give and the reference."""
    w = worlds.dense(n)
    st = _stream()
    jobs = [(w.ds, v0, v1) for v0, v1 in _ranges(w.m)] + [(w.ds_off, OFF, w.m - 3), (w.ds_off, OFF + 4, OFF + 30)]
    bufs = [[Guarded(16 * (v1 - v0)), Guarded(4 * n), Guarded(16 * (v1 - v0)), Guarded(4 * n)] for _, v0, v1 in jobs]
    _sync()
    for (ds, v0, v1), (fc, fm, c, m) in zip(jobs, bufs):
        ds.fused_tally_dev(v0, v1, fc.ptr, fm.ptr, st.cuda_stream)
        ds.counts_range_dev(v0, v1, c.ptr, st.cuda_stream)
        ds.missing_per_sample_dev(v0, v1, m.ptr, st.cuda_stream)
    _sync()
    ref = SS.counts_ref(w.codes)
    for (ds, v0, v1), (fc, fm, c, m) in zip(jobs, bufs):
        for g in (fc, c):
            g.check(ref[v0:v1])
        for g in (fm, m):
            g.check(missing_per_sample_ref(w.codes[v0:v1]))


# ---- 5: pgh_hwe_lnp_batch_dev --------------------------------------------------------------------------------------

def _hwe_pool(total, counts_head):
    """`total` count rows: the head is what a counts kernel will write (reference values here), then hand-made
    rows -- empty, monomorphic, all het -- and random tables of up to 60 individuals, a few of 2,000."""
    rng = np.random.default_rng(total)
    rows = [(0, 0, 0, 0), (0, 0, 0, 9), (31, 0, 0, 2), (0, 0, 17, 0), (0, 40, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0)]
    for _ in range(8):
        a = int(rng.integers(1, 2001))
        ks = sorted(exact_tables(2000, a))
        het = int(rng.choice(ks))
        h1 = (a - het) // 2
        if 2000 - het - h1 >= 0:
            rows.append((h1, het, 2000 - het - h1, 0))
    pool = np.zeros((total, 4), dtype=np.uint32)
    k = len(counts_head)
    pool[:k] = counts_head
    pool[k:k + len(rows)] = rows
    rest = total - k - len(rows)
    ind = rng.integers(0, 61, rest)
    h1 = (rng.random(rest) * (ind + 1)).astype(np.int64)
    het = (rng.random(rest) * (ind - h1 + 1)).astype(np.int64)
    pool[k + len(rows):] = np.stack([h1, het, ind - h1 - het, rng.integers(0, 5, rest)], axis=1)
    return pool


@gpu
@pytest.mark.parametrize("midp", [False, True])
@pytest.mark.parametrize("where", ["below", "at", "above"])
def test_hwe_lnp_batch_dev(gpu_lib, worlds, where, midp):
    """n on both sides of the ordered-path threshold (kHweOrderMin: threshold - 1, threshold, threshold + 257), on
    a side stream behind an event recorded after the counts kernel that writes the head of the batch on another
    stream -- the benchmark's shape.  exp(ln p) within 1e-9 relative of the rational enumeration (the bound of
    test_device_exact_tests_against_the_rational_enumeration); bit-identical to hwe_lnp_batch as a second check."""
    import torch

    L = gpu_lib
    t = hwe_order_min()
    total = {"below": t - 1, "at": t, "above": t + 257}[where]
    w = worlds.dense(65)
    head = SS.counts_ref(w.codes)
    pool = _hwe_pool(total, head)
    main, side = _stream(), _stream()
    d_counts, d_lnp = Guarded(16 * total), Guarded(8 * total)
    hand = _upload(pool[len(head):])
    _sync()
    with torch.cuda.stream(main):  # the hand-made rows behind the head, device to device on the main stream
        d_counts.t[d_counts.off + 16 * len(head):d_counts.off + 16 * total].copy_(hand, non_blocking=True)
    w.ds.counts_range_dev(0, w.m, d_counts.ptr, main.cuda_stream)
    tallied = torch.cuda.Event()
    tallied.record(main)
    side.wait_event(tallied)
    L.hwe_lnp_batch_dev(d_counts.ptr, total, d_lnp.ptr, midp, side.cuda_stream)
    _sync()
    d_counts.check(pool)
    want = np.array([hwe_exact(int(r[0]), int(r[1]), int(r[2]))[midp] for r in pool])
    twin = L.hwe_lnp_batch(pool, midp)

    def close(lnp):
        assert np.allclose(np.exp(lnp), want, rtol=1e-9, atol=1e-300), int(np.argmax(np.abs(np.exp(lnp) - want)))
        assert empty.sum() >= 3 and (lnp[empty] == 0.0).all()  # no calls: p = 1, mid-p or not
        assert np.array_equal(lnp.view(np.uint64), twin.view(np.uint64))

    empty = pool[:, :3].sum(axis=1) == 0
    d_lnp.check_with(np.float64, close)


# ---- 6: pgh_unpack_range_dev ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_unpack_range_dev(gpu_lib, worlds, cell):
    """out_pitch at the minimum ceil16(n_out) and 64 wider (bytes [ceil16(n_out), out_pitch) of every row stay
    poison; bytes [n_out, ceil16(n_out)) are unspecified and not compared), missing_code -9 and 0, d_out only,
    d_validity only and both -- the plain kernels without a subset, the gather kernel with one.  Validity words equal
    the reference, the bits at and past n_out clear.  A pitch that is no multiple of 16 or too small is refused and
    leaves the buffers poison."""
    L = gpu_lib
    n, shape = cell
    w = worlds.dense(n)
    ss = w.subset(w.ds, shape)[1]
    codes = w.view(shape)
    n_out = codes.shape[1]
    v0, v1 = 2, 42  # rows 3 (all missing) and 4 (monomorphic) among them
    rows, min_pitch, words = v1 - v0, (n_out + 15) // 16 * 16, (n_out + 63) // 64
    st = _stream()
    jobs = [(extra, code, want_out, want_val) for extra in (0, 64) for code in (-9, 0)
            for want_out, want_val in ((True, False), (False, True), (True, True))]
    bufs = [(Guarded(rows * (min_pitch + extra)) if o else None, Guarded(8 * rows * words) if v else None)
            for extra, _, o, v in jobs]
    bad_out, bad_val = Guarded(rows * (min_pitch + 64)), Guarded(8 * rows * words)
    _sync()
    for (extra, code, _, _), (go, gv) in zip(jobs, bufs):
        w.ds.unpack_range_dev(v0, v1, go.ptr if go else None, min_pitch + extra, gv.ptr if gv else None, code,
                              st.cuda_stream, subset=ss)
    for pitch in (min_pitch + 8, min_pitch - 16, 0):
        with pytest.raises(L.PghArgError) as e:
            w.ds.unpack_range_dev(v0, v1, bad_out.ptr, pitch, bad_val.ptr, -9, st.cuda_stream, subset=ss)
        assert e.value.code == L.PGH_ERR_ARG
    _sync()
    validity = SS.validity_ref(codes[v0:v1])
    assert n_out % 64 == 0 or not (validity[:, -1] >> np.uint64(n_out % 64)).any()
    for (extra, code, _, _), (go, gv) in zip(jobs, bufs):
        if go:
            go.check(*unpack_image(go, codes[v0:v1], min_pitch + extra, code))
        if gv:
            gv.check(validity)
    bad_out.check(bad_out.image())
    bad_val.check(bad_val.image())


# ---- 7: pgh_sample_counts_dev --------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", WIDTHS)
def test_sample_counts_dev(gpu_lib, worlds, n):
    """uint32[3][ceil(N / 64) * 64]: het, hom-alt, missing (hom-ref by subtraction).  Columns [N, padded) are inside
    the extent and zero (the code's memset); nothing past the extent is touched."""
    w = worlds.dense(n)
    padded = (n + 63) // 64 * 64
    st = _stream()
    jobs = [(w.ds, v0, v1) for v0, v1 in _ranges(w.m)] + [(w.ds_off, OFF, w.m - 3), (w.ds_off, OFF + 4, OFF + 30)]
    bufs = [Guarded(12 * padded) for _ in jobs]
    _sync()
    for (ds, v0, v1), g in zip(jobs, bufs):
        ds.sample_counts_dev(v0, v1, g.ptr, st.cuda_stream)
    _sync()
    for (ds, v0, v1), g in zip(jobs, bufs):
        cls = sample_classes_ref(w.codes[v0:v1])
        hom_ref = (v1 - v0) - cls[:, :n].sum(axis=0)
        assert np.array_equal(hom_ref, (w.codes[v0:v1] == 0).sum(axis=0))
        g.check(cls)


@gpu
@pytest.mark.parametrize("n", SPARSE_WIDTHS)
def test_sample_counts_dev_sparse_resident(gpu_lib, worlds, n):
    """The sparse branch of the device form (pgh_sparse::SampleClasses): the same extent and the same zeros."""
    w = worlds.rare(n)
    padded = (n + 63) // 64 * 64
    st = _stream()
    for max_minor in (0, n):
        ds = w.sparse(max_minor)
        jobs = _ranges(w.m)
        bufs = [Guarded(12 * padded) for _ in jobs]
        _sync()
        for (v0, v1), g in zip(jobs, bufs):
            ds.sample_counts_dev(v0, v1, g.ptr, st.cuda_stream)
        _sync()
        for (v0, v1), g in zip(jobs, bufs):
            g.check(sample_classes_ref(w.codes[v0:v1]))


# ---- 8: pgh_dosage_sums_dev, pgh_dosage_unpack_dev -----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_dosage_sums_dev(gpu_lib, worlds, cell):
    """d_sums = uint64[n][3] over the written dosage file (track kinds 0, 0x20, 0x40, 0x60), with and without a
    subset; an empty range writes nothing; a NULL d_sums for a non-empty range is PGH_ERR_ARG."""
    L = gpu_lib
    n, shape = cell
    w = worlds.dosage(n)
    ss = w.subset(w.ds, shape)[1]
    st = _stream()
    jobs = [(0, w.m), (3, w.m - 5), (6, 6)]
    bufs = [Guarded(24 * (v1 - v0)) for v0, v1 in jobs]
    _sync()
    for (v0, v1), g in zip(jobs, bufs):
        w.ds.dosage_sums_dev(v0, v1, g.ptr, st.cuda_stream, subset=ss)
    with pytest.raises(L.PghArgError) as e:
        w.ds.dosage_sums_dev(0, w.m, None, st.cuda_stream, subset=ss)
    assert e.value.code == L.PGH_ERR_ARG
    _sync()
    ref = SS.dosage_moments_ref(w.view(shape))
    for (v0, v1), g in zip(jobs, bufs):
        g.check(ref[v0:v1])


@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_dosage_unpack_dev(gpu_lib, worlds, cell):
    """d_out = double rows of out_stride elements: out_stride == n_out and n_out + 3 (the stride padding stays
    poison), -9.0 where a sample has neither a dosage nor a call; a NULL d_out or a stride below n_out is
    PGH_ERR_ARG and writes nothing."""
    L = gpu_lib
    n, shape = cell
    w = worlds.dosage(n)
    ss = w.subset(w.ds, shape)[1]
    want = w.view(shape)
    n_out = want.shape[1]
    st = _stream()
    jobs = [(v0, v1, n_out + extra) for v0, v1 in [(0, w.m), (3, w.m - 5), (6, 6)] for extra in (0, 3)]
    bufs = [Guarded(8 * (v1 - v0) * stride) for v0, v1, stride in jobs]
    bad = Guarded(8 * w.m * n_out)
    _sync()
    for (v0, v1, stride), g in zip(jobs, bufs):
        w.ds.dosage_unpack_dev(v0, v1, g.ptr, stride, st.cuda_stream, subset=ss)
    for d_out, stride in ((None, n_out), (bad.ptr, n_out - 1)):
        with pytest.raises(L.PghArgError) as e:
            w.ds.dosage_unpack_dev(0, w.m, d_out, stride, st.cuda_stream, subset=ss)
        assert e.value.code == L.PGH_ERR_ARG
    _sync()
    for (v0, v1, stride), g in zip(jobs, bufs):
        img = g.image().view(np.float64).reshape(v1 - v0, stride)
        img[:, :n_out] = want[v0:v1]
        g.check(img)
    bad.check(bad.image())


# ---- 9: pgh_ld_pairs_dev, pgh_ld_pairs_status ----------------------------------------------------------------------

def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


@gpu
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_ld_pairs_dev(gpu_lib, worlds, cell):
    """test_ld_pair_sums_match_oracle's pair list (anchors with 1..9 consecutive partners, a repeated, a reversed and
    a self pair, the all-missing with the monomorphic row), with and without a subset: d_sums zeroed by the call and
    filled, the status PGH_OK afterwards; n_pairs == 0 is PGH_OK and touches nothing."""
    L = gpu_lib
    n, shape = cell
    w = worlds.dense(n)
    ss = w.subset(w.ds, shape)[1]
    a, b = SS.ld_pair_list(n)
    a, b = _u32(a + [0]), _u32(b + [1])  # (0, 1) a second time: a repeated pair is a repeated row
    none = _u32([])
    st = _stream()
    g, untouched = Guarded(24 * len(a)), Guarded(24)
    _sync()
    w.ds.ld_pairs_dev(a, b, g.ptr, st.cuda_stream, subset=ss)
    w.ds.ld_pairs_dev(none, none, untouched.ptr, st.cuda_stream, subset=ss)
    L.ld_pairs_status()
    _sync()
    ref = ld_sums_ref(w.view(shape), a, b)
    assert not ref[-2].any() and np.array_equal(ref[-1], ref[0])  # the all-missing row; the repeat
    g.check(ref)
    untouched.check(untouched.image())


# ---- 10: pgh_score_dev ---------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("ncols", [1, 4])
@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_score_dev(gpu_lib, oracle, worlds, cell, ncols):
    """One pass (1 and 4 weight columns), raw-sample order: the kept rows equal oracle.score within
    test_score_matches_oracle's bound.  The rows of samples outside the subset are overwritten as well -- not with
    zeros: the kernels score every raw sample, with the per-variant means of the kept ones (pgenhip.h says so since
    this test) -- so they equal the same arithmetic carried out for those samples, and nothing is left as poison."""
    L = gpu_lib
    n, shape = cell
    w = worlds.dense(n)
    mask, ss = w.subset(w.ds, shape)
    rng = np.random.default_rng(100 * n + ncols)
    vidx = np.union1d(rng.choice(w.m, size=35, replace=False), [SS.ROW_ALL_MISSING, SS.ROW_MONO]).astype(np.uint32)
    weights = rng.standard_normal((len(vidx), ncols))
    flip = (rng.random(len(vidx)) < 0.3).astype(np.uint8)
    st = _stream()
    g_s, g_d, g_a = Guarded(8 * n * ncols), Guarded(8 * n), Guarded(4 * n)
    _sync()
    w.ds.score_dev(vidx, weights, g_s.ptr, g_d.ptr, g_a.ptr, flip, L.SCORE_MEAN_IMPUTE, st.cuda_stream, subset=ss)
    _sync()
    keep = np.ones(n, dtype=bool) if mask is None else mask
    es, ed, eac = oracle.score(oracle.Pgen(w.path), vidx, weights, flip=flip, include=None if mask is None else
                               mask.astype(np.uint8))
    rs, rd, rac = score_ref_all(w.codes, vidx, weights, flip, mask)
    scale = np.abs(weights).sum(axis=0) * 2.0  # magnitude of the terms being summed

    def near(got, want):
        return np.all(np.abs(got - want) <= REL * np.maximum(np.abs(want), 1e-9 * scale))

    def scores(s):
        s = s.reshape(n, ncols)
        assert near(s[keep], es)
        assert near(s[~keep], rs[~keep])

    def dosages(d):
        assert np.allclose(d[keep], ed, rtol=REL, atol=1e-9)
        assert np.allclose(d[~keep], rd[~keep], rtol=REL, atol=1e-9)

    assert np.array_equal(rac[keep], eac) and near(rs[keep], es)  # the two references agree where both speak
    g_s.check_with(np.float64, scores)
    g_d.check_with(np.float64, dosages)
    g_a.check(rac)


# ---- 11 and 12: the two further device forms lib.py wraps: pgh_score_run_dev, pgh_probe_unpack_shape_dev ----------

@gpu
@pytest.mark.parametrize("mode", ["default", "no_mean_imputation"])
@pytest.mark.parametrize("n", (65, 4099, 70001))
def test_score_run_dev(gpu_lib, oracle, worlds, n, mode):
    """The enqueue-only half of plink_score: two plans (other weights, other flips) run A, B, A on one stream into one
    set of guarded buffers with no synchronisation in between -- each run zeroes and refills its outputs, so the set
    holds A's result -- and once more without the dosage sum (d_dosage_sum NULL).  no_mean_imputation takes its
    missing counts through a PghThreadScratch block of the stream."""
    L = gpu_lib
    w = worlds.dense(n)
    mask, ss = w.subset(w.ds, "all_but_one")
    code = {"default": L.SCORE_MEAN_IMPUTE, "no_mean_imputation": L.SCORE_NO_MEAN_IMPUTATION}[mode]
    rng = np.random.default_rng(n + code)
    vidx = np.union1d(rng.choice(w.m, size=30, replace=False), [SS.ROW_ALL_MISSING, SS.ROW_MONO]).astype(np.uint32)
    sets = [(rng.standard_normal((len(vidx), 3)), (rng.random(len(vidx)) < 0.3).astype(np.uint8)) for _ in range(2)]
    plans = [w.ds.score_plan(vidx, wt, fl, code, ss) for wt, fl in sets]
    st = _stream()
    g_s, g_d, g_a = Guarded(24 * n), Guarded(8 * n), Guarded(4 * n)
    h_s, h_d, h_a = Guarded(24 * n), Guarded(8 * n), Guarded(4 * n)
    _sync()
    for k in (0, 1, 0):
        plans[k].run_dev(g_s.ptr, g_d.ptr, g_a.ptr, st.cuda_stream)
    plans[1].run_dev(h_s.ptr, None, h_a.ptr, st.cuda_stream)
    _sync()
    for (wt, fl), (gs, gd, ga) in zip(sets, ((g_s, g_d, g_a), (h_s, None, h_a))):
        rs, rd, rac = score_ref_all(w.codes, vidx, wt, fl, mask, mean_impute=mode == "default")
        es, ed, eac = oracle.score(oracle.Pgen(w.path), vidx, wt, flip=fl, mode=mode, include=mask.astype(np.uint8))
        scale = np.abs(wt).sum(axis=0) * 2.0

        def near(got, want):
            return np.all(np.abs(got - want) <= REL * np.maximum(np.abs(want), 1e-9 * scale))

        assert np.array_equal(rac[mask], eac) and near(rs[mask], es) and np.allclose(rd[mask], ed, rtol=REL, atol=1e-9)
        def scores(x):
            assert near(x.reshape(n, 3), rs)

        gs.check_with(np.float64, scores)
        if gd is not None:
            gd.check_with(np.float64, lambda x: np.testing.assert_allclose(x, rd, rtol=REL, atol=1e-9))
        ga.check(rac)
    h_d.check(h_d.image())  # never handed to the library
    for p in plans:
        p.close()


@gpu
@pytest.mark.parametrize("n_vec", [64, 64 * 5, 64 * 1031])
def test_probe_unpack_shape_dev(gpu_lib, n_vec):
    """bench.py's store-ceiling probe: d_dst n_vec x 64 B (a wave's 64 vectors, piece-major: vector i's k-th 16 bytes
    at 16-byte slot (i & ~63) * 4 + 64 k + (i & 63), its first word raised by k), d_val n_vec x 8 B (the first word).
    A ragged n_vec, whose last wave would store past d_dst, is refused and writes nothing."""
    L = gpu_lib
    rng = np.random.default_rng(n_vec)
    src = rng.integers(0, 2 ** 32 - 8, size=(n_vec, 4), dtype=np.uint32)
    d_src = _upload(src)
    g_dst, g_val = Guarded(64 * n_vec), Guarded(8 * n_vec)
    bad_dst, bad_val = Guarded(64 * 65), Guarded(8 * 65)
    st = _stream()
    _sync()
    L.probe_unpack_shape_dev(d_src.data_ptr(), n_vec, g_dst.ptr, g_val.ptr, st.cuda_stream)
    for ragged in (1, 63, 65):
        with pytest.raises(L.PghArgError) as e:
            L.probe_unpack_shape_dev(d_src.data_ptr(), ragged, bad_dst.ptr, bad_val.ptr, st.cuda_stream)
        assert e.value.code == L.PGH_ERR_ARG
    L.probe_unpack_shape_dev(None, 0, None, None, st.cuda_stream)
    _sync()
    i = np.arange(n_vec)
    want = np.zeros((4 * n_vec, 4), dtype=np.uint32)
    for k in range(4):
        piece = src.copy()
        piece[:, 0] += k
        want[(i & ~63) * 4 + 64 * k + (i & 63)] = piece
    g_dst.check(want)
    g_val.check(src[:, 0].astype(np.uint64))
    bad_dst.check(bad_dst.image())
    bad_val.check(bad_val.image())


# ---- calling patterns ----------------------------------------------------------------------------------------------

def _three_ranges(m):
    """Three different ranges of one length."""
    span = m // 2
    return span, [(0, span), (m - span, m), (3, 3 + span)]


@gpu
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_benchmark_pipeline(gpu_lib, worlds, n):
    """bench.py's fused step, six times over two buffer sets with no host synchronisation: fused tally, then
    plink_freq's arithmetic on the main stream; an event; the side stream waits for it and runs the exact tests;
    the main stream waits for a set's `drained` event before it writes that set again.  The ranges go A B B A A B, so
    each set is overwritten with another range's results twice; after the one synchronise each set holds the results
    of the last range written into it."""
    import torch

    L = gpu_lib
    w = worlds.dense(n)
    span = w.m * 3 // 5
    ranges = [(0, span), (w.m - span, w.m)]
    main, side = _stream(), _stream()
    sets = [{"counts": Guarded(16 * span), "miss": Guarded(4 * n), "freq": Guarded(8 * span),
             "obs": Guarded(4 * span), "lnp": Guarded(8 * span)} for _ in range(2)]
    tallied = [torch.cuda.Event() for _ in range(2)]
    drained, last = [None, None], [None, None]
    _sync()
    for step, r in enumerate([0, 1, 1, 0, 0, 1]):
        b = step & 1
        s = sets[b]
        v0, v1 = ranges[r]
        if drained[b] is not None:
            main.wait_event(drained[b])  # the set is free again
        w.ds.fused_tally_dev(v0, v1, s["counts"].ptr, s["miss"].ptr, main.cuda_stream)
        L.freq_from_counts_dev(s["counts"].ptr, span, s["freq"].ptr, s["obs"].ptr, main.cuda_stream)
        tallied[b].record(main)
        side.wait_event(tallied[b])
        L.hwe_lnp_batch_dev(s["counts"].ptr, span, s["lnp"].ptr, False, side.cuda_stream)
        drained[b] = torch.cuda.Event()
        drained[b].record(side)
        last[b] = r
    _sync()
    assert last == [0, 1]
    for b in range(2):
        v0, v1 = ranges[last[b]]
        counts = SS.counts_ref(w.codes[v0:v1])
        af, obs = freq_ref(counts)
        sets[b]["counts"].check(counts)
        sets[b]["miss"].check(missing_per_sample_ref(w.codes[v0:v1]))
        sets[b]["freq"].check(af)
        sets[b]["obs"].check(obs)
        want = np.array([hwe_float_ref(int(c[0]), int(c[1]), int(c[2])) for c in counts])
        twin = L.hwe_lnp_batch(counts, False)

        def close(lnp):
            assert np.allclose(np.exp(lnp), want, rtol=1e-9, atol=1e-300)
            assert np.array_equal(lnp.view(np.uint64), twin.view(np.uint64))

        sets[b]["lnp"].check_with(np.float64, close)


def _pair_lists(n):
    """Three different pair lists of one length over variants 0..39."""
    a, b = SS.ld_pair_list(n)
    a, b = np.array(a), np.array(b)
    return [(_u32(a), _u32(b)), (_u32(b), _u32(a)), (_u32((7 * a + 1) % 40), _u32((3 * b + 2) % 40))]


FORMS = ["counts_range", "missing_per_sample", "unpack_range", "sample_counts", "dosage_sums", "dosage_unpack",
         "ld_pairs", "score"]


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_three_calls_back_to_back(gpu_lib, worlds, n, form):
    """Every device form outside the benchmark pipeline, three times on one stream into ONE guarded buffer, over
    different ranges (pair lists, weights), synchronised only after the third: the buffer holds the third result --
    overwrite and zeroing under stream order, without the host in between."""
    L = gpu_lib
    w = worlds.dosage(n) if form.startswith("dosage") else worlds.dense(n)
    ss_name = "stride4"
    mask, ss = w.subset(w.ds, ss_name)
    span, ranges = _three_ranges(w.m)
    st = _stream()
    s = st.cuda_stream
    v0, v1 = ranges[2]
    if form == "counts_range":
        g = Guarded(16 * span)
        _sync()
        for r0, r1 in ranges:
            w.ds.counts_range_dev(r0, r1, g.ptr, s, subset=ss)
        _sync()
        g.check(SS.counts_ref(w.view(ss_name)[v0:v1]))
    elif form == "missing_per_sample":
        g = Guarded(4 * n)
        _sync()
        for r0, r1 in ranges:
            w.ds.missing_per_sample_dev(r0, r1, g.ptr, s)
        _sync()
        g.check(missing_per_sample_ref(w.codes[v0:v1]))
    elif form == "unpack_range":
        pitch, words = (n + 15) // 16 * 16 + 64, (n + 63) // 64
        g, gv = Guarded(span * pitch), Guarded(8 * span * words)
        _sync()
        for (r0, r1), code in zip(ranges, (0, -9, 0)):
            w.ds.unpack_range_dev(r0, r1, g.ptr, pitch, gv.ptr, code, s)
        _sync()
        g.check(*unpack_image(g, w.codes[v0:v1], pitch, 0))
        gv.check(SS.validity_ref(w.codes[v0:v1]))
    elif form == "sample_counts":
        g = Guarded(12 * ((n + 63) // 64 * 64))
        _sync()
        for r0, r1 in ranges:
            w.ds.sample_counts_dev(r0, r1, g.ptr, s)
        _sync()
        g.check(sample_classes_ref(w.codes[v0:v1]))
    elif form == "dosage_sums":
        g = Guarded(24 * span)
        _sync()
        for r0, r1 in ranges:
            w.ds.dosage_sums_dev(r0, r1, g.ptr, s, subset=ss)
        _sync()
        g.check(SS.dosage_moments_ref(w.view(ss_name)[v0:v1]))
    elif form == "dosage_unpack":
        n_out = int(mask.sum())
        g = Guarded(8 * span * (n_out + 3))
        _sync()
        for r0, r1 in ranges:
            w.ds.dosage_unpack_dev(r0, r1, g.ptr, n_out + 3, s, subset=ss)
        _sync()
        img = g.image().view(np.float64).reshape(span, n_out + 3)
        img[:, :n_out] = w.view(ss_name)[v0:v1]
        g.check(img)
    elif form == "ld_pairs":
        lists = _pair_lists(n)
        g = Guarded(24 * len(lists[0][0]))
        _sync()
        for a, b in lists:
            w.ds.ld_pairs_dev(a, b, g.ptr, s, subset=ss)
        L.ld_pairs_status()
        _sync()
        g.check(ld_sums_ref(w.view(ss_name), *lists[2]))
    else:
        rng = np.random.default_rng(n)
        vidx = np.sort(rng.choice(w.m, size=30, replace=False)).astype(np.uint32)
        sets = [(rng.standard_normal((30, 2)), (rng.random(30) < 0.3).astype(np.uint8)) for _ in range(3)]
        g_s, g_d, g_a = Guarded(16 * n), Guarded(8 * n), Guarded(4 * n)
        _sync()
        for weights, flip in sets:
            w.ds.score_dev(vidx, weights, g_s.ptr, g_d.ptr, g_a.ptr, flip, L.SCORE_MEAN_IMPUTE, s, subset=ss)
        _sync()
        weights, flip = sets[2]
        rs, rd, rac = score_ref_all(w.codes, vidx, weights, flip, mask)
        scale = np.abs(weights).sum(axis=0) * 2.0
        g_s.check_with(np.float64, lambda x: np.testing.assert_array_less(
            np.abs(x.reshape(n, 2) - rs), REL * np.maximum(np.abs(rs), 1e-9 * scale) + 1e-300))
        g_d.check_with(np.float64, lambda x: np.testing.assert_allclose(x, rd, rtol=REL, atol=1e-9))
        g_a.check(rac)


@gpu
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_two_streams_one_thread(gpu_lib, worlds, n):
    """pgh_missing_per_sample_dev and pgh_sample_counts_dev alternately on streams A and B of one thread, over
    different ranges, no synchronisation until the end: the scratch block is keyed by stream, so what A's first
    kernel left for its second is not B's to overwrite.  All four results must be right."""
    w = worlds.dense(n)
    padded = (n + 63) // 64 * 64
    sa, sb = _stream(), _stream()
    span = w.m // 2
    jobs = [("missing", sa, 0, span), ("classes", sb, w.m - span, w.m), ("missing", sb, 3, 3 + span),
            ("classes", sa, 1, w.m - 1)]
    bufs = [Guarded(4 * n if kind == "missing" else 12 * padded) for kind, _, _, _ in jobs]
    _sync()
    for (kind, st, v0, v1), g in zip(jobs, bufs):
        if kind == "missing":
            w.ds.missing_per_sample_dev(v0, v1, g.ptr, st.cuda_stream)
        else:
            w.ds.sample_counts_dev(v0, v1, g.ptr, st.cuda_stream)
    _sync()
    for (kind, _, v0, v1), g in zip(jobs, bufs):
        g.check(missing_per_sample_ref(w.codes[v0:v1]) if kind == "missing" else sample_classes_ref(w.codes[v0:v1]))


@gpu
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_ten_live_streams_one_thread(gpu_lib, worlds, n):
    """pgh_missing_per_sample_dev round-robin over ten streams, twice around, from a thread whose scratch list starts
    empty: the ninth and tenth stream evict the oldest blocks (PghThreadScratch keeps eight), the second round finds
    some of its blocks gone.  Every stream stays alive until after the final synchronise."""
    w = worlds.dense(n)
    streams = [_stream() for _ in range(10)]
    assert len({st.cuda_stream for st in streams}) == 10
    span = w.m // 2
    jobs = [(streams[k % 10], k, k + span) for k in range(20)]
    bufs = [Guarded(4 * n) for _ in jobs]
    _sync()

    def work():
        for (st, v0, v1), g in zip(jobs, bufs):
            w.ds.missing_per_sample_dev(v0, v1, g.ptr, st.cuda_stream)

    _in_fresh_thread(work)
    _sync()
    for (_, v0, v1), g in zip(jobs, bufs):
        g.check(missing_per_sample_ref(w.codes[v0:v1]))
    del streams


@gpu
def test_scratch_growth_in_flight(gpu_lib, worlds):
    """On one stream of a fresh thread: pgh_missing_per_sample_dev on the 4,099-sample dataset, at once on the
    70,001-sample one (more scratch: the block is drained and grown while the first call may still be running), then
    on the small one again."""
    small, wide = worlds.dense(4099), worlds.dense(70001)
    st = _stream()
    jobs = [(small, 0, small.m), (wide, 0, wide.m), (small, 7, small.m - 9)]
    bufs = [Guarded(4 * w.n) for w, _, _ in jobs]
    _sync()

    def work():
        for (w, v0, v1), g in zip(jobs, bufs):
            w.ds.missing_per_sample_dev(v0, v1, g.ptr, st.cuda_stream)

    _in_fresh_thread(work)
    _sync()
    for (w, v0, v1), g in zip(jobs, bufs):
        g.check(missing_per_sample_ref(w.codes[v0:v1]))


@gpu
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_ld_task_buffers_regrow_between_launches(gpu_lib, worlds, n):
    """A short pair list on stream A, immediately a list more than 100 times longer on stream B -- more than the
    64 KiB the thread's task buffers start with (4,096 tasks of 16 bytes), so they are released and allocated anew
    after the first launch is waited for -- then the short list again.  A fresh thread, so that the buffers do start
    small.  All three results right, each in its own buffer; the status PGH_OK."""
    L = gpu_lib
    w = worlds.dense(n)
    mask, ss = w.subset(w.ds, "all_but_one")
    sa, sb = _stream(), _stream()
    a, b = SS.ld_pair_list(n)
    short = (_u32(a), _u32(b))
    rng = np.random.default_rng(n)
    long_a = rng.integers(0, w.m, 8000)
    long_b = (long_a + 2 + 2 * rng.integers(0, w.m // 2 - 2, 8000)) % w.m  # never the partner after the last one
    long = (_u32(long_a), _u32(long_b))
    assert len(long[0]) >= 100 * len(short[0]) and 16 * len(long[0]) > (64 << 10)
    jobs = [(short, sa, None), (long, sb, ss), (short, sa, ss)]
    bufs = [Guarded(24 * len(p[0])) for p, _, _ in jobs]
    _sync()

    def work():
        for ((pa, pb), st, sub), g in zip(jobs, bufs):
            w.ds.ld_pairs_dev(pa, pb, g.ptr, st.cuda_stream, subset=sub)
        L.ld_pairs_status()

    _in_fresh_thread(work)
    _sync()
    for ((pa, pb), _, sub), g in zip(jobs, bufs):
        g.check(ld_sums_ref(w.codes if sub is None else w.codes[:, mask], pa, pb))


@gpu
@pytest.mark.parametrize("n", PATTERN_WIDTHS)
def test_a_second_python_thread(gpu_lib, worlds, n):
    """The back-to-back pattern of pgh_ld_pairs_dev and pgh_missing_per_sample_dev on a second thread's own stream
    while the main thread does the same on its own: scratch blocks and LD task buffers are per thread.  The thread is
    joined with a time limit and every result is checked here, as test_thread_scratch_grows_and_is_reused does."""
    L = gpu_lib
    w = worlds.dense(n)
    span, ranges = _three_ranges(w.m)
    lists = _pair_lists(n)
    errors = []

    def plan():
        return {"st": _stream(), "ld": Guarded(24 * len(lists[0][0])), "miss": Guarded(4 * n)}

    def work(p):
        try:
            for (a, b), (v0, v1) in zip(lists, ranges):
                w.ds.ld_pairs_dev(a, b, p["ld"].ptr, p["st"].cuda_stream)
                w.ds.missing_per_sample_dev(v0, v1, p["miss"].ptr, p["st"].cuda_stream)
            L.ld_pairs_status()
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    mine, theirs = plan(), plan()
    _sync()
    t = threading.Thread(target=work, args=(theirs,))
    t.start()
    work(mine)
    t.join(timeout=120)
    assert not errors and not t.is_alive(), errors
    _sync()
    v0, v1 = ranges[2]
    for p in (mine, theirs):
        p["ld"].check(ld_sums_ref(w.codes, *lists[2]))
        p["miss"].check(missing_per_sample_ref(w.codes[v0:v1]))
