"""Structured sample subsets: the mask catalogue, the matrices and the NumPy references of tests/test_subset_shapes.py.

Nothing here touches the GPU or the library.  shapes(N) names the masks at which gather, compaction and tiled kernels
go wrong -- whole include words of zeros or ones, kept sets that live in the ragged last word, n_out at and next to an
output tile, one or two samples, empty 8192-sample tiles, nobody -- and every reference is the operation itself in
NumPy on the physically subsetted matrix (codes[:, mask], y[mask], Z[:, mask]), never another call into the library.
The heavier yardsticks are the ones the suite already has (tests/test_king.py, test_grm.py, test_ld_prune.py,
test_ld_scores.py, test_score_sparse.py, test_burden_sparse.py and the glm oracles); they are imported where they are
used, so that the catalogue and its CPU test need nothing but numpy."""

import numpy as np

import pgen_writer as W

N_SMALL, N_WIDE = 1003, 16451  # 250 bytes + 3 samples, 15 words + 43 | 257 words + 3, a row pitch above 4 KiB
SAMPLE_COUNTS = (N_SMALL, N_WIDE)
M = 130                        # more than kLdTileA = 96 and kLdTileB = 128 variants
PAIR_TILE = 128                # kKingTile = kGrmTile
SPARSE_TILE = 8192             # kSparseTile: the LDS-privatised sample tiles of sparse.hip and score_sparse.hip
# the made rows of hard_codes(); 3 and 4 are where test_ld_pair_sums_match_oracle's pair list expects them
ROW_ALL_MISSING, ROW_MONO, ROW_BLOCK = 3, 4, 5
SHAPE_NAMES = ("all", "first", "last", "ends", "all_but_one", "last_word", "word_block", "tile_plus_one",
               "tile_minus_one", "stride64", "stride4", "tile_edges", "third_tile", "empty")


def shapes(n):
    """name -> bool[n], in SHAPE_NAMES order; the wide-only masks need more than two sparse tiles."""
    s = np.arange(n)
    out = {
        "all": np.ones(n, dtype=bool),
        "first": s == 0,
        "last": s == n - 1,
        "ends": (s == 0) | (s == n - 1),
        "all_but_one": s != 64 * (n // 128) + 31,  # mid-word
        "last_word": s >= 64 * (n // 64),
        "word_block": (s >= 64) & (s < 192),
        "tile_plus_one": (s >= 61) & (s < 190),
        "tile_minus_one": (s >= 3) & (s < 130),
        "stride64": s % 64 == 63,
        "stride4": s % 4 == 3,
    }
    if n > 2 * SPARSE_TILE:
        out["tile_edges"] = np.isin(s, [SPARSE_TILE - 1, SPARSE_TILE, 2 * SPARSE_TILE - 1, 2 * SPARSE_TILE, n - 1])
        out["third_tile"] = s >= 2 * SPARSE_TILE
    out["empty"] = np.zeros(n, dtype=bool)
    return {name: out[name] for name in SHAPE_NAMES if name in out}


def cases():
    """Every (N, shape name) of the matrix, the pytest ids of the GPU tests."""
    return [(n, name) for n in SAMPLE_COUNTS for name in shapes(n)]


def include_words(mask):
    """The uint64 words pgh_subset_create takes: bit s of word s // 64 = sample s kept."""
    words = np.zeros((len(mask) + 63) // 64, dtype=np.uint64)
    bits = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    words.view(np.uint8)[:len(bits)] = bits
    return words


def word_classes(mask):
    """(zero, full): the indices of the include words that keep nobody / every sample they cover."""
    n = len(mask)
    pad = np.zeros((n + 63) // 64 * 64, dtype=bool)
    pad[:n] = mask
    valid = np.zeros(len(pad), dtype=bool)
    valid[:n] = True
    kept, have = pad.reshape(-1, 64).sum(axis=1), valid.reshape(-1, 64).sum(axis=1)
    return np.flatnonzero(kept == 0).tolist(), np.flatnonzero(kept == have).tolist()


def empty_tiles(mask, tile=SPARSE_TILE):
    """The sample tiles of `tile` samples without a kept sample."""
    n = len(mask)
    return [t for t in range((n + tile - 1) // tile) if not mask[t * tile:(t + 1) * tile].any()]


# ---- the matrices ------------------------------------------------------------------------------------------------

def hard_codes(n, seed=None, m=M):
    """(m, n) hardcall codes (3 = missing), about 8 % missing: variants 0..89 carry LD (two haplotypes per sample whose
    latent uniforms are redrawn with probability 0.1 per variant, as tests/test_ld_prune.py's ld_codes), variants 90..
    follow three populations drawn per sample (so every mask of 127 samples and more holds all three, and a PCA of it
    has two separated leading components).  Row 3 is all missing, row 4 monomorphic, and row 5's only non-reference
    calls sit in samples that the word_block mask [64, 192) drops."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    codes = np.zeros((m, n), dtype=np.uint8)
    p = rng.uniform(0.05, 0.5, m)
    u = rng.random(2 * n)
    for k in range(90):
        redraw = rng.random(2 * n) < 0.1
        u = np.where(redraw, rng.random(2 * n), u)
        allele = (u < p[k]).astype(np.uint8)
        codes[k] = allele[:n] + allele[n:]
    pop = rng.integers(0, 3, n)
    levels = np.array([0.08, 0.5, 0.92])
    for k in range(90, m):
        freq = levels[rng.permutation(3)] if k % 2 else np.array([0.1, 0.1, 0.9])[rng.permutation(3)]
        codes[k] = rng.binomial(2, freq[pop])
    codes[rng.random((m, n)) < 0.08] = 3
    codes[ROW_ALL_MISSING] = 3
    codes[ROW_MONO] = 0
    outside = np.ones(n, dtype=bool)
    outside[64:192] = False
    codes[ROW_BLOCK] = 0
    hit = outside & (rng.random(n) < 0.3)
    codes[ROW_BLOCK, hit] = rng.integers(1, 3, int(hit.sum()), dtype=np.uint8)
    return codes


def rare_codes(n, seed=None, m=M):
    """(codes, y): m pgen_writer.rare_matrix rows (every majority code, 0..many entries) with the two het-majority rows
    of the sparse tests, a 0/1 phenotype over the raw samples, and every fourth hom-ref-majority variant enriched for
    ALT calls among its cases (tests/glm_spa_oracle.py), so that score tests beyond the saddlepoint cutoff exist."""
    import glm_spa_oracle as S

    rng = np.random.default_rng(2000 + n if seed is None else seed)
    codes = W.rare_matrix(m, n, rng)
    for v, rate in zip((7, 8), (0.01, 0.3)):
        hit = rng.random(n) < rate
        codes[v] = 1
        codes[v, hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
    y = (rng.random(n) < 0.2).astype(np.float64)
    return S.enriched_matrix(codes, y, rng, 5.0), y


def calls(codes):
    """int8 calls, -9 = missing (pgh_unpack_range's missing_code -9)."""
    return np.where(codes == 3, -9, codes).astype(np.int8)


def values(codes):
    """float64 values, -9.0 = missing: what the glm oracles take."""
    return np.where(codes == 3, -9.0, codes.astype(np.float64))


# ---- integer references ------------------------------------------------------------------------------------------

def counts_ref(codes):
    """uint32[V][4] = {hom_ref, het, hom_alt, missing} per variant."""
    return np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)


def sample_counts_ref(codes):
    """uint32[n][4] = {hom_ref, het, hom_alt, missing} per sample."""
    return np.stack([(codes == c).sum(axis=0) for c in range(4)], axis=1).astype(np.uint32)


def validity_ref(codes):
    """uint64[V][ceil(n / 64)]: bit k set = sample k called, zero padding."""
    v, n = codes.shape
    words = np.zeros((v, (n + 63) // 64), dtype=np.uint64)
    if n and v:
        bits = np.packbits(codes != 3, axis=1, bitorder="little")
        words.view(np.uint8).reshape(v, -1)[:, :bits.shape[1]] = bits
    return words


def packed_2bit_ref(row):
    """uint64[ceil(n / 32)]: the codes of one variant, 2 bits a sample (pgh_get_2bit)."""
    n = len(row)
    pad = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    pad[:n] = row
    shifts = (2 * np.arange(32, dtype=np.uint64))[None, :]
    return (pad.reshape(-1, 32) << shifts).sum(axis=1, dtype=np.uint64)


def bits_ref(flags):
    """uint64[ceil(n / 64)]: one bit per sample."""
    words = np.zeros((len(flags) + 63) // 64, dtype=np.uint64)
    if len(flags):
        bits = np.packbits(np.asarray(flags, dtype=bool), bitorder="little")
        words.view(np.uint8)[:len(bits)] = bits
    return words


def dosage_moments_ref(want_rows):
    """uint64[V][3] = {sum, sum of squares, observed} of the dosages in 1/16384 units (test_dosage_tracks._moments)."""
    out = np.zeros((len(want_rows), 3), dtype=np.uint64)
    for i, d in enumerate(want_rows):
        u = np.rint(d[d != -9.0] * 16384.0).astype(np.uint64)
        out[i] = (u.sum(), (u * u).sum(), len(u))
    return out


def ld_pair_list(n, m=40):
    """The pair list of test_gpu_parity.test_ld_pair_sums_match_oracle: anchors with 1..9 consecutive partners, then
    a variant with itself, a reversed pair, the far corner and the all-missing with the monomorphic row."""
    rng = np.random.default_rng(n)
    a, b = [], []
    for anchor in range(0, 30, 3):
        span = int(rng.integers(1, 10))
        for j in range(anchor + 1, min(m, anchor + 1 + span)):
            a.append(anchor)
            b.append(j)
    return a + [7, 9, 9, 39, 3], b + [7, 2, 9, 0, 4]


def ld_planes(codes):
    """test_ld_prune.brute_sums of every pair of (V, n) codes -- (6, V, V) int64: n, sum_a, sum_b, sum_ab, sum_a2,
    sum_b2 -- with the products taken in float64 (BLAS; exact, every sum is far below 2^53, as test_king.brute_counts
    does): the int64 products cost seconds at 16,451 samples."""
    c = (codes != 3).astype(np.float64)
    g = np.array([0.0, 1.0, 2.0, 0.0])[codes]
    q = np.array([0.0, 1.0, 4.0, 0.0])[codes]
    return np.stack([c @ c.T, g @ c.T, c @ g.T, g @ g.T, q @ c.T, c @ q.T]).astype(np.int64)


def ld_prune_ref(planes, codes, win_end, t, near):
    """test_ld_prune.brute_prune from planes that are already there: the header's formula and its sequential loop."""
    from test_ld_prune import maf_keys, prune_loop, r2_matrix

    r2 = r2_matrix(planes)
    band = np.zeros_like(r2, dtype=bool)
    for k in range(len(win_end)):
        band[k, k + 1:int(win_end[k])] = True
    assert not (np.abs(r2[band & ~np.isnan(r2)] - t) <= near).any(), "a band pair sits on the threshold: reseed"
    with np.errstate(invalid="ignore"):
        exc = r2 > t  # NaN: never
    mc, obs = maf_keys(codes)
    return prune_loop(exc, win_end, mc, obs)


def ld_scores_ref(planes, codes, win_end, unbiased):
    """test_ld_scores.brute_scores from planes that are already there: (fsum score, bound, n_partners) per variant."""
    import math

    from test_ld_scores import band_mask, self_terms, term_matrix

    ok, term = term_matrix(planes, unbiased)
    use = band_mask(win_end) & ok
    use = use | use.T  # a band pair counts for both of its variants
    selfs = self_terms(codes, unbiased)
    v = len(codes)
    score, bound = np.zeros(v), np.zeros(v)
    for k in range(v):
        terms = [selfs[k]] + term[k, use[k] & (np.arange(v) > k)].tolist() + term[use[:, k] & (np.arange(v) < k), k].tolist()
        score[k] = math.fsum(terms)
        bound[k] = len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)
    return score, bound, use.sum(axis=1).astype(np.uint32)


class MatrixPgen:
    """What oracle.score() reads of a Pgen, served from a value matrix that is already subsetted."""

    def __init__(self, vals):
        self.vals = vals
        self.N = vals.shape[1]

    def dosage(self, v, include=None):
        assert include is None
        return self.vals[v]


def freq_norm(counts):
    """(keep, center, inv_stdev) of plink_pca from counts: the variants with 0 < ALT_FREQ < 1 and their 2 p and
    1 / sqrt(2 p (1 - p)) (oracle.variant_norm)."""
    c = counts.astype(np.float64)
    obs = c[:, 0] + c[:, 1] + c[:, 2]
    af = np.where(obs > 0, (c[:, 1] + 2 * c[:, 2]) / np.maximum(2 * obs, 1), 0.0)
    keep = np.flatnonzero((obs > 0) & (af > 0) & (af < 1))
    return keep, 2 * af[keep], 1.0 / np.sqrt(2 * af[keep] * (1 - af[keep]))


def pca_ref(codes, n_pcs, g1):
    """plink_pca on (V, n) codes, the arithmetic of oracle.pca (src/plink_pca.cpp:392-416, 630-724) on a matrix:
    returns (eigenvalues, eigenvectors, keep, the whole spectrum found).  g1: the (n, 2 n_pcs) start the device call
    gets too."""
    keep, center, inv = freq_norm(counts_ref(codes))
    g = codes[keep].astype(np.float64)
    x = np.where(codes[keep] == 3, 0.0, (g - center[:, None]) * inv[:, None])
    m, k2 = len(keep), 2 * n_pcs
    qq = np.zeros((m, (n_pcs + 1) * k2))
    g1 = g1.copy()
    for p in range(n_pcs + 1):
        y = x @ g1
        qq[:, p * k2:(p + 1) * k2] = y
        if p < n_pcs:
            g1 = (x.T @ y) / m
    u, _, _ = np.linalg.svd(qq, full_matrices=False)
    u2, s, _ = np.linalg.svd(x.T @ u, full_matrices=False)
    return (s[:n_pcs] ** 2) / m, u2[:, :n_pcs], keep, (s ** 2) / m


# ---- phenotypes and covariates over the raw samples ---------------------------------------------------------------

def covariates(n, k=2, seed=5):
    """k covariates on different scales."""
    rng = np.random.default_rng(seed + n)
    return rng.normal(size=(k, n)) * (10.0 ** (np.arange(k) % 3 - 1.0))[:, None]


def nan_samples(n):
    """The samples without a phenotype: a few at random, and one of tile_edges' five, so that no mask of five samples
    or fewer has more observations than a fit with two covariates has parameters (intercept, genotype, 2)."""
    rng = np.random.default_rng(77 + n)
    gone = rng.random(n) < 0.03
    gone[:2] = False
    gone[n - 1] = False
    if n > 2 * SPARSE_TILE:
        gone[2 * SPARSE_TILE] = True
    return gone


def linear_phenotypes(n, z, count=3):
    """count quantitative phenotypes: the first two share nan_samples(n), the last has gaps of its own."""
    rng = np.random.default_rng(91 + n)
    y = 0.3 * z.sum(axis=0)[None, :] / np.maximum(np.abs(z).max(), 1.0) + rng.normal(size=(count, n))
    y[:, nan_samples(n)] = np.nan
    y[count - 1, rng.random(n) < 0.02] = np.nan
    return y


def binary_phenotypes(n, z, count=3, rate=0.35):
    rng = np.random.default_rng(92 + n)
    y = (rng.random((count, n)) < rate).astype(np.float64)
    y[:, nan_samples(n)] = np.nan
    y[count - 1, rng.random(n) < 0.02] = np.nan
    return y
