"""Structured carrier rows: the row catalogue, the phenotypes and the variant sets of tests/test_carrier_shapes.py.

Nothing here touches the GPU or the library.  rows(n) names the carrier rows at which a walk of a row's entries goes
wrong: entry counts at and next to the steps of a wave (64) and of a workgroup (256), at and next to the team split
kGlmSparseLong = 1024 and its multiples (the segments of the multi kernels), at the levels of the 64-way search (64,
4096); each count once at the start of the first sample tile, at the start of the second, in the last samples of the
row (the ragged last tile) and spread over the row; every base code at the split; entries on the samples next to every
tile boundary; runs of exactly 64 and 128 entries that end with a tile; rows whose list set (the missing entries, or
for a missing-majority row the called ones) is everything or nothing; and rows whose entries lose their phenotype.

A row is one base code and its designed entries, and the entry codes cycle through the codes other than the base in
entry order, so that a row of three entries and more holds all of them unless its name says otherwise.  The names are
the contract: test_carrier_shapes.py derives what a row must hold from its name alone.

The phenotypes, covariates and yardsticks are subset_shapes' and the families' own; the catalogue and its CPU test
need nothing but numpy."""

import os
import re

import numpy as np

import subset_shapes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plinking_duck_amd", "csrc")


def header_constant(header, name):
    """`constexpr uint32_t name = value;` of a header under csrc/."""
    text = open(os.path.join(CSRC, header)).read()
    found = re.findall(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(found) == 1, (header, name, found)
    return int(found[0])


# the structural constants of the sparse walk: the catalogue's edges are these, so a changed constant fails the import
# of the catalogue instead of silently leaving the rows beside the edges
LONG = header_constant("glm.hpp", "kGlmSparseLong")
SPARSE_TILE = header_constant("sparse.hpp", "kSparseTile")
SCORE_ACC_BYTES = header_constant("sparse.hpp", "kScoreSparseAccBytes")
SCORE_CHUNK = header_constant("sparse.hpp", "kScoreSparseChunk")
assert (LONG, SPARSE_TILE, SCORE_ACC_BYTES, SCORE_CHUNK) == (1024, 8192, 131072, 8), "the catalogue's design values"
assert SPARSE_TILE == SS.SPARSE_TILE

WAVE, BLOCK = 64, 256          # entries a wave form and a workgroup form take per step
PHENO_BLOCK = 64               # kGlmScoreSparsePb = kGlmSparseMultiPb: the phenotypes of one walk

N_WIDE = SS.N_WIDE             # 16,451: three sparse tiles, the last of 67 samples; a row pitch above 4 KiB
N_TILE = SPARSE_TILE           # one full tile and a full last word
SAMPLE_COUNTS = (N_TILE, N_WIDE)

ENTRY_COUNTS = (1, 63, 64, 65, 128, 255, 256, 257, 1023, 1024, 1025, 1280, 1281, 2048, 2049, 4096, 4097)
PLACEMENTS = ("tile0", "tile1", "last", "spread")
BASE_COUNTS = (0, 1, 64, 1024, 1025)
NOCALL_ENTRIES = 1500
ALLMISS_ENTRIES = 100
HELD, HELD_UNUSED = LONG + 76, 76  # long_held_short_used: 1,100 entries held, 1,024 of them with a phenotype


def score_tile(n_acc):
    """ScoreSparseTile(n_acc) of sparse.hpp."""
    return SCORE_ACC_BYTES // (8 * n_acc + 4) // 64 * 64


def score_tiles():
    """Every tile k_score_sparse takes: 1 .. kScoreSparseChunk weight columns, with and without the dosage sum."""
    return sorted({score_tile(a) for a in range(1, SCORE_CHUNK + 2)})


def nan_samples(n):
    """The samples without a phenotype in the single-phenotype calls (subset_shapes.nan_samples)."""
    return SS.nan_samples(n)


def _spread(n, e):
    return (np.arange(e, dtype=np.int64) * n) // max(e, 1)


def _row(n, base, samples, codes=None):
    """A row of `base` with entries at `samples` (ascending); codes None: the codes other than base, cycling."""
    samples = np.asarray(samples, dtype=np.int64)
    assert len(samples) == 0 or (np.all(np.diff(samples) > 0) and samples[0] >= 0 and samples[-1] < n)
    if codes is None:
        codes = [c for c in range(4) if c != base]
    row = np.full(n, base, dtype=np.uint8)
    row[samples] = np.asarray(codes, dtype=np.uint8)[np.arange(len(samples)) % len(codes)]
    return row


def placement(n, e, where):
    """The entry samples of E{e}_{where}, or None when they do not fit in n samples."""
    if where == "tile0":
        s = np.arange(e)
    elif where == "tile1":
        s = SPARSE_TILE + np.arange(e)
    elif where == "last":
        s = n - e + np.arange(e)
    else:
        s = _spread(n, e)
    return s if e <= n and len(s) and s[-1] < n and s[0] >= 0 else None


def edge_samples(n):
    """The first and last sample of every sparse tile of n samples: {0, 8191, 8192, 16383, 16384, n - 1} at N_WIDE."""
    s = {0, n - 1}
    for t in range(SPARSE_TILE, n, SPARSE_TILE):
        s |= {t - 1, t}
    return sorted(s)


def rows(n):
    """name -> uint8[n] codes (3 = missing), in catalogue order; at N_TILE only the rows that fit."""
    out = {}
    for e in ENTRY_COUNTS:
        for where in PLACEMENTS:
            s = placement(n, e, where)
            if s is not None:
                out[f"E{e}_{where}"] = _row(n, 0, s)
    for base in (1, 2, 3):
        for e in BASE_COUNTS:
            out[f"b{base}_E{e}"] = _row(n, base, _spread(n, e))
    out["edges"] = _row(n, 0, edge_samples(n))
    at = np.arange(n)
    out["stride64"] = _row(n, 0, at[(at % 64 == 0) | (at % 64 == 63)])
    if n > SPARSE_TILE + 3:
        for run in (64, 128):  # a whole number of wave steps ends with tile 0; the row goes on in tile 1
            out[f"run{run}_then_next"] = _row(n, 0, np.arange(SPARSE_TILE - run, SPARSE_TILE + 3))
    out["allmiss_entries"] = _row(n, 0, _spread(n, ALLMISS_ENTRIES), codes=[3])
    out["nocall_missing"] = _row(n, 0, _spread(n, NOCALL_ENTRIES), codes=[1, 2])
    gone = np.flatnonzero(nan_samples(n))
    have = np.flatnonzero(~nan_samples(n))
    assert len(gone) >= HELD_UNUSED
    out["carriers_without_phenotype"] = _row(n, 0, gone)
    # more than kGlmSparseLong entries held, exactly kGlmSparseLong of them used: the team split follows the held ones
    used = have[(np.arange(LONG, dtype=np.int64) * len(have)) // LONG]
    out["long_held_short_used"] = _row(n, 0, np.sort(np.concatenate([used, gone[:HELD_UNUSED]])))
    return out


def matrix(n):
    """(names, codes): the catalogue as a matrix, one variant per designed row."""
    cat = rows(n)
    return list(cat), np.stack(list(cat.values()))


def entry_samples(row):
    """(base code, the samples that differ from it): the majority code, ties to the lower one."""
    base = int(np.bincount(row, minlength=4).argmax())
    return base, np.flatnonzero(row != base)


# ---- phenotypes and covariates over the raw samples ---------------------------------------------------------------

def covariates(n, k=2):
    """k = 2: SS.covariates(n, seed=9), the sparse families' covariates in test_subset_shapes; k = 0: none."""
    return SS.covariates(n, k=2, seed=9) if k else np.zeros((0, n))


def linear_phenotype(n):
    return SS.linear_phenotypes(n, covariates(n))[0]


def binary_phenotype(n):
    return SS.binary_phenotypes(n, covariates(n))[0]


# the phenotypes of a block: their NaN patterns differ; two are aimed at designed rows
PHENO_PLAIN, PHENO_ROW_GONE, PHENO_PAST_LONG, PHENO_COMPLETE, PHENO_OWN_GAPS = range(5)
ROW_GONE = "E257_spread"        # PHENO_ROW_GONE has no value at any of its entries
ROW_PAST_LONG = "E1025_tile0"   # PHENO_PAST_LONG has a value at its first 1,024 entries and none at the one past them
BLOCK_COUNTS = (3, 5, PHENO_BLOCK + 3)  # not a power of two; every distinct phenotype; two phenotype blocks


def distinct_phenotypes(n, binary):
    """The five distinct phenotypes (5 x n): PLAIN is the single-phenotype calls' own, ROW_GONE loses the entries of
    its row on top of nan_samples(n), PAST_LONG has a value at the first kGlmSparseLong entries of its row and none at
    the rest of them, COMPLETE has a value everywhere, OWN_GAPS has gaps of its own."""
    z = covariates(n)
    y = (SS.binary_phenotypes(n, z, count=5) if binary else SS.linear_phenotypes(n, z, count=5)).copy()
    cat = rows(n)
    rng = np.random.default_rng(93 + n)
    fill = (rng.random(n) < 0.35).astype(np.float64) if binary else rng.normal(size=n)
    y[PHENO_ROW_GONE, entry_samples(cat[ROW_GONE])[1]] = np.nan
    past = entry_samples(cat[ROW_PAST_LONG])[1]
    y[PHENO_PAST_LONG, past] = np.where(np.isnan(y[PHENO_PAST_LONG, past]), fill[past], y[PHENO_PAST_LONG, past])
    y[PHENO_PAST_LONG, past[LONG:]] = np.nan
    y[PHENO_COMPLETE] = np.where(np.isnan(y[PHENO_COMPLETE]), fill, y[PHENO_COMPLETE])
    return y


def phenotype_block(n, count, binary):
    """count x n: phenotype j of the block is distinct phenotype j % 5, so that the oracle's rows of five phenotypes
    serve a block of any size."""
    return np.ascontiguousarray(distinct_phenotypes(n, binary)[np.arange(count) % 5])


# ---- variant sets for the burden and SKAT tests -------------------------------------------------------------------

MIXED_BASES = ("E64_spread", "b1_E64", "b2_E64", "b3_E64")
TWICE = "E4097_spread"


def variant_sets(names):
    """(labels, sets): a singleton per designed row, every tile1 row, the four base codes together, a long row twice."""
    at = {name: i for i, name in enumerate(names)}
    labels = list(names)
    sets = [[at[name]] for name in names]
    tile1 = [at[name] for name in names if name.endswith("_tile1")]
    if tile1:
        labels.append("all_tile1")
        sets.append(tile1)
    labels += ["mixed_bases", "long_twice"]
    sets += [[at[name] for name in MIXED_BASES], [at[TWICE], at[TWICE]]]
    return labels, [np.array(s, dtype=np.uint32) for s in sets]
