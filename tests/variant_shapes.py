"""Structured variant lists and windows: the placements, the list catalogue, the matrices and the NumPy references of
tests/test_variant_shapes.py.

Nothing here touches the GPU or the library.  A PLACEMENT is how a dataset holds the M_V rows of a matrix: all of them
(`whole`), the odd window [37, 318) (`window`, variant_begin is no multiple of 4 or 64) or two shards cut at 150
(`group`, the cut lies inside a 64-, a 96- and a 128-variant tile); the sparse-resident form has `sparse_whole` and
`sparse_window`, opened under PGH_SPARSE_WINDOW_BYTES of 97 rows.  shapes(b, e) names the variant lists at which a
translation (local = global - variant_begin), a tile tail or an order rule goes wrong, as GLOBAL indices over the
resident range [b, e).  Every reference is the operation itself in NumPy on codes[list] (want[list] for dosages), the
same for every placement: the yardsticks are subset_shapes' and the ones it borrows, never another call into the
library."""

import numpy as np

import subset_shapes as SS

N = SS.N_SMALL                # the only sample count: the variant axis is what is under test
M_V = 323                     # 5 * 64 + 3 = 2 * 128 + 67 = 3 * 96 + 35
WINDOW = (37, 318)            # 281 rows
CUT = 150                     # 2 * 64 + 22 = 96 + 54 = 128 + 22
SPARSE_WINDOW_ROWS = 97       # the sparse windows of an open end at 97, 194, 291
ROWS_ALL_MISSING, ROWS_MONO = (40, 300), (41, 301)  # resident in every placement
MADE_ROWS = (40, 41, 300, 301)
HET_ROWS = (107, 208)         # het-majority rows of the rare matrix inside the window (copies of its rows 7 and 8)
DENSE_PLACEMENTS = ("whole", "window", "group")
SPARSE_PLACEMENTS = ("sparse_whole", "sparse_window")
LIST_NAMES = ("range_all", "all_listed", "first", "last", "ends", "tile64", "tile64_plus", "tile64_minus", "tile96_plus",
              "tile128_plus", "stride3", "all_but_one", "made_only", "reversed", "shuffled", "repeated", "outside_low",
              "outside_high", "empty")
CONTIGUOUS = ("all_listed", "first", "last", "tile64", "tile64_plus", "tile64_minus", "tile96_plus", "tile128_plus")
UNORDERED = ("reversed", "shuffled", "repeated")  # what a strictly increasing list is not
OUTSIDE = ("outside_low", "outside_high")
DROPPED_LOCAL = 100           # all_but_one
REPEAT_AT = 10                # repeated: positions 10..15 of tile64_plus become [a, a, c, a, d, c]


def resident(placement):
    """[b, e): the global variants a placement holds."""
    return WINDOW if placement in ("window", "sparse_window") else (0, M_V)


def shapes(b, e):
    """name -> int64 global variant indices over the resident range [b, e), in LIST_NAMES order; range_all is None
    (the variant_begin / n_var form of the whole range) and outside_low exists only when b > 0."""
    every = np.arange(b, e, dtype=np.int64)

    def run(first, count):
        return np.arange(b + first, b + first + count, dtype=np.int64)

    stride3 = every[::3]
    plus = run(61, 65)
    repeated = plus.copy()
    a, c, d = plus[REPEAT_AT], plus[REPEAT_AT + 2], plus[REPEAT_AT + 4]
    repeated[REPEAT_AT:REPEAT_AT + 6] = [a, a, c, a, d, c]
    out = {
        "range_all": None,
        "all_listed": every,
        "first": every[:1],
        "last": every[-1:],
        "ends": every[[0, -1]],
        "tile64": run(64, 64),
        "tile64_plus": plus,
        "tile64_minus": run(3, 63),
        "tile96_plus": run(2, 97),
        "tile128_plus": run(5, 129),
        "stride3": stride3,
        "all_but_one": every[every != b + DROPPED_LOCAL],
        "made_only": np.array([r for r in MADE_ROWS if b <= r < e], dtype=np.int64),
        "reversed": every[::-1].copy(),
        "shuffled": stride3[np.random.default_rng(M_V).permutation(len(stride3))],
        "repeated": repeated,
    }
    if b > 0:
        out["outside_low"] = np.array([b - 1], dtype=np.int64)
    out["outside_high"] = np.array([e], dtype=np.int64)
    out["empty"] = np.zeros(0, dtype=np.int64)
    return {name: out[name] for name in LIST_NAMES if name in out}


def as_range(name, b, e):
    """(v_begin, v_end) of a list that a range can name, else None: the contiguous lists, range_all, empty (a
    zero-length range inside the resident one) and the outside ranges of one variant."""
    lst = shapes(b, e).get(name, ())
    if name == "range_all":
        return b, e
    if name == "empty":
        return b + 5, b + 5
    if name in CONTIGUOUS or name in OUTSIDE:
        return int(lst[0]), int(lst[-1]) + 1
    return None


def cases(placements):
    """Every (placement, list name): the pytest ids of the GPU tests."""
    return [(p, name) for p in placements for name in shapes(*resident(p))]


# ---- the matrices ------------------------------------------------------------------------------------------------

def _interleave():
    """Row k of hard_codes() <- row order[k] of subset_shapes.hard_codes(N, m=M_V): its 90 LD rows at the even rows
    below 180 (neighbours in the chain are two rows apart), population rows everywhere else, so that every list of
    63 variants holds both kinds and a PCA of it has two separated components."""
    order = np.arange(M_V)
    order[0:180:2] = np.arange(90)
    order[1:180:2] = np.arange(90, 180)
    return order


def hard_codes():
    """(M_V, N) hardcall codes from subset_shapes.hard_codes' generators, rows interleaved (see _interleave), with the
    made rows of this catalogue: all missing at 40 and 300, monomorphic at 41 and 301."""
    codes = SS.hard_codes(N, m=M_V)[_interleave()]
    codes[list(ROWS_ALL_MISSING)] = 3
    codes[list(ROWS_MONO)] = 0
    return codes


def rare_codes():
    """(codes, y): subset_shapes.rare_codes(N, m=M_V) with this catalogue's made rows and, inside the window, copies
    of its two het-majority rows."""
    codes, y = SS.rare_codes(N, m=M_V)
    codes = codes.copy()
    codes[HET_ROWS[0]], codes[HET_ROWS[1]] = codes[7], codes[8]
    codes[list(ROWS_ALL_MISSING)] = 3
    codes[list(ROWS_MONO)] = 0
    return codes, y


# ---- references on codes[list] -----------------------------------------------------------------------------------

G_OF = np.array([0, 1, 2, 0], dtype=np.int64)


def ld_pair_lists(lst):
    """(a, b): the pairs made from a list -- every two neighbours, (first, last), (last, first) and a variant with
    itself -- as global indices; empty for the empty list."""
    lst = np.asarray(lst, dtype=np.int64)
    if len(lst) == 0:
        return lst, lst
    mid = lst[len(lst) // 2]
    return (np.concatenate([lst[:-1], [lst[0], lst[-1], mid]]), np.concatenate([lst[1:], [lst[-1], lst[0], mid]]))


def ld_pairs_ref(codes, a, b):
    """uint32[n_pairs][6] = {n, sum_a, sum_b, sum_ab, sum_a2, sum_b2} of the pairs (a[p], b[p]) of rows of codes."""
    ca, cb = codes[np.asarray(a, dtype=np.int64)], codes[np.asarray(b, dtype=np.int64)]
    both = (ca != 3) & (cb != 3)
    ga, gb = G_OF[ca] * both, G_OF[cb] * both
    return np.stack([both.sum(axis=1), ga.sum(axis=1), gb.sum(axis=1), (ga * gb).sum(axis=1), (ga * ga).sum(axis=1),
                     (gb * gb).sum(axis=1)], axis=1).astype(np.uint32).reshape(len(ca), 6)


def king_table_ref(counts):
    """The pairs i < j of test_king.brute_counts' planes with test_king.py_kinship's formula, vectorised: (i, j, nsnp,
    hethet, ibs0, het1hom2, het2hom1, kinship).  The integers are far below 2^53, so the float64 quotient is the
    correctly rounded int / int."""
    i, j = np.triu_indices(counts.shape[1], k=1)
    nsnp, hethet, ibs0, h1, h2 = (counts[p][i, j].astype(np.int64) for p in range(5))
    den = 4 * (hethet + np.minimum(h1, h2))
    with np.errstate(all="ignore"):
        kin = 0.5 - (4 * ibs0 + h1 + h2).astype(np.float64) / den.astype(np.float64)
    kin[den == 0] = np.nan
    return i, j, nsnp, hethet, ibs0, h1, h2, kin


def supplied_freq(n_var):
    """One frequency per variant of a pgh_grm call: most usable, one each that the rule skips (0, 1, NaN)."""
    f = np.random.default_rng(500 + n_var).uniform(0.05, 0.95, n_var)
    for k, bad in zip((1, 5, 9), (0.0, 1.0, np.nan)):
        if k < n_var:
            f[k] = bad
    return f


def score_inputs(n_scored, ncols):
    """(weights, flip) for a list of n_scored variants; with more than one column the last is the unit column, which
    comes out as the dosage sum."""
    rng = np.random.default_rng(17 * ncols + n_scored)
    w = rng.standard_normal((n_scored, ncols))
    if ncols > 1:
        w[:, ncols - 1] = 1.0
    return w, (rng.random(n_scored) < 0.3).astype(np.uint8)


def phenotypes():
    """(z, y_lin, y_bin) over the N samples for the dense GLMs: two covariates, three phenotypes each."""
    z = SS.covariates(N)
    return z, SS.linear_phenotypes(N, z), SS.binary_phenotypes(N, z)


def set_weights(n_memb):
    """One weight per membership, one in five negative (test_burden_sparse._weights' shape)."""
    rng = np.random.default_rng(900 + n_memb)
    return rng.uniform(0.25, 25.0, n_memb) * np.where(rng.random(n_memb) < 0.2, -1.0, 1.0)
