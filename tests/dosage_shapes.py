"""Structured dosage tracks: the row catalogue of tests/test_dosage_shapes.py.

Nothing here touches the GPU or the library.  rows(n) names the tracks at which the dosage kernels go wrong.  A row is
a hardcall row (uint8[n], 3 = missing) and a dosage row (uint16[n], 0xFFFF = no explicit dosage, else 0..32768 = 0..2
ALT copies); the edges are those of dosage.hip and api_analysis.cpp:

  * entry counts at and next to the sixteen values k_score_dosage_fix preloads per 64-sample word, a wave (64), the
    difflist groups of the 0x20 list (64, 128), the 512 records k_score_dosage_records fetches at a time and their
    multiples, the 2/5 cut between the explicit-entry kernels and the sample-owning k_score_dosage, and a full track
    but for one sample -- each count at the start of tile 0, at the start of tile 1, in the last samples of the row
    and spread over the row;
  * words that are empty, hold one entry, sixteen, seventeen or all 64; a tile without an entry between two that have
    some; entries on both samples next to every word and tile boundary;
  * the values 0, 16384 and 32768, alone and meeting every hardcall code;
  * entries on missing calls only, on called samples only, a full track over an all-missing row, tracks that restate
    their calls (sparse, with gaps and full);
  * rows of 0, 7, 8 and 15 hets, whose phase track in front of the dosage track is 1, 8, 9 and 16 bits long.

The names are the contract: test_dosage_shapes.py derives what a row must hold from its name alone.  layout(n) is the
file: every row as three variants, one per track encoding (0x20 list, 0x40 dense, 0x60 bit array), with a track-less
variant of the same calls after the first of them, so that a track has track-less neighbours on both sides; the full
row E{n}_tile0_ref is last, so that a full track ends the value run."""

import zlib

import numpy as np

from carrier_shapes import header_constant

# the design values of the dosage kernels: the catalogue's edges are these, so a changed constant fails the import of
# the catalogue instead of silently leaving the rows beside the edges
WORD = header_constant("dosage.hpp", "kDosageWord")
PRELOAD = header_constant("dosage.hpp", "kDosagePreload")  # values of a word held in registers before the scalar tail
TILE = header_constant("dosage.hpp", "kDosageTile")
REC_FETCH = header_constant("dosage.hpp", "kDosageRecFetch")
ENTRY_STAGE = header_constant("dosage.hpp", "kDosageEntryStage")
LANE_STAGE = header_constant("dosage.hpp", "kDosageLaneStage")
CUT_NUM = header_constant("dosage.hpp", "kDosageCutNum")
CUT_DEN = header_constant("dosage.hpp", "kDosageCutDen")
assert (WORD, PRELOAD, TILE, REC_FETCH, ENTRY_STAGE, LANE_STAGE, CUT_NUM, CUT_DEN) == (64, 16, 4096, 512, 128, 64, 2, 5), \
    "the catalogue's design values"

NONE = 0xFFFF
N_TILE = TILE                 # one tile, 64 full words
N_WIDE = 2 * TILE + 67        # 8259: three tiles, the last tile's last word holds 3 samples
SAMPLE_COUNTS = (N_TILE, N_WIDE)
TINY_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65)   # the 4-samples-per-lane tail of the sample-owning kernels
ID_COUNTS = (255, 256)                      # 1- and 2-byte sample ids in the 0x20 list
N_IDS3 = 65537                              # 3-byte sample ids
ENCODINGS = (0x20, 0x40, 0x60)
HARD, SPARSE, GAPS, FULL = 0, 1, 2, 3       # the plan's classes (DosageTrackClass of dosage.hpp)
PLACEMENTS = ("tile0", "tile1", "last", "spread")
BACKGROUND_OF = {"tile0": "ref", "tile1": "common", "last": "ref", "spread": "common"}
PHASE_HETS = (0, 7, 8, 15)
VALUE_ENTRIES, NONE_ON_MISSING_ENTRIES, PHASE_ENTRIES, RESTATED_SPARSE_ENTRIES = 600, 500, 100, 300


def cut_counts(n):
    """(the last sparse count, the first count that goes to the sample-owning kernel)."""
    hi = -(-CUT_NUM * n // CUT_DEN)  # the least e with e * CUT_DEN >= CUT_NUM * n
    return hi - 1, hi


def entry_counts(n):
    lo, hi = cut_counts(n)
    return (0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513, 1023, 1024, 1025, lo, hi, n - 1, n)


def track_class(have, n):
    """DosageTrackClass of dosage.hpp for a row that has a track."""
    return FULL if have == n else GAPS if have * CUT_DEN >= n * CUT_NUM else SPARSE


def _rng(n, name):
    return np.random.default_rng([n, zlib.crc32(name.encode())])


def common(n, name="common"):
    """A common-variant hardcall row with about 3 % missing calls, seeded by the sample count and the name."""
    return _rng(n, name).choice(4, size=n, p=[0.55, 0.3, 0.12, 0.03]).astype(np.uint8)


def background(n, kind, name):
    if kind == "common":
        return common(n, name)
    return np.full(n, {"ref": 0, "het": 1, "missing": 3}[kind], dtype=np.uint8)


def _spread(n, e):
    return (np.arange(e, dtype=np.int64) * n) // max(e, 1)


def placement(n, e, where):
    """The entry samples of E{e}_{where}, or None when the placement does not fit or repeats another."""
    if e == 0 or e > n:
        return None
    if where == "tile0":
        return np.arange(e)
    if where == "tile1":
        return TILE + np.arange(e) if TILE + e <= n else None
    if where == "last":
        return n - e + np.arange(e) if e < n else None  # e == n is tile0
    return _spread(n, e) if 2 * e <= n else None


def _with(hard, samples, values):
    dos = np.full(len(hard), NONE, dtype=np.uint16)
    dos[np.asarray(samples, dtype=np.int64)] = values
    return hard, dos


def _uniform(n, name, count):
    return _rng(n, name + "/values").integers(0, 32769, count).astype(np.uint16)


def rows(n):
    """name -> (uint8[n] hardcalls, uint16[n] dosages), in catalogue order, for the two wide sample counts."""
    assert n in SAMPLE_COUNTS
    out = {}
    at = np.arange(n)
    words = (n + WORD - 1) // WORD
    in_word = np.minimum(WORD, n - WORD * np.arange(words))  # samples each word holds
    for bg in ("ref", "common", "missing"):
        name = f"E0_{bg}"
        out[name] = _with(background(n, bg, name), [], [])
    for e in entry_counts(n)[:-1]:
        for where in PLACEMENTS:
            s = placement(n, e, where)
            if s is not None:
                name = f"E{e}_{where}_{BACKGROUND_OF[where]}"
                out[name] = _with(background(n, BACKGROUND_OF[where], name), s, _uniform(n, name, e))
    name = "E64_spread_het"
    out[name] = _with(background(n, "het", name), _spread(n, 64), _uniform(n, name, 64))
    # ---- word fills
    name = "word64_only"
    out[name] = _with(background(n, "ref", name), 5 * WORD + np.arange(WORD), _uniform(n, name, WORD))
    name = "one_per_word"
    s = WORD * np.arange(words) + (7 * np.arange(words)) % in_word
    out[name] = _with(background(n, "ref", name), s, _uniform(n, name, words))
    for fill in (PRELOAD, PRELOAD + 1):
        name = f"word{fill}"
        w = np.arange(words)[in_word == WORD]
        bits = (w[:, None] + 4 * np.arange(PRELOAD)[None, :]) % WORD
        if fill > PRELOAD:
            bits = np.concatenate([bits, ((w + 1) % WORD)[:, None]], axis=1)
        s = np.sort((WORD * w[:, None] + bits).reshape(-1))
        out[name] = _with(background(n, "ref", name), s, _uniform(n, name, len(s)))
    if n > 2 * TILE:
        name = "tile_gap"
        s = np.concatenate([np.arange(0, TILE, 100), 2 * TILE + np.array([0, 5, n - 2 * TILE - 1])])
        out[name] = _with(background(n, "ref", name), s, _uniform(n, name, len(s)))
    name = "boundaries"
    s = at[(at % WORD == 0) | (at % WORD == WORD - 1) | (at == n - 1)]
    out[name] = _with(background(n, "common", name), s, _uniform(n, name, len(s)))
    # ---- values
    for value in (0, 16384, 32768):
        name = f"val{value}"
        out[name] = _with(background(n, "common", name), _spread(n, VALUE_ENTRIES), value)
    name = "val_cycle"
    hard = background(n, "common", name)
    dos = np.full(n, NONE, dtype=np.uint16)
    for code in range(4):
        s = np.flatnonzero(hard == code)[:6]
        dos[s] = np.array([0, 16384, 32768], dtype=np.uint16)[np.arange(6) % 3]
    out[name] = (hard, dos)
    # ---- missing calls
    name = "all_on_missing"
    hard = background(n, "common", name)
    s = np.flatnonzero(hard == 3)
    out[name] = _with(hard, s, _uniform(n, name, len(s)))
    name = "none_on_missing"
    hard = background(n, "common", name)
    called = np.flatnonzero(hard != 3)
    s = called[_spread(len(called), NONE_ON_MISSING_ENTRIES)]
    out[name] = _with(hard, s, _uniform(n, name, len(s)))
    name = "full_over_allmissing"
    out[name] = _with(background(n, "missing", name), at, _uniform(n, name, n))
    name = "restated_gaps"
    hard = background(n, "common", name)
    out[name] = (hard, np.where(hard == 3, NONE, hard.astype(np.uint16) << 14).astype(np.uint16))
    name = "restated_sparse"
    hard = background(n, "common", name)
    called = np.flatnonzero(hard != 3)
    s = called[_spread(len(called), RESTATED_SPARSE_ENTRIES)]
    out[name] = _with(hard, s, hard[s].astype(np.uint16) << 14)
    name = "restated_full"
    hard = background(n, "common", name)
    hard[hard == 3] = 0
    out[name] = (hard, (hard.astype(np.uint16) << 14).astype(np.uint16))
    # ---- phase tracks in front: 1 + hets bits
    for hets in PHASE_HETS:
        name = f"phase_het{hets}"
        hard = background(n, "common", name)
        hard[hard == 1] = 0
        hard[_spread(n, hets) + 3] = 1
        out[name] = _with(hard, _spread(n, PHASE_ENTRIES), _uniform(n, name, PHASE_ENTRIES))
    # ---- the full row last: its values end the value run
    name = f"E{n}_tile0_ref"
    out[name] = _with(background(n, "ref", name), at, _uniform(n, name, n))
    return out


def small_rows(n):
    """The catalogue of the tiny sample counts and of the 1- and 2-byte sample ids: every count that fits at the start
    and at the end of the row, over a common background."""
    out = {}
    for bg in ("common", "missing"):
        name = f"E0_{bg}"
        out[name] = _with(background(n, bg, name), [], [])
    for e in sorted({1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 128, 129, n // 2, n - 1} - {0}):
        for where in ("tile0", "last"):
            s = placement(n, e, where) if e < n else None  # the full row comes last
            if s is not None:
                name = f"E{e}_{where}_common"
                out[name] = _with(background(n, "common", name), s, _uniform(n, name, e))
    name = "full_over_allmissing"
    out[name] = _with(background(n, "missing", name), np.arange(n), _uniform(n, name, n))
    name = "restated_gaps"
    hard = background(n, "common", name)
    hard[0] = 3  # at least one sample without a dosage, whatever the draw
    out[name] = (hard, np.where(hard == 3, NONE, hard.astype(np.uint16) << 14).astype(np.uint16))
    name = f"E{n}_tile0_common"
    out[name] = _with(background(n, "common", name), np.arange(n), _uniform(n, name, n))
    return out


IDS3_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)


def ids3_rows(n=N_IDS3):
    """A dozen 0x20 rows whose sample ids take three bytes: the difflist group steps, spread and in the last samples."""
    out = {}
    for e in IDS3_COUNTS:
        name = f"E{e}_spread_common"
        out[name] = _with(background(n, "common", name), _spread(n, e), _uniform(n, name, e))
    for e in (64, 65, 129):
        name = f"E{e}_last_common"
        out[name] = _with(background(n, "common", name), n - e + np.arange(e), _uniform(n, name, e))
    return out


def catalogue(n):
    return rows(n) if n in SAMPLE_COUNTS else ids3_rows(n) if n == N_IDS3 else small_rows(n)


class Layout:
    """The file of one sample count: names[v], kinds[v] (0 = no track) and the (m, n) hardcall and dosage matrices."""

    def __init__(self, n):
        cat = catalogue(n)
        self.n = n
        self.row_names = list(cat)
        encodings = (0x20,) if n == N_IDS3 else ENCODINGS
        self.names, self.kinds, hard, dos = [], [], [], []
        for name, (h, d) in cat.items():
            for i, kind in enumerate(encodings):
                self.names.append(name)
                self.kinds.append(kind)
                hard.append(h)
                dos.append(d)
                if i == 0:  # the same calls without a track
                    self.names.append(name)
                    self.kinds.append(0)
                    hard.append(h)
                    dos.append(np.full(n, NONE, dtype=np.uint16))
        self.hard, self.dos = np.stack(hard), np.stack(dos)
        self.kinds = np.array(self.kinds)
        self.m = len(self.names)
        self.have = (self.dos != NONE).sum(axis=1)
        self.cls = np.array([track_class(int(e), n) if k else HARD for e, k in zip(self.have, self.kinds)])

    def variants(self, name, kind=None):
        return [v for v in range(self.m) if self.names[v] == name and (kind is None or self.kinds[v] == kind)]


def values(hard, dos):
    """The float64 value rows: the explicit dosage / 16384, else the call, -9.0 for neither."""
    return np.where(dos != NONE, dos.astype(np.float64) / 16384.0, np.where(hard == 3, -9.0, hard.astype(np.float64)))


def moments(x):
    """uint64[V][3] = {sum, sum of squares, observed} on the 16384-per-copy scale, in Python integers."""
    out = np.zeros((len(x), 3), dtype=np.uint64)
    for i, row in enumerate(x):
        u = [int(v) for v in np.rint(row[row != -9.0] * 16384.0)]
        out[i] = (sum(u), sum(v * v for v in u), len(u))
    return out


def word_fills(dos):
    """Entries per 64-sample word of one dosage row."""
    n = len(dos)
    pad = np.zeros((n + WORD - 1) // WORD * WORD, dtype=bool)
    pad[:n] = dos != NONE
    return pad.reshape(-1, WORD).sum(axis=1)


def tile_runs(dos):
    """Entries per 4096-sample tile of one dosage row: the (row, tile) runs of the entry records."""
    n = len(dos)
    return [int((dos[t:t + TILE] != NONE).sum()) for t in range(0, n, TILE)]


def record_order(dos, tile):
    """The samples of a tile's entries in the order of the entry records: round-major -- the first entry of every word
    of the tile (words ascending), then every word's second entry, and so on."""
    s = np.flatnonzero(dos[tile * TILE:(tile + 1) * TILE] != NONE)
    word = s // WORD
    rnd = np.arange(len(s)) - np.searchsorted(word, word)  # the entry's index within its word
    return tile * TILE + s[np.lexsort((word, rnd))]
