"""Structured hardcall records: the row catalogue of tests/test_record_shapes.py.

Nothing here touches the GPU or the library.  rows(n) names the records at which the device record decoder goes wrong
(k_decode_records of decode.hip, WalkDifflistIds of decode_device.hpp, k_phase_extract of phase.hip); the edges are:

  * difflist lengths at and next to the value section's byte (4 entries), a group (64 entries, 63 gaps), two groups,
    the 64 groups one trip of the group-first loop takes (4096 entries) and 65 whole groups (4160), plus len == N at
    the small sample counts -- each at the start of the row, ending on sample N-1 and spread over the row, under every
    difflist kind (4, 6, 7 and 1);
  * gap streams by design: every gap 1 (64 varints per 64-byte trip, so that trip t starts k_base % 63 == t % 63 into
    its group), every gap at a varint step (127 | 128, 16383 | 16384, 2^21 - 1 | 2^21), a 2-byte varint that starts
    at trip byte 63, a 3-byte varint at trip bytes 62 and 63, a trip that ends on a group's 63rd gap, and a run of 130
    consecutive samples that ends on sample N-1;
  * single entries on both sides of the 16- and 64-sample words, on sample N-1 and on every sample of the ragged last
    16-sample word;
  * type 1: every (low, high) pair, with an empty and a 65-entry difflist, and with the unused bits of the bit array
    set; type 0 with the unused bits of its last byte set;
  * LD runs off every base kind (0, 1, 4, 6, 7): types 2 and 3, empty and with 65 entries, and a type-3 record whose
    one entry restates the base's value;
  * phase tracks of exact content on rows stored as type 0 and as type 4: both forms at the byte steps of the 1 + hets
    header, hets filling one 64-sample word and split 1 | 63 over two, hets in the ragged last word only and beyond
    word 256 only, the explicit form with no, all, 8, 64 and 65 flags.

The names are the contract: test_record_shapes.py derives what a row must hold from its name alone.  A row is a tuple
(kind, codes[n], base row name or None, phase, pair, dirty, keep): phase is None or the exact track (explicit form?,
present bit per het, info bit per flagged het); pair, dirty and keep are the writer's options (pgen_writer.
encode_record)."""

import os
import re
import zlib
from typing import NamedTuple

import numpy as np

from carrier_shapes import CSRC


def source_constant(source, name):
    """`constexpr <integer type> name = value;` of a file under csrc/."""
    text = open(os.path.join(CSRC, source)).read()
    found = re.findall(r"constexpr\s+(?:int|uint32_t)\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(found) == 1, (source, name, found)
    return int(found[0])


# the design values of the decoder and of pgh_open's routes: the catalogue's edges are these, so a changed constant
# fails the import of the catalogue instead of silently leaving the rows beside the edges
DECODE_THREADS = source_constant("decode.hip", "kDecodeThreads")
MIN_PLAIN_RUN = source_constant("api_dataset.cpp", "kMinPlainRun")
assert (DECODE_THREADS, MIN_PLAIN_RUN) == (256, 256), "the catalogue's design values"

# the format's own steps
GROUP = 64                     # entries of a difflist group: one outright id and 63 gaps
GAPS = GROUP - 1               # (a trip of the device walk is 64 bytes of the gap stream: at most 64 gaps)
VARINT_STEPS = (1 << 7, 1 << 14, 1 << 21)
SCAN_WORDS = 256               # words one trip of phase.hip's block prefix sum takes

N_WIDE = 3 * (1 << 14) - 17    # 49,135: N % 4 = 3, N % 16 = 15, N % 64 = 47; 768 64-sample words
assert N_WIDE > 1 << 14 and N_WIDE % 4 == 3 and N_WIDE % 16 == 15
ID_COUNTS = (255, 256, 65535, 65536)   # sample-id bytes 1 | 2 and 2 | 3
N_GAP4 = (1 << 21) + 70        # 4-byte gap varints
N_ID4 = (1 << 24) + 17         # 4-byte sample ids
BIG_COUNTS = (N_GAP4, N_ID4)
SAMPLE_COUNTS = ID_COUNTS + (N_WIDE,)

DIFF_KINDS = (4, 6, 7, 1)
ENTRY_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4160)
PLACEMENTS = ("tile0", "last", "spread")
GAP_VALUES = tuple(g for step in VARINT_STEPS for g in (step - 1, step))
GAP_ROW_ENTRIES = 200          # entries of a d6_gap{g} row, where N holds that many
GAP1_COUNTS = (130, 4160)      # all gaps 1: trips start 0, 1 and, for 4160, up to 62 gaps into their group
RUN1_FIRST = 5                 # first sample of the d6_gap1 rows
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
D1_PAIR = (0, 2)               # the pair of the d1_E rows
BASE_KINDS = (0, 1, 4, 6, 7)
PHASE_HETS = (1, 7, 8, 15, 16, 63, 64, 65)
PHASE_FLAGS = (8, 64, 65)
PHASE_FLAG_HETS = 100          # hets of the ph_explicit_flag{f} rows
PHASE_STORES = (0, 4)
CONST_OF = {4: 0, 6: 2, 7: 3}
INV = np.array([2, 1, 0, 3], dtype=np.uint8)


class Row(NamedTuple):
    kind: int
    codes: np.ndarray
    base: str | None = None
    phase: tuple | None = None
    pair: tuple | None = None
    dirty: bool = False
    keep: np.ndarray | None = None

    def options(self):
        """encode_record's options of this row."""
        out = {}
        if self.pair is not None:
            out["pair"] = self.pair
        if self.dirty:
            out["dirty_tail"] = True
        if self.keep is not None:
            out["keep"] = self.keep
        return out


def _rng(n, name):
    return np.random.default_rng([n, zlib.crc32(name.encode())])


def common(n, name):
    """A dense row that holds every code, seeded by the sample count and the name."""
    return _rng(n, name).choice(4, size=n, p=[0.5, 0.3, 0.15, 0.05]).astype(np.uint8)


def spread(n, e):
    return (np.arange(e, dtype=np.int64) * n) // max(e, 1)


def placement(n, e, where):
    """The entry samples of E{e}_{where}, or None when the placement does not fit or repeats another."""
    if e > n:
        return None
    if where == "tile0":
        return np.arange(e, dtype=np.int64)
    if e == 0 or e == n:
        return None  # tile0 is that row
    if where == "last":
        return n - e + np.arange(e, dtype=np.int64)
    return spread(n, e) if 2 * e <= n else None


def others(kind):
    """The codes a difflist entry of this kind can hold, in the order the entries cycle through them."""
    base = D1_PAIR if kind == 1 else (CONST_OF[kind],)
    return [c for c in range(4) if c not in base]


def pair_background(n, pair):
    """low everywhere, high on every third sample: both codes in every 16-sample word."""
    g = np.full(n, pair[0], dtype=np.uint8)
    g[1::3] = pair[1]
    return g


def diff_row(n, kind, ids, pair=D1_PAIR):
    """A row of difflist kind `kind` whose entries are the samples `ids`, their codes cycling through the others."""
    ids = np.asarray(ids, dtype=np.int64)
    g = pair_background(n, pair) if kind == 1 else np.full(n, CONST_OF[kind], dtype=np.uint8)
    cyc = [c for c in range(4) if c not in pair] if kind == 1 else others(kind)
    g[ids] = np.array(cyc, dtype=np.uint8)[np.arange(len(ids)) % len(cyc)]
    return Row(kind, g, pair=pair if kind == 1 else None)


def designed_gaps(n):
    """name -> (first sample, gaps): the gap streams that put a varint on a designed byte of a trip.  One group's gaps
    are 63, so the streams that need a trip's 64th byte run over two groups; the first id of the second group is the
    sample after the first group's last, and the gap between them is not stored."""
    one = [1]
    out = {
        # 3 + 2 + 58 bytes, then a 2-byte varint on byte 63; 60 gaps before it
        "d6_mix123_v2_at63": (0, [16384, 128] + one * 58 + [200, 1, 16500, 129, 1]),
        # 62 one-byte gaps, then a 3-byte varint on bytes 62, 63 | 0
        "d6_v3_at62": (1, one * 62 + [16385] + one * 3),
        # a 2-byte varint, 61 one-byte gaps, then a 3-byte varint on bytes 63 | 0, 1: 62 gaps before it
        "d6_v3_at63": (2, [130] + one * 61 + [16386] + one * 3),
        # 63 one-byte gaps fill group 0 and bytes 0..62; group 1 opens with a 2-byte varint on byte 63, so the trip
        # takes exactly group 0's gaps and the next one starts on a group
        "d6_trip_ends_group": (3, one * 63 + [128, 1, 1]),
    }
    return {name: v for name, v in out.items() if v[0] + sum(v[1]) + len(v[1]) // GAPS < n}


def entries_of_gaps(first, gaps):
    """The sample ids of a difflist with the given stored gaps: every 64th entry opens a group, with an outright id one
    above the last entry's."""
    ids = [first]
    for k, g in enumerate(gaps):
        if k and k % GAPS == 0:
            ids.append(ids[-1] + 1)
        ids.append(ids[-1] + g)
    return np.array(ids, dtype=np.int64)


def phase_bits(n, name, count):
    return _rng(n, name + "/info").integers(0, 2, count).astype(np.uint8)


def phase_designs(n):
    """tag -> (explicit, het samples, present bit per het or None): the phase rows without their store suffix."""
    out = {}
    words = (n + 63) // 64
    for explicit, form in ((False, "implicit"), (True, "explicit")):
        for h in PHASE_HETS:
            if 2 * h <= n:
                out[f"ph_{form}_het{h}"] = (explicit, 3 + spread(n - 3, h), (np.arange(h) % 3 != 1).astype(np.uint8))
        out[f"ph_{form}_word64"] = (explicit, 128 + np.arange(64), (np.arange(64) % 2).astype(np.uint8))
        out[f"ph_{form}_split1_63"] = (explicit, 127 + np.arange(64), (np.arange(64) % 2 == 0).astype(np.uint8))
        if n % 64:
            last = np.arange(64 * (words - 1), n)
            out[f"ph_{form}_lastword"] = (explicit, last, (np.arange(len(last)) % 4 != 0).astype(np.uint8))
        if words > SCAN_WORDS + 1:
            s = 64 * SCAN_WORDS + spread(n - 64 * SCAN_WORDS, 100)
            out[f"ph_{form}_beyond256"] = (explicit, s, (np.arange(100) % 5 != 2).astype(np.uint8))
    out["ph_explicit_none_het8"] = (True, 3 + spread(n - 3, 8), np.zeros(8, dtype=np.uint8))
    out["ph_explicit_all_het65"] = (True, 3 + spread(n - 3, 65), np.ones(65, dtype=np.uint8))
    for f in PHASE_FLAGS:
        present = np.zeros(PHASE_FLAG_HETS, dtype=np.uint8)
        present[(np.arange(f) * PHASE_FLAG_HETS) // f] = 1
        out[f"ph_explicit_flag{f}_het{PHASE_FLAG_HETS}"] = (True, 3 + spread(n - 3, PHASE_FLAG_HETS), present)
    return out


def patched(codes):
    """The row with 65 samples spread over it changed, each to a code other than its own."""
    n = len(codes)
    at = 2 + spread(n - 2, 65)
    out = codes.copy()
    out[at] = (out[at] + 1 + np.arange(65) % 3) % 4
    return out


def ld_run(n, b):
    """The six rows of the LD run off a base of kind b."""
    name = f"ldbase_d{b}"
    if b == 0:
        base = Row(0, common(n, name))
    elif b == 1:
        base = diff_row(n, 1, spread(n, min(100, n // 3)), pair=(1, 3))
    else:
        base = diff_row(n, b, 1 + spread(n - 1, min(100, n // 3)))
    out = {name: base}
    out[f"ld2_empty_on_d{b}"] = Row(2, base.codes.copy(), name)
    out[f"ld3_empty_on_d{b}"] = Row(3, INV[base.codes], name)
    out[f"ld2_E65_on_d{b}"] = Row(2, patched(base.codes), name)
    out[f"ld3_E65_on_d{b}"] = Row(3, INV[patched(base.codes)], name)
    out[f"ld3_E1_same_on_d{b}"] = Row(3, INV[base.codes], name, keep=np.array([n // 2], dtype=np.int64))
    return out


def rows(n):
    """name -> Row, in file order, for the sample counts up to N_WIDE.  An LD row directly follows its run."""
    assert n in SAMPLE_COUNTS
    out = {}
    # ---- difflist lengths and placements
    counts = ENTRY_COUNTS + ((n,) if n <= 256 else ())
    for kind in DIFF_KINDS:
        for e in counts:
            for where in PLACEMENTS:
                s = placement(n, e, where)
                if s is not None:
                    out[f"d{kind}_E{e}_{where}"] = diff_row(n, kind, s)
    # ---- gap streams
    for e in GAP1_COUNTS:
        if RUN1_FIRST + e <= n:
            out[f"d6_gap1_E{e}"] = diff_row(n, 6, RUN1_FIRST + np.arange(e))
    for g in GAP_VALUES:
        e = min(GAP_ROW_ENTRIES, (n - 1) // g + 1)
        if e >= 2:
            out[f"d6_gap{g}"] = diff_row(n, 6, g * np.arange(e, dtype=np.int64))
    for name, (first, gaps) in designed_gaps(n).items():
        out[name] = diff_row(n, 6, entries_of_gaps(first, gaps))
    if n > 130:
        out["d6_run130_last"] = diff_row(n, 6, n - 130 + np.arange(130))
    # ---- word boundaries
    for s in sorted({0, 15, 16, 63, 64, n - 1} | set(range(n - n % 16, n))):
        out[f"d4_at{s}"] = diff_row(n, 4, [s])
    # ---- type 1 and type 0
    for low, high in PAIRS:
        tag = f"d1_pair{low}{high}"
        out[tag] = diff_row(n, 1, [], pair=(low, high))
        out[tag + "_E65"] = diff_row(n, 1, 1 + spread(n - 1, 65), pair=(low, high))
        out[tag + "_dirty"] = diff_row(n, 1, [n - 1], pair=(low, high))._replace(dirty=True)
    out["d0_common"] = Row(0, common(n, "d0_common"))
    out["d0_dirty"] = Row(0, common(n, "d0_dirty"), dirty=True)
    # ---- LD runs
    for b in BASE_KINDS:
        out.update(ld_run(n, b))
    # ---- phase tracks
    for tag, (explicit, hets, present) in phase_designs(n).items():
        for store in PHASE_STORES:
            name = f"{tag}_d{store}"
            g = np.zeros(n, dtype=np.uint8)
            g[hets] = 1
            if store == 0:  # a literal row holds the other codes too, off the hets
                free = np.flatnonzero(g == 0)
                g[free[::7]] = 2
                g[free[3::11]] = 3
            info = phase_bits(n, name, int(present.sum()) if explicit else len(hets))
            out[name] = Row(store, g, phase=(explicit, present if explicit else None, info))
    out["d4_E0_end"] = diff_row(n, 4, [])  # an empty record ends the file
    return out


def big_rows(n):
    """The few rows of the two sample counts whose gaps and ids take four bytes."""
    assert n in BIG_COUNTS
    out = {}
    out["d1_pair02_E65"] = diff_row(n, 1, 1 + spread(n - 1, 65), pair=(0, 2))
    out["ld3_E65_on_d1"] = Row(3, INV[patched(out["d1_pair02_E65"].codes)], "d1_pair02_E65")
    for g in GAP_VALUES[-2:]:
        e = (n - 1) // g + 1
        first = (n - 1) - g * (e - 1)  # the last entry is sample N-1
        out[f"d6_gap{g}"] = diff_row(n, 6, first + g * np.arange(e, dtype=np.int64))
    # 61 one-byte gaps, then a 4-byte varint on bytes 61, 62, 63 | 0, then a group change
    out["d4_v4_at61"] = diff_row(n, 4, entries_of_gaps(0, [1] * 61 + [1 << 21, 1, 1, 1]))
    out["d7_E129_last"] = diff_row(n, 7, n - 129 + np.arange(129))
    out["d0_dirty"] = Row(0, common(n, "d0_dirty"), dirty=True)
    return out


def catalogue(n):
    return big_rows(n) if n in BIG_COUNTS else rows(n)


def pack_rows(geno):
    """uint8[m][ceil(n / 4)]: the 2-bit rows, unused bits clear."""
    m, n = geno.shape
    out = np.zeros((m, (n + 3) // 4), dtype=np.uint8)
    for j in range(4):
        part = geno[:, j::4]
        out[:, :part.shape[1]] |= part << (2 * j)
    return out


def phase_arrays(row):
    """(present bool[n], info bool[n]) of a row's phase track over the samples; info only where present."""
    n = len(row.codes)
    present, info = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    if row.phase is None:
        return present, info
    explicit, flags, bits = row.phase
    hets = np.flatnonzero(row.codes == 1)
    flagged = hets[np.asarray(flags, dtype=bool)] if explicit else hets
    present[flagged] = True
    info[flagged] = np.asarray(bits, dtype=bool)
    return present, info


class Layout:
    """The file of one sample count: names[v], the rows and the (m, n) matrix, with the writer's arguments."""

    def __init__(self, n):
        cat = catalogue(n)
        self.n = n
        self.names = list(cat)
        self.rows = list(cat.values())
        self.m = len(self.names)
        self.at = {name: v for v, name in enumerate(self.names)}
        self.geno = np.stack([r.codes for r in self.rows])
        self.kinds = [r.kind for r in self.rows]
        self.packed = pack_rows(self.geno)
        self.counts = np.stack([(self.geno == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)
        self.phase_rows = [v for v, r in enumerate(self.rows) if r.phase is not None]
        last_base = None
        for v, r in enumerate(self.rows):  # the format's rule: an LD record refers to the last non-LD record
            if r.kind in (2, 3):
                assert r.base == last_base, (n, self.names[v])
            else:
                last_base = self.names[v]

    def write(self, W, path):
        W.write_pgen(path, self.geno, self.kinds, record_opts=[r.options() for r in self.rows],
                     phase_tracks=[r.phase for r in self.rows] if self.phase_rows else None)

    def ld_runs(self):
        """[(base variant, [its LD variants])]."""
        out = []
        for v, r in enumerate(self.rows):
            if r.kind in (2, 3):
                out[-1][1].append(v)
            else:
                out.append((v, []))
        return [run for run in out if run[1]]
