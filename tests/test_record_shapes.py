"""The device record decoder under the structured records of tests/record_shapes.py.

Every analysis reads the 2-bit matrix pgh_open builds, and for a real file that matrix comes from k_decode_records
(decode.hip), WalkDifflistIds (decode_device.hpp) and k_phase_extract (phase.hip).  The catalogue puts records on their
hard edges: difflist lengths around the value section's byte, a group, 64 groups and 65 whole groups; gap varints at
every step of their length, on every byte of a 64-byte trip where they can straddle it, and trips that start 0, 1 and
62 gaps into a group or end on a group's last gap; entries next to every word boundary and in the ragged last word;
every type-1 pair; unused bits set in type-0 and type-1 records; LD runs off every base kind; phase tracks of exact
content at the byte steps of their header, the word steps of the het ranks and the second trip of the block scan.

The reference of every comparison is the catalogue's own arrays (np.array_equal, no tolerance anywhere).  The writer,
the oracle and the host normaliser come from one reading of the format, so the CPU half checks them against each other
and against the catalogue; the GPU half holds the device decoder to all of them, over every ingest route of pgh_open."""

import os
import re
import time
import types

import numpy as np
import pytest

import pgen_writer as W
import record_shapes as RS

ALL_COUNTS = RS.SAMPLE_COUNTS + RS.BIG_COUNTS
N_WIDE = RS.N_WIDE
STAGE_BYTES = 64 << 20  # api_dataset.cpp: the staging buffer of pgh_open


def _layout(n, _made={}):
    if n not in _made:
        _made[n] = RS.Layout(n)
    return _made[n]


# ---- the catalogue itself (no GPU) -------------------------------------------------------------------------------

def _entries(row):
    """The samples a record of a difflist kind lists."""
    if row.kind == 1:
        return np.flatnonzero((row.codes != row.pair[0]) & (row.codes != row.pair[1]))
    return np.flatnonzero(row.codes != {4: 0, 6: 2, 7: 3}[row.kind])


def _stored_gaps(ids):
    """The varint gaps of a difflist in stream order: 63 per group, none across a group change."""
    return np.concatenate([np.diff(ids[g:g + 64]) for g in range(0, len(ids), 64)] or [np.zeros(0, dtype=np.int64)])


def _varint_bytes(gaps):
    return 1 + sum((gaps >= step).astype(np.int64) for step in (1 << 7, 1 << 14, 1 << 21, 1 << 28))


def _trips(gaps):
    """[(k_base, gaps taken, [(byte of the trip, varint bytes)] of the taken varints and the first one not taken)]:
    the walk of a gap stream in 64-byte trips, each taking the varints that end inside it and the next starting
    behind the last of them -- WalkDifflistIds' trips, restated over the varint lengths alone."""
    size = _varint_bytes(gaps)
    start = np.cumsum(size) - size
    out, pos, k = [], 0, 0
    while k < len(gaps):
        j = k
        while j < len(gaps) and start[j] + size[j] <= pos + 64:
            j += 1
        assert j > k
        out.append((k, j - k, [(int(start[i] - pos), int(size[i])) for i in range(k, min(j + 1, len(gaps)))]))
        pos, k = int(start[j - 1] + size[j - 1]), j
    return out


def _cycle(row, ids, cyc):
    return np.array_equal(row.codes[ids], np.array(cyc, dtype=np.uint8)[np.arange(len(ids)) % len(cyc)])


def _check_row(n, name, row, cat):
    """What the row must hold, from its name alone -- written out independently of record_shapes.rows()."""
    g = row.codes
    assert g.dtype == np.uint8 and g.shape == (n,) and g.max() <= 3, name
    m = re.fullmatch(r"d([1467])_E(\d+)_(tile0|last|spread|end)", name)
    if m:
        kind, e, where = int(m.group(1)), int(m.group(2)), m.group(3)
        ids = _entries(row)
        want = {"tile0": np.arange(e), "end": np.arange(e), "last": n - e + np.arange(e),
                "spread": np.arange(e) * n // max(e, 1)}[where]
        assert row.kind == kind and np.array_equal(ids, want), name
        assert row.pair == ((0, 2) if kind == 1 else None) and row.base is None and not row.dirty, name
        assert _cycle(row, ids, {4: [1, 2, 3], 6: [0, 1, 3], 7: [0, 1, 2], 1: [1, 3]}[kind]), name
        if kind == 1 and e < n:
            rest = np.delete(g, ids)
            assert set(rest.tolist()) == {0, 2}, name
        return
    m = re.fullmatch(r"d6_gap1_E(\d+)", name)
    if m:
        e = int(m.group(1))
        ids = _entries(row)
        assert row.kind == 6 and np.array_equal(ids, 5 + np.arange(e)), name
        trips = _trips(_stored_gaps(ids))
        assert all(taken == 64 or k + taken == e - (e + 63) // 64 for k, taken, _ in trips), name
        phases = {k % 63 for k, _, _ in trips}
        assert phases >= ({0, 1} if e == 130 else set(range(63))), name
        if e == 4160:
            # the trip 62 gaps into its group ends that group and holds the whole of the next; the one behind it
            # starts on a group and holds exactly that group
            assert (62 * 64, 64) in {(k, taken) for k, taken, _ in trips} and trips[-1][:2] == (63 * 64, 63), name
        return
    m = re.fullmatch(r"d6_gap(\d+)", name)
    if m:
        gap = int(m.group(1))
        ids = _entries(row)
        assert row.kind == 6 and len(ids) >= 2 and (np.diff(ids) == gap).all(), name
        if n in RS.BIG_COUNTS:
            assert ids[-1] == n - 1 and len(ids) == (n - 1) // gap + 1, name
        else:
            assert ids[0] == 0 and len(ids) == min(200, (n - 1) // gap + 1), name
        assert gap in (127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21), name
        assert set(_varint_bytes(_stored_gaps(ids)).tolist()) == {1 + sum(gap >= 1 << s for s in (7, 14, 21))}, name
        return
    if name in ("d6_mix123_v2_at63", "d6_v3_at62", "d6_v3_at63", "d6_trip_ends_group", "d4_v4_at61"):
        ids = _entries(row)
        assert row.kind == int(name[1]), name
        gaps = _stored_gaps(ids)
        trips = _trips(gaps)
        first = trips[0]
        size, at = {"d6_mix123_v2_at63": (2, 63), "d6_v3_at62": (3, 62), "d6_v3_at63": (3, 63),
                    "d6_trip_ends_group": (2, 63), "d4_v4_at61": (4, 61)}[name]
        assert first[2][-1] == (at, size) and len(first[2]) == first[1] + 1, (name, first)  # the straddler is not taken
        assert len(trips) == 2 and trips[1][0] == first[1], name
        if name == "d6_trip_ends_group":
            assert first[1] == 63 and len(ids) > 65, name
        else:
            assert first[1] < 63 and len(gaps) > 63, "the second trip crosses into the next group"
        if name == "d6_mix123_v2_at63":
            assert {1, 2, 3} == set(_varint_bytes(gaps).tolist()), name
        return
    if name == "d6_run130_last":
        assert row.kind == 6 and np.array_equal(_entries(row), n - 130 + np.arange(130)), name
        return
    m = re.fullmatch(r"d4_at(\d+)", name)
    if m:
        assert row.kind == 4 and _entries(row).tolist() == [int(m.group(1))] and g[int(m.group(1))] == 1, name
        return
    m = re.fullmatch(r"d1_pair(\d)(\d)(_E65|_dirty)?", name)
    if m:
        low, high, what = int(m.group(1)), int(m.group(2)), m.group(3)
        ids = _entries(row)
        assert row.kind == 1 and row.pair == (low, high) and low < high and row.dirty == (what == "_dirty"), name
        assert len(ids) == {None: 0, "_E65": 65, "_dirty": 1}[what], name
        rest = np.delete(g, ids)
        assert set(rest.tolist()) == {low, high}, name
        assert _cycle(row, ids, [c for c in range(4) if c not in (low, high)]), name
        if what == "_dirty":
            assert ids[0] == n - 1, "the last used bit of the bit array belongs to an entry"
        full = g[:n - n % 16].reshape(-1, 16)  # both codes in every 16-sample word: the spread of the bit array shows
        assert (full == high).any(axis=1).all() and (full == low).any(axis=1).all(), name
        return
    if name in ("d0_common", "d0_dirty"):
        assert row.kind == 0 and row.dirty == (name == "d0_dirty") and set(np.unique(g).tolist()) == {0, 1, 2, 3}, name
        return
    m = re.fullmatch(r"ldbase_d([01467])", name)
    if m:
        assert row.kind == int(m.group(1)) and row.base is None, name
        assert len(set(g.tolist())) >= 3, "inverting the row changes it"
        return
    m = re.fullmatch(r"ld([23])_(empty|E65|E1_same)_on_d([01467])", name)
    if m:
        kind, what = int(m.group(1)), m.group(2)
        base_name = f"ldbase_d{m.group(3)}" if n not in RS.BIG_COUNTS else "d1_pair02_E65"
        assert row.kind == kind and row.base == base_name, name
        base = cat[base_name].codes
        target = g if kind == 2 else RS.INV[g]  # the record's difflist is against the row before inversion
        differs = np.flatnonzero(target != base)
        assert len(differs) == {"empty": 0, "E65": 65, "E1_same": 0}[what], name
        if what == "E65":
            assert differs[0] >= 1 and len(set(target[differs].tolist())) >= 3, name
        if what == "E1_same":
            assert row.keep is not None and len(row.keep) == 1 and 0 < row.keep[0] < n, name
        else:
            assert row.keep is None, name
        return
    m = re.fullmatch(r"ph_(implicit|explicit)_(\w+)_d([04])", name)
    assert m, f"a row the name check does not know: {name}"
    explicit, what, store = m.group(1) == "explicit", m.group(2), int(m.group(3))
    assert row.kind == store and row.phase is not None and row.phase[0] == explicit, name
    hets = np.flatnonzero(g == 1)
    present = np.asarray(row.phase[1]) if explicit else np.ones(len(hets), dtype=np.uint8)
    info = np.asarray(row.phase[2])
    assert len(present) == len(hets) and len(info) == int(present.sum()), name
    assert set(g.tolist()) == ({0, 1, 2, 3} if store == 0 else {0, 1}), name
    words = hets // 64
    mm = re.fullmatch(r"(none_|all_|flag(\d+)_)?het(\d+)", what)
    if mm:
        assert len(hets) == int(mm.group(3)), name
        if mm.group(1) == "none_":
            assert explicit and not present.any() and len(info) == 0, "zero phase-info bytes"
        elif mm.group(1) == "all_":
            assert explicit and present.all(), name
        elif mm.group(1):
            assert explicit and int(present.sum()) == int(mm.group(2)), name
        elif explicit:
            assert 0 < present.sum() < len(hets) or len(hets) == 1, name
    elif what == "word64":
        assert np.array_equal(hets, 128 + np.arange(64)) and len(set(words.tolist())) == 1, name
    elif what == "split1_63":
        assert len(hets) == 64 and np.bincount(words)[-2:].tolist() == [1, 63], name
    elif what == "lastword":
        assert n % 64 and np.array_equal(hets, np.arange(n - n % 64, n)), name
    elif what == "beyond256":
        assert hets.min() >= 64 * 256 and len(hets) == 100 and (n + 63) // 64 > 2 * 256, name
    else:
        raise AssertionError(f"a phase row the name check does not know: {name}")
    if len(info) >= 8:
        assert 0 < info.sum() < len(info), name


def _required(n):
    """The names the catalogue of a sample count must hold, written out from the edges themselves."""
    if n in RS.BIG_COUNTS:
        return ["d1_pair02_E65", "ld3_E65_on_d1", f"d6_gap{(1 << 21) - 1}", f"d6_gap{1 << 21}", "d4_v4_at61",
                "d7_E129_last", "d0_dirty"]
    out = []
    counts = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4160] + ([n] if n <= 256 else [])
    for kind in (4, 6, 7, 1):
        for e in counts:
            if e > n:
                continue
            out.append(f"d{kind}_E{e}_tile0")
            if 0 < e < n:
                out.append(f"d{kind}_E{e}_last")
                if 2 * e <= n:
                    out.append(f"d{kind}_E{e}_spread")
    out += ["d6_gap1_E130"] + (["d6_gap1_E4160"] if n > 4165 else [])
    out += [f"d6_gap{g}" for g in (127, 128, 16383, 16384) if n > g]
    if n > 40000:  # the rows that hold gaps of three bytes
        out += ["d6_mix123_v2_at63", "d6_v3_at62", "d6_v3_at63"]
    out += ["d6_trip_ends_group", "d6_run130_last"]
    out += [f"d4_at{s}" for s in sorted({0, 15, 16, 63, 64, n - 1} | set(range(n - n % 16, n)))]
    for pair in ("01", "02", "03", "12", "13", "23"):
        out += [f"d1_pair{pair}", f"d1_pair{pair}_E65", f"d1_pair{pair}_dirty"]
    out += ["d0_common", "d0_dirty"]
    for b in (0, 1, 4, 6, 7):
        out += [f"ldbase_d{b}"] + [f"{r}_on_d{b}" for r in ("ld2_empty", "ld3_empty", "ld2_E65", "ld3_E65", "ld3_E1_same")]
    phase = []
    for form in ("implicit", "explicit"):
        phase += [f"ph_{form}_het{h}" for h in (1, 7, 8, 15, 16, 63, 64, 65)]
        phase += [f"ph_{form}_word64", f"ph_{form}_split1_63"]
        phase += [f"ph_{form}_lastword"] if n % 64 else []
        phase += [f"ph_{form}_beyond256"] if n > 64 * 257 else []
    phase += ["ph_explicit_none_het8", "ph_explicit_all_het65", "ph_explicit_flag8_het100", "ph_explicit_flag64_het100",
              "ph_explicit_flag65_het100"]
    out += [f"{p}_d{store}" for p in phase for store in (0, 4)]
    return out + ["d4_E0_end"]


def test_the_sample_counts_sit_on_their_edges():
    assert (RS.DECODE_THREADS, RS.MIN_PLAIN_RUN) == (256, 256)
    assert [W._id_bytes(n) for n in RS.ID_COUNTS] == [1, 2, 2, 3] and W._id_bytes(RS.N_ID4) == 4
    assert W._id_bytes(RS.N_GAP4) == 3 and RS.N_GAP4 == (1 << 21) + 70 and RS.N_ID4 == (1 << 24) + 17
    assert N_WIDE > 1 << 14 and N_WIDE % 4 == 3 and N_WIDE % 16 == 15 and 0 < N_WIDE % 64 < 63
    assert (N_WIDE + 63) // 64 > 2 * 256, "three trips of the block prefix sum"
    assert N_WIDE // 4 // 4 > 2 * 256, "a workgroup takes more than two trips over the row's 32-bit words"
    # the unused bits the dirty rows set exist at every count that has such rows
    assert all(n % 8 for n in ALL_COUNTS if n not in (256, 65536)) and all(n % 4 for n in (255, 65535, N_WIDE) + RS.BIG_COUNTS)
    assert {n % 16 for n in ALL_COUNTS} >= {0, 1, 6, 15}, "type 1: the second byte of the last 16 bits is and is not there"


@pytest.mark.parametrize("n", ALL_COUNTS)
def test_the_catalogue_is_what_the_decoder_is_meant_to_see(n):
    """Every row holds what its name says and every required name is there, in an order in which an LD row follows
    its base; the file's route plan holds no plain run, so every record goes through the device decoder."""
    cat = RS.catalogue(n)
    assert sorted(cat) == sorted(_required(n)), (set(cat) ^ set(_required(n)))
    for name, row in cat.items():
        _check_row(n, name, row, cat)
    lay = _layout(n)
    runs = lay.ld_runs()
    if n in RS.BIG_COUNTS:
        assert len(cat) == 7 and [lay.kinds[v] for v in (0, 1)] == [1, 3]
        return
    assert [lay.kinds[b] for b, _ in runs] == [0, 1, 4, 6, 7]
    assert all([lay.kinds[v] for v in lds] == [2, 3, 2, 3, 3] and lds == list(range(b + 1, b + 6)) for b, lds in runs)
    literal = [k == 0 for k in lay.kinds]
    longest = max(len(run) for run in "".join("x" if x else " " for x in literal).split())
    assert longest < RS.MIN_PLAIN_RUN
    # the difflist lengths around every step, over all rows
    lens = {len(_entries(r)) for r in lay.rows if r.kind in (1, 4, 6, 7)}
    assert {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129} <= lens
    assert n < 4200 or {4095, 4096, 4097, 4160} <= lens
    assert n > 256 or n in lens
    if n == N_WIDE:
        sizes = set()
        for r in lay.rows:
            if r.kind in (4, 6, 7):
                sizes |= set(_varint_bytes(_stored_gaps(_entries(r))).tolist())
        assert sizes == {1, 2, 3}


def test_the_trip_walk_restated():
    """_trips on streams small enough to check by hand."""
    assert _trips(np.ones(64, dtype=np.int64)) == [(0, 64, [(i, 1) for i in range(64)])]
    assert [t[:2] for t in _trips(np.ones(130, dtype=np.int64))] == [(0, 64), (64, 64), (128, 2)]
    t = _trips(np.array([1] * 63 + [128, 1]))
    assert [x[:2] for x in t] == [(0, 63), (63, 2)] and t[0][2][-1] == (63, 2) and t[1][2][0] == (0, 2)
    assert _varint_bytes(np.array([127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21])).tolist() == [1, 2, 2, 3, 3, 4]


# ---- the files ---------------------------------------------------------------------------------------------------

class _File:
    def __init__(self, tmp, n):
        self.lay = lay = _layout(n)
        self.n = n
        self.path = str(tmp / f"records_{n}.pgen")
        lay.write(W, self.path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_shapes")
    made = {}

    def get(n):
        if n not in made:
            made[n] = _File(tmp, n)
        return made[n]

    return get


def _by_name(lay, got, want, ctx, v0=0):
    """np.array_equal over the variants, a failure naming the designed rows."""
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        raise AssertionError((ctx, len(bad), [lay.names[v0 + v] for v in bad[:12]]))


def _ld_starts(lay):
    """(begin, end) ranges: on the base of every LD run, on each of its LD rows and on the row behind it; and ranges
    that end inside the run."""
    out = []
    for b, lds in lay.ld_runs():
        behind = lds[-1] + 1
        for lo in [b] + lds + [behind]:
            out.append((lo, min(lay.m, behind + 3)))
        out += [(max(0, b - 2), lds[len(lds) // 2]), (b, lds[-1])]
    return out


@pytest.mark.parametrize("n", ALL_COUNTS)
def test_oracle_and_host_normaliser_read_the_written_records(files, oracle, lib, n):
    """Writer -> oracle (calls, record types, phase tracks) and -> the product's host normaliser, both equal to the
    catalogue; the host normaliser also over ranges that start on every row of every LD run."""
    f = files(n)
    lay = f.lay
    pg = oracle.Pgen(f.path)
    assert (pg.M, pg.N) == (lay.m, n) and pg.has_phase == bool(lay.phase_rows)
    for v, row in enumerate(lay.rows):
        assert pg.vrtype(v) == row.kind | (0x10 if row.phase is not None else 0), lay.names[v]
        got = pg.geno(v).astype(np.int16)
        got[got == -9] = 3
        assert np.array_equal(got, row.codes), lay.names[v]
    for v in lay.phase_rows:
        g, pp, pi = pg.phase(v)
        present, info = RS.phase_arrays(lay.rows[v])
        assert np.array_equal(pp != 0, present) and np.array_equal((pi != 0) & (pp != 0), info), lay.names[v]
    _by_name(lay, lib.normalize_range_host(f.path), lay.packed, (n, "host"))
    for lo, hi in _ld_starts(lay):
        _by_name(lay, lib.normalize_range_host(f.path, lo, hi), lay.packed[lo:hi], (n, "host", lo, hi), lo)


# ---- on the GPU --------------------------------------------------------------------------------------------------

def _open_both(L, path, monkeypatch, **kw):
    ds = L.Dataset.open(path, **kw)
    monkeypatch.setenv("PGH_HOST_NORMALIZE", "1")
    hosted = L.Dataset.open(path, **kw)
    monkeypatch.delenv("PGH_HOST_NORMALIZE")
    return (("device", ds), ("host", hosted))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_device_decode(gpu_lib, files, n, monkeypatch):
    """pgh_open's matrix equals the packed catalogue row for row, and the tallies equal the per-code counts; the same
    with every row expanded by the host normaliser."""
    f = files(n)
    lay = f.lay
    t0 = time.perf_counter()
    for how, ds in _open_both(gpu_lib, f.path, monkeypatch):
        _by_name(lay, ds.copy_rows_to_host(0, lay.m), lay.packed, (n, how))
        _by_name(lay, ds.counts_range(), lay.counts, (n, how, "counts"))
        ds.close()
    print(f"n={n}: {lay.m} records opened twice and compared in {time.perf_counter() - t0:.2f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_COUNTS)
def test_partial_opens(gpu_lib, files, n):
    """Ranges that open on the base of an LD run, on each of its LD rows (the leading LD rows go through the host, the
    next records through the device) and behind it, and ranges that end inside a run: each the slice of the catalogue."""
    f = files(n)
    lay = f.lay
    for lo, hi in _ld_starts(lay):
        part = gpu_lib.Dataset.open(f.path, variant_begin=lo, variant_end=hi)
        _by_name(lay, part.copy_rows_to_host(lo, hi), lay.packed[lo:hi], (n, lo, hi), lo)
        _by_name(lay, part.counts_range(), lay.counts[lo:hi], (n, lo, hi, "counts"), lo)
        part.close()


# ---- the routes of pgh_open ----------------------------------------------------------------------------------------

ROUTE_N = 773  # N % 4 = 1: six unused bits in a literal record's last byte; N % 8 = 5


def _route_mix():
    """[encoded, 255 literal, encoded, 256 literal, ld2, ld3, 257 literal, ld3, encoded]: names, rows."""
    n = ROUTE_N
    rows = []

    def literal(count, tag):
        for i in range(count):
            rows.append((f"{tag}_{i}", RS.Row(0, RS.common(n, f"{tag}_{i}"), dirty=True)))

    rows.append(("enc_a", RS.diff_row(n, 4, RS.spread(n, 65))))
    literal(255, "lit255")
    rows.append(("enc_b", RS.diff_row(n, 6, RS.spread(n, 70))))
    literal(256, "lit256")
    base = rows[-1][1].codes
    rows.append(("ld2_behind_256", RS.Row(2, base.copy(), "lit256_255")))
    rows.append(("ld3_behind_256", RS.Row(3, RS.INV[base], "lit256_255")))
    literal(257, "lit257")
    base = rows[-1][1].codes
    rows.append(("ld3_behind_257", RS.Row(3, RS.INV[RS.patched(base)], "lit257_256")))
    rows.append(("enc_c", RS.diff_row(n, 1, RS.spread(n, 5), pair=(1, 2))._replace(dirty=True)))
    return [name for name, _ in rows], [row for _, row in rows]


def _route_file(tmp_path):
    n = ROUTE_N
    names, rows = _route_mix()
    kinds = [r.kind for r in rows]
    runs = [len(x) for x in "".join("L" if k == 0 else " " for k in kinds).split()]
    assert runs == [RS.MIN_PLAIN_RUN - 1, RS.MIN_PLAIN_RUN, RS.MIN_PLAIN_RUN + 1] and n % 4 and n % 8
    assert [kinds[i] for i in (0, 256, 257 + 256, 258 + 256, 259 + 256 + 257)] == [4, 6, 2, 3, 3] and len(rows) == 774
    geno = np.stack([r.codes for r in rows])
    path = str(tmp_path / "routes.pgen")
    W.write_pgen(path, geno, kinds, record_opts=[r.options() for r in rows])
    first_literal = W.encode_record(0, geno[1], None, dirty_tail=True)
    assert first_literal[-1] >> 2 == 0x3F and first_literal in open(path, "rb").read(), "the dirty tails are in the file"
    return path, names, geno, RS.pack_rows(geno)


def test_the_route_mix_on_the_host(lib, oracle, tmp_path):
    """The oracle and the host normaliser read the route-mix file, dirty tails included, to the encoded rows."""
    path, names, geno, want = _route_file(tmp_path)
    pg = oracle.Pgen(path)
    for v in range(len(names)):
        got = pg.geno(v).astype(np.int16)
        got[got == -9] = 3
        assert np.array_equal(got, geno[v]), names[v]
    _by_name(types.SimpleNamespace(names=names), lib.normalize_range_host(path), want, "host")


@pytest.mark.gpu
def test_the_route_mix(gpu_lib, tmp_path, monkeypatch):
    """Literal runs of 255 (device route), 256 and 257 records (plain route: copy engine and LaunchSanitizeTail) with
    dirty tails, LD records directly behind a plain-route run (their base is its last row), encoded neighbours."""
    n = ROUTE_N
    path, names, geno, want = _route_file(tmp_path)
    at = {name: v for v, name in enumerate(names)}
    lay = types.SimpleNamespace(names=names)

    def unpack(row):
        return ((row[np.arange(n) // 4] >> (2 * (np.arange(n) % 4))) & 3).astype(np.uint8)

    for how, ds in _open_both(gpu_lib, path, monkeypatch):
        got = ds.copy_rows_to_host(0, len(names))
        _by_name(lay, got, want, how)
        # the LD rows against their base as the device holds it: the last row of the plain-route run
        base = unpack(got[at["lit256_255"]])
        assert np.array_equal(unpack(got[at["ld2_behind_256"]]), base), how
        assert np.array_equal(unpack(got[at["ld3_behind_256"]]), RS.INV[base]), how
        base = unpack(got[at["lit257_256"]])
        assert int((unpack(got[at["ld3_behind_257"]]) != RS.INV[base]).sum()) == 65, how
        assert (got[:, -1] >> 2 == 0).all(), "the unused bits of every row's last byte are clear"
        counts = np.stack([(geno == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)
        assert np.array_equal(ds.counts_range(), counts), how
        ds.close()
    # a range that opens on the LD records behind the plain run: host rows first, then the plain route again
    for lo in (at["ld2_behind_256"], at["ld3_behind_256"], at["ld3_behind_257"]):
        part = gpu_lib.Dataset.open(path, variant_begin=lo)
        _by_name(lay, part.copy_rows_to_host(lo, len(names)), want[lo:], ("from", lo), lo)
        part.close()


# ---- phase tracks ------------------------------------------------------------------------------------------------

def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", RS.SAMPLE_COUNTS)
def test_phase_tracks(gpu_lib, files, oracle, n, monkeypatch):
    """pgh_get_phased of every phase row against the oracle and the catalogue's own bits, from the device-expanded
    tracks and from the host parser's, without a subset and under one (test_phase_tracks_through_the_device_form's
    comparison)."""
    f = files(n)
    lay = f.lay
    pg = oracle.Pgen(f.path)
    mask = np.random.default_rng(n).random(n) < 0.5
    mask[[0, n - 1]] = True
    mask[128:192] = np.arange(64) % 2 == 0
    for how, ds in _open_both(gpu_lib, f.path, monkeypatch):
        assert ds.info.raw_variant_ct == lay.m
        for subset_mask in (None, mask):
            ss = ds.subset(subset_mask) if subset_mask is not None else None
            inc = None if subset_mask is None else subset_mask.astype(np.uint8)
            keep = slice(None) if subset_mask is None else subset_mask
            n_out = n if subset_mask is None else int(subset_mask.sum())
            rd = ds.reader(ss)
            for v in lay.phase_rows:
                ctx = (n, how, subset_mask is not None, lay.names[v])
                g, pp, pi = rd.get_phased(v)
                eg, epp, epi = pg.phase(v, inc)
                codes = (np.unpackbits(g.view(np.uint8), bitorder="little")[: 2 * n_out].reshape(-1, 2) * [1, 2]).sum(axis=1)
                assert np.array_equal(np.where(codes == 3, -9, codes), eg), ctx
                assert np.array_equal(_bits(pp, n_out), epp != 0), ctx
                assert np.array_equal(_bits(pi, n_out) & _bits(pp, n_out), (epi != 0) & (epp != 0)), ctx
                present, info = RS.phase_arrays(lay.rows[v])
                assert np.array_equal(codes, lay.geno[v][keep]), ctx
                assert np.array_equal(_bits(pp, n_out) != 0, present[keep]), ctx
                assert np.array_equal((_bits(pi, n_out) & _bits(pp, n_out)) != 0, info[keep]), ctx
            rd.close()
            if ss is not None:
                ss.close()
        ds.close()


# ---- staging batches ---------------------------------------------------------------------------------------------

STAGE_N = 1_000_003
STAGE_GROUPS = 3           # distinct [type 0, ld2, ld3, ld2] groups, cycled through
STAGE_LD_ENTRIES = (150_001, 90_001, 120_001)


def _stage_group(i):
    """Four rows [type 0, ld2, ld3, ld2] of distinct group i: the base and three rows that differ from it (from its
    inverse for type 3) at the given numbers of samples."""
    n = STAGE_N
    base = RS.common(n, f"stage_{i}")
    rows = [base]
    for j, (kind, e) in enumerate(zip((2, 3, 2), STAGE_LD_ENTRIES)):
        at = (j + i) % 5 + RS.spread(n - 5, e)
        target = base.copy()
        target[at] = (target[at] + 1 + (np.arange(e) + j) % 3) % 4
        rows.append(target if kind == 2 else RS.INV[target])
    return rows


def _stage_cuts(lens):
    """The first record of every staging batch behind the first, by api_dataset.cpp's byte budget: a batch of n records
    and raw bytes takes record r while raw + len(r) + 64 + 41 * (n + 2) <= the stage."""
    cuts, raw, count = [], 0, 0
    for r, ln in enumerate(lens):
        if count and raw + ln + 64 + 41 * (count + 2) > STAGE_BYTES:
            cuts.append(r)
            raw = count = 0
        raw += ln
        count += 1
    return cuts


def _stage_records(_made=[]):
    """(groups, records, order, lens, cuts): the distinct rows and their records, the (group, record) of every
    variant of the file, the record lengths and the budget's cuts."""
    if not _made:
        groups = [_stage_group(i) for i in range(STAGE_GROUPS)]
        records = [[W.encode_record(kind, row, rows[0]) for kind, row in zip((0, 2, 3, 2), rows)] for rows in groups]
        per_group = [sum(len(r) for r in recs) for recs in records]
        reps = STAGE_BYTES // min(per_group) + 2
        order = [(g % STAGE_GROUPS, j) for g in range(reps) for j in range(4)]
        lens = [len(records[i][j]) for i, j in order]
        _made.append((groups, records, order, lens, _stage_cuts(lens)))
    return _made[0]


def test_the_stage_budget_cuts_in_front_of_an_ld_record():
    """The byte budget of api_dataset.cpp, restated in _stage_cuts, ends the first staging batch of the file of
    test_an_ld_record_opens_a_staging_batch directly in front of an LD record: a changed budget fails here instead of
    silently moving the cut."""
    text = open(os.path.join(RS.CSRC, "api_dataset.cpp")).read()
    assert "64ull << 20" in text and re.search(r"raw \+ len \+ 64 \+ 41ull \* \(n \+ 2\) > stage_bytes", text)
    groups, records, order, lens, cuts = _stage_records()
    assert STAGE_N // 4 + 4096 < STAGE_BYTES and sum(lens) > STAGE_BYTES
    assert all(len(records[i][0]) == (STAGE_N + 3) // 4 for i in range(STAGE_GROUPS))
    assert cuts and any(order[c][1] != 0 for c in cuts), ("no cut in front of an LD record", [order[c] for c in cuts])
    assert _stage_cuts([10, 20, STAGE_BYTES, 5]) == [2, 3] and _stage_cuts([STAGE_BYTES - 64 - 41 * 3 - 1, 1]) == []
    assert _stage_cuts([STAGE_BYTES - 64 - 41 * 3 - 1, 2]) == [1]


@pytest.mark.gpu
def test_an_ld_record_opens_a_staging_batch(gpu_lib, tmp_path):
    """A file whose record bytes exceed the 64 MiB stage, built record by record: the budget of api_dataset.cpp,
    restated here, cuts it directly in front of an LD record, whose base was decoded by the batch before.  The
    tallies of every row and the rows on both sides of every cut are exact."""
    n = STAGE_N
    groups, records, order, lens, cuts = _stage_records()
    assert cuts and any(order[c][1] != 0 for c in cuts), ("no cut in front of an LD record", [order[c] for c in cuts])
    path = str(tmp_path / "stage.pgen")
    W.write_records(path, n, [(0, 2, 3, 2)[j] for _, j in order], [records[i][j] for i, j in order])
    packed = [RS.pack_rows(np.stack(rows)) for rows in groups]
    counts = [np.stack([(np.stack(rows) == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32) for rows in groups]
    t0 = time.perf_counter()
    ds = gpu_lib.Dataset.open(path)
    t1 = time.perf_counter()
    got = ds.counts_range()
    want = np.stack([counts[i][j] for i, j in order])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, ("counts", bad[:8], cuts)
    for c in cuts:
        lo, hi = max(0, c - 4), min(len(order), c + 4)
        rows = ds.copy_rows_to_host(lo, hi)
        for v in range(lo, hi):
            i, j = order[v]
            assert np.array_equal(rows[v - lo], packed[i][j]), (v, order[v], "cut at", c)
    ds.close()
    print(f"{len(order)} records, {sum(lens) >> 20} MiB, cuts at {[(c, order[c]) for c in cuts]}: opened in "
          f"{t1 - t0:.2f} s, checked in {time.perf_counter() - t1:.2f} s")
