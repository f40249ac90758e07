"""pgh_het's host side, with no device: pgh_het_expected and pgh_het_scale against the yardstick of
tests/het_oracle.py bit for bit, the refusals that need no dataset, and the fixed-point bound of the header against
exact rational sums."""

import ctypes as C
import math
import os
import struct
from fractions import Fraction

import numpy as np

import het_oracle as H
from conftest import ROOT

NAMES = ("pgh_het", "pgh_het_expected", "pgh_het_scale")


def bits(x):
    return None if x is None else struct.pack("<d", x)


def test_header_declares_and_library_exports_het(lib):
    header = open(os.path.join(ROOT, "include", "pgenhip.h")).read()
    for name in NAMES:
        assert name + "(" in header
        assert name in lib.EXPORTED_SYMBOLS
        assert hasattr(lib.raw(), name)
    assert "PGH_HET_SMALL_SAMPLE = 1" in header and f"#define PGH_HET_TILE {lib.HET_TILE}" in header
    assert lib.HET_SMALL_SAMPLE == 1 and lib.HET_SLICES_ENV == "PGH_HET_SLICES"
    assert C.sizeof(lib.PghHetRow) == 32 == lib.HET_ROW_DTYPE.itemsize == H.ROW_DTYPE.itemsize
    assert lib.HET_ROW_DTYPE == H.ROW_DTYPE
    for name, _ in lib.PghHetRow._fields_:
        assert getattr(lib.PghHetRow, name).offset == lib.HET_ROW_DTYPE.fields[name][1]
    # two workgroups and more fit the 160 KiB of LDS of a compute unit, at 8 bytes a sample
    assert lib.HET_TILE % 64 == 0 and 2 * 8 * lib.HET_TILE <= 160 * 1024


def test_het_expected_is_the_formula_bit_for_bit_on_random_counts(lib):
    rng = np.random.default_rng(20261021)
    top = 2 ** 31 - 1
    n = 0
    for hi in (3, 50, 5000, 10 ** 6, top):
        for _ in range(800):
            called = int(rng.integers(1, hi + 1))
            het = int(rng.integers(0, called + 1))
            alt = int(rng.integers(0, called - het + 1))
            for small in (True, False):
                assert bits(lib.het_expected(het, alt, called, None, small)) == bits(H.expected(het, alt, called, None, small))
                n += 1
    assert n >= 4000


def test_het_expected_at_the_edges(lib):
    top = 2 ** 31 - 1
    for small in (True, False):
        # nothing called; monomorphic either way: skipped
        for het, alt, called in ((0, 0, 0), (0, 0, 7), (0, 7, 7), (0, top, top), (0, 0, top)):
            assert lib.het_expected(het, alt, called, None, small) is None
            assert H.expected(het, alt, called, None, small) is None
        for het, alt, called in ((1, 0, 2), (1, 1, 2), (top, 0, top), (1, 0, top), (top // 2, top // 2, top)):
            assert bits(lib.het_expected(het, alt, called, None, small)) == bits(H.expected(het, alt, called, None, small))
    # one call, which is het: p = 0.5, u = 0.5, and the correction 2 / 1 makes it 1
    assert lib.het_expected(1, 0, 1, None, True) == 0.0 == H.expected(1, 0, 1, None, True)
    assert lib.het_expected(1, 0, 1, None, False) == 0.5 == H.expected(1, 0, 1, None, False)
    # supplied frequencies (no correction with them)
    for freq in (0.0, 1.0, -0.1, math.inf, -math.inf, 1.5):
        assert lib.het_expected(3, 1, 10, freq, False) is None and H.expected(3, 1, 10, freq, False) is None
    for freq in (0.5, 5e-324, 1e-300, 0.25, 1.0 - 2.0 ** -53, 0.1):
        got = lib.het_expected(3, 1, 10, freq, False)
        assert got is not None and 0.0 <= got <= 1.0
        assert bits(got) == bits(H.expected(3, 1, 10, freq, False))
    assert lib.het_expected(3, 1, 10, 0.5, False) == 0.5 and lib.het_expected(3, 1, 10, 5e-324, False) == 1.0
    assert lib.het_expected(3, 1, 0, 0.5, False) is None  # nothing called: skipped whatever the frequency
    raw = lib.raw()
    e = C.c_double(-7.0)
    # NaN: the frequency of the counts
    assert raw.pgh_het_expected(3, 1, 10, math.nan, 0, C.byref(e)) == 1 and bits(e.value) == bits(H.expected(3, 1, 10, None, False))
    # refused: unknown flags, the correction with a frequency, no destination; *e is left alone
    e = C.c_double(-7.0)
    assert raw.pgh_het_expected(3, 1, 10, math.nan, 2, C.byref(e)) == 0
    assert raw.pgh_het_expected(3, 1, 10, 0.5, 1, C.byref(e)) == 0
    assert raw.pgh_het_expected(3, 1, 10, math.nan, 0, None) == 0
    assert raw.pgh_het_expected(0, 10, 10, math.nan, 0, C.byref(e)) == 0
    assert e.value == -7.0


def test_het_scale(lib):
    want = {0: 62, 1: 62, 2: 61, 3: 60, 4: 60, 5: 59, 2 ** 20: 42, 2 ** 20 + 1: 41, 2 ** 31 - 1: 31, 2 ** 31: 31,
            2 ** 31 + 1: 30, 2 ** 32 - 1: 30}
    for n_var, k in want.items():
        assert lib.het_scale(n_var) == k == H.scale(n_var), n_var
    # n_var terms of at most 2^k each cannot pass 2^62
    for n_var in (1, 2, 3, 1000, 2 ** 20 + 1, 2 ** 31 - 1):
        assert n_var * 2 ** lib.het_scale(n_var) <= 2 ** 62


def test_flags_are_refused_before_anything_else(lib):
    """Unknown flag bits, and the small-sample correction together with freq, are PGH_ERR_ARG with their own message
    even with no dataset at all: the binding level needs no device for them.  Nothing is written."""
    raw = lib.raw()
    freq = np.full(4, 0.25)
    out = np.full(4, 0x5A, dtype=np.uint8).repeat(32).view(lib.HET_ROW_DTYPE)
    used = np.full(4, 9, dtype=np.uint8)
    before = out.tobytes()
    n_used = C.c_uint32(77)
    for f, flags, text in ((freq, lib.HET_SMALL_SAMPLE, "freq"), (None, 2, "unknown flag bits"),
                           (freq, 6, "unknown flag bits"), (None, 0, "null argument")):
        eb = C.create_string_buffer(lib.ERRBUF_LEN)
        rc = raw.pgh_het(None, None, 0, 4, None, None if f is None else f.ctypes.data_as(C.c_void_p), flags,
                         out.ctypes.data_as(C.c_void_p), used.ctypes.data_as(C.c_void_p), C.byref(n_used), eb)
        assert rc == lib.PGH_ERR_ARG and text in eb.value.decode()
        assert out.tobytes() == before and (used == 9).all() and n_used.value == 77


def test_fixed_point_sum_is_within_its_bound_of_the_exact_sum(lib):
    """|e_hom - exact| <= obs_ct 2^-(k+1) + 2^-53 exact, exact = the rational sum of the doubles e_v: every q_v is
    within half a unit of e_v 2^k, the integer sum is exact, and the one conversion to double rounds once."""
    rng = np.random.default_rng(7)
    for n_var in (1, 2, 3, 37, 1000, 4097):
        k = lib.het_scale(n_var)
        es = []
        while len(es) < n_var:
            called = int(rng.integers(1, 3000))
            het = int(rng.integers(0, called + 1))
            alt = int(rng.integers(0, called - het + 1))
            e = lib.het_expected(het, alt, called, None, bool(len(es) % 2))
            if e is not None:
                es.append(e)
        for obs in sorted({1, n_var // 2 + 1, n_var}):
            take = rng.choice(n_var, size=obs, replace=False)
            e_sum = sum(H.fixed(es[i], k) for i in take)
            assert 0 <= e_sum <= 2 ** 62
            exact = sum(Fraction(es[i]) for i in take)
            e_hom = math.ldexp(float(e_sum), -k)
            assert abs(Fraction(e_hom) - exact) <= Fraction(obs, 2 ** (k + 1)) + Fraction(1, 2 ** 53) * exact
            assert 0.0 <= e_hom <= obs
