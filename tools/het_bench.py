#!/usr/bin/env python3
"""Times pgh_het (Dataset.het) on pgh_synth_create data, in the style of tools/grm_bench.py.

Two cases over a resident matrix of --variants x --samples calls (default 1,000,000 x 500,000, 125 GB of 2-bit rows):
2 % missing calls (QC'd biobank data has a few per cent) and 50 % missing calls, which shows how the cost of the new
kernel follows the missing calls -- it adds one LDS atomic per missing call.  --slices times Dataset.het under other
numbers of variant slices than the default as well (the rows must be the same bytes).  Per case, in the same run and
over the same rows, the median of --reps calls after one warm-up call of
  het             Dataset.het (counts pass, host tables, three-class column tally, k_het_missing_sum, copies)
  sample_counts   pgh_sample_counts (the three-class column tally alone, and its copy)
  counts_range    pgh_counts_range (the row tally alone, and its copy)
and "read_floor_seconds": the bytes of ONE read of the matrix at 8 TB/s.  Dataset.het reads the matrix three times.
Before anything is timed the first 200 variants are compared with a numpy evaluation of the header's formulas
("check": "ok" or "MISMATCH"; e_sum as an exact int64 product).  One JSON line per case.

The kernel's own time is not in these numbers: take it from a separate run of this tool under
rocprofv3 --kernel-trace --stats (k_het_missing_sum's row), e.g. with --reps 1 --cases 2."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

HBM_RATE = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cases", default="2,50", help="comma list of missing-call percentages")
ap.add_argument("--slices", default="", help="comma list of PGH_HET_SLICES values to time Dataset.het under as well")
ap.add_argument("--skip-check", action="store_true", help="no comparison with numpy first (a profiler run)")
args = ap.parse_args()


def unpack(rows, n):
    return ((rows[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(rows.shape[0], -1)[:, :n]


def check(ds):
    """The first variants against numpy: e from lib.het_expected (itself pinned by tests/test_het_host.py)."""
    n, v = ds.n_samples, min(200, ds.v_end)
    codes = unpack(ds.copy_rows_to_host(0, v), n)
    k = L.het_scale(v)
    q = np.zeros(v, dtype=np.int64)
    used = np.zeros(v, dtype=np.uint8)
    for i in range(v):
        c = codes[i]
        e = L.het_expected(int((c == 1).sum()), int((c == 2).sum()), int((c != 3).sum()))
        if e is not None:
            q[i], used[i] = int(np.rint(np.float64(e) * 2.0 ** k)), 1
    called = (codes != 3) & (used[:, None] == 1)
    hom = (((codes == 0) | (codes == 2)) & (used[:, None] == 1)).sum(axis=0)
    e_sum = called.astype(np.int64).T @ q
    rows, got_used, n_used = ds.het(v_begin=0, v_end=v)
    ok = (np.array_equal(got_used, used) and n_used == int(used.sum()) and np.array_equal(rows["e_sum"], e_sum)
          and np.array_equal(rows["obs_ct"], called.sum(axis=0)) and np.array_equal(rows["hom_ct"], hom)
          and np.array_equal(rows["e_hom"], np.ldexp(e_sum.astype(np.float64), -k)))
    return "ok" if ok else "MISMATCH"


def median_seconds(call):
    """(median seconds, every time, the last call's result) of --reps calls after one warm-up call."""
    out = call()  # warm-up (code objects, block cache)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(x, 6) for x in times], out


for pct in [int(x) for x in args.cases.split(",")]:
    m, n = args.variants, args.samples
    ds = L.Dataset.synth(0, m, n, 20261021, pct / 100.0)
    checked = "skipped" if args.skip_check else check(ds)
    t_het, all_het, (rows, _, n_used) = median_seconds(ds.het)
    t_sc, all_sc, _ = median_seconds(ds.sample_counts)
    t_cr, all_cr, _ = median_seconds(ds.counts_range)
    by_slices = {}
    for slices in [x for x in args.slices.split(",") if x]:
        os.environ[L.HET_SLICES_ENV] = slices
        t, _, (rows_s, _, _) = median_seconds(ds.het)
        by_slices[slices] = round(t, 6) if rows_s.tobytes() == rows.tobytes() else "MISMATCH"
    os.environ.pop(L.HET_SLICES_ENV, None)
    matrix_bytes = m * ds.info.pitch_bytes
    print(json.dumps({
        "case": f"missing{pct}", "shape": f"{m}x{n}", "missing_rate": pct / 100.0, "check": checked, "n_used": n_used,
        "het_seconds_per_call": round(t_het, 6), "het_times": all_het,
        "sample_counts_seconds_per_call": round(t_sc, 6), "sample_counts_times": all_sc,
        "counts_range_seconds_per_call": round(t_cr, 6), "counts_range_times": all_cr,
        "matrix_bytes": matrix_bytes, "read_floor_seconds": round(matrix_bytes / HBM_RATE, 6),
        "het_over_sample_counts": round(t_het / t_sc, 3), "het_seconds_by_slices": by_slices,
        "mean_f": round(float(np.nanmean(rows["f"])), 6),
    }), flush=True)
    ds.close()
