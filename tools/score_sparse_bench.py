#!/usr/bin/env python3
"""Times pgh_score_sparse (Dataset.score_sparse) on the sparse-resident dataset of a rare-variant file, with 1 and 16
weight columns, and in the same run the existing per-sample sparse tally (Dataset.sample_counts on the same dataset
and variants), which does the same walk of the entries with +1s: the figure to set it against (DESIGN.md section
3.11, pgh_score_sparse).

The file is tools/glm_sparse_bench.py's: written straight from carrier lists, never through a dense matrix.
Per call: seconds (median of --reps after one warm-up call) and nanoseconds per entry over the entries of the scored
variants.  The results of the timed calls are compared byte for byte.
One JSON line.

usage: python tools/score_sparse_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--scored N]
                                          [--cols 1,16] [--reps 3] [--dir DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402
from tools.sparse_bench import carrier_rows, write_carrier_pfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--rate", type=float, default=0.001)
ap.add_argument("--scored", type=int, default=0, help="variants scored, from the first on (default: all)")
ap.add_argument("--cols", default="1,16")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n = args.variants, args.samples
scored = args.scored or m
assert 1 <= scored <= m
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
t0 = time.perf_counter()
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))
rec = {"shape": f"{m}x{n}", "carrier_rate_max": 2 * args.rate, "scored_variants": scored,
       "file_bytes": os.path.getsize(prefix + ".pgen"), "write_s": round(time.perf_counter() - t0, 1)}


def timed(call):
    out = call()  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        again = call()
        times.append(time.perf_counter() - t)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_parts(out), _parts(again)))
    return out, float(np.median(times)), [round(x, 6) for x in times]


def _parts(out):
    return [a for a in out if a is not None] if isinstance(out, tuple) else [out]


t0 = time.perf_counter()
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
rec["sparse_open_s"] = round(time.perf_counter() - t0, 2)
info = sp.sparse_info()
rec.update(entries=int(info.entry_ct), sparse_rows=int(info.sparse_variant_ct), dense_rows=int(info.dense_variant_ct),
           sparse_resident_bytes=int(info.resident_bytes))
# the entries of the scored variants: per-variant counts of the calls off the base code (hom-ref in this file)
counts = sp.counts_range(0, scored).astype(np.int64)
entries = int((counts.sum(axis=1) - counts.max(axis=1)).sum())
rec["scored_entries"] = entries
vidx = np.arange(scored, dtype=np.uint32)
rng = np.random.default_rng(1)
_, t_tally, rec["sample_counts_times"] = timed(lambda: sp.sample_counts(0, scored))
rec.update(sample_counts_seconds_per_call=round(t_tally, 6), sample_counts_ns_per_entry=round(1e9 * t_tally / entries, 4))
for n_cols in [int(c) for c in args.cols.split(",")]:
    w = rng.standard_normal((scored, n_cols))
    for dos in (True, False):
        key = f"score_sparse_{n_cols}col" + ("" if dos else "_no_dosage_sum")
        _, t, rec[key + "_times"] = timed(lambda: sp.score_sparse(vidx, w, dosage_sum=dos))
        rec[key + "_seconds_per_call"] = round(t, 6)
        rec[key + "_ns_per_entry"] = round(1e9 * t / entries, 4)
        rec[key + "_over_sample_counts"] = round(t / t_tally, 2)
sp.close()
print(json.dumps(rec), flush=True)
