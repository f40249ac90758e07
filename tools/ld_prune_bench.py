#!/usr/bin/env python3
"""Times pgh_ld_prune (Dataset.ld_prune) against the only other route to the same sums, pgh_ld_pairs_dev over the same
band of pairs, on pgh_synth_create data (2 % missing calls), in the style of tools/king_bench.py.

Shape: --samples x --variants resident, window --window variants (default 500,000 x 100,000, window 1,000), r2
threshold --r2.  Before anything is timed, ld_window_sums of a 150 x 200 rectangle is compared with ld_pairs on the
same pairs, and ld_prune over the first 2,000 variants with the rule run in numpy from ld_pairs' sums; both results are
in the output ("check").
  prune      seconds per ld_prune call: median of --reps after one warm-up call.  The call is the class counts, the
             band kernel, the copy of the band bits and the host's sequential rule.
  yardstick  pgh_ld_pairs_dev on the band pairs of the first --yardstick-anchors anchors (a stated fraction of the
             band: the whole band's sums would be 24 bytes x 1e8 pairs), median of --reps after a warm-up, device
             synchronised, scaled to the whole band by the number of pairs.
The int8 rate uses the model 2 ops x 6 products x samples x pairs issued, where pairs issued counts whole 96 x 128
tiles that meet the band, over the 5e15 op/s dense int8 peak; it is the whole call's rate, not the kernel's (the
kernel's own time is in a rocprofv3 kernel trace of this tool).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

INT8_PEAK = 5e15

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=100_000)
ap.add_argument("--window", type=int, default=1000)
ap.add_argument("--r2", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--yardstick-anchors", type=int, default=2000)
ap.add_argument("--no-yardstick", action="store_true", help="time ld_prune only (for a kernel trace)")
args = ap.parse_args()

n, m, w = args.samples, args.variants, args.window
win = np.minimum(np.arange(m, dtype=np.int64) + w, m).astype(np.uint32)


def band_pairs(k0, k1):
    a = np.concatenate([np.full(int(win[k]) - k - 1, k, dtype=np.uint32) for k in range(k0, k1)])
    b = np.concatenate([np.arange(k + 1, int(win[k]), dtype=np.uint32) for k in range(k0, k1)])
    return a, b


def tiles_issued():
    total = 0
    for k0 in range(0, m, L.LD_TILE_A):
        lo, hi = k0 + 1, int(win[min(k0 + L.LD_TILE_A, m) - 1])
        if lo < hi:
            total += (hi - 1) // L.LD_TILE_B - lo // L.LD_TILE_B + 1
    return total


def exceeds(s, t):
    s = s.astype(np.int64)
    num = s[:, 0] * s[:, 3] - s[:, 1] * s[:, 2]
    va, vb = s[:, 0] * s[:, 4] - s[:, 1] ** 2, s[:, 0] * s[:, 5] - s[:, 2] ** 2
    ok = (s[:, 0] >= 2) & (va > 0) & (vb > 0)
    with np.errstate(all="ignore"):
        r2 = (num.astype(np.float64) * num.astype(np.float64)) / (va.astype(np.float64) * vb.astype(np.float64))
    return ok & (r2 > t)


def check(ds):
    got = ds.ld_window_sums(v_begin=0, v_end=min(m, 400), a_range=(0, 150), b_range=(100, 300))
    a, b = np.divmod(np.arange(150 * 200, dtype=np.uint32), np.uint32(200))
    sums_ok = np.array_equal(ds.ld_pairs(a, b + 100), np.stack([got[p][a, b] for p in range(6)], axis=1))
    v = min(m, 2000)
    sub_win = np.minimum(win[:v], v).astype(np.uint32)
    t = 2.0 / n  # unrelated synthetic variants: r2 is of the order of 1 / samples
    ka = np.concatenate([np.full(int(sub_win[k]) - k - 1, k, dtype=np.uint32) for k in range(v)])
    ub = np.concatenate([np.arange(k + 1, int(sub_win[k]), dtype=np.uint32) for k in range(v)])
    hit = exceeds(ds.ld_pairs(ka, ub), t)
    counts = ds.counts_range(0, v).astype(np.int64)
    alt, obs = counts[:, 1] + 2 * counts[:, 2], 2 * counts[:, :3].sum(axis=1)
    mc = np.minimum(alt, obs - alt)
    keep = np.ones(v, dtype=bool)
    by_anchor = np.split(ub[hit], np.searchsorted(ka[hit], np.arange(1, v)))
    for k in range(v):
        if keep[k]:
            for u in by_anchor[k]:
                if keep[u]:
                    if int(mc[k]) * int(obs[u]) < int(mc[u]) * int(obs[k]):
                        keep[k] = False
                        break
                    keep[u] = False
    prune_ok = np.array_equal(ds.ld_prune(t, win_end=sub_win, v_begin=0, v_end=v), keep) and 0 < keep.sum() < v
    return "ok" if sums_ok and prune_ok else f"MISMATCH(sums {sums_ok}, prune {prune_ok})"


ds = L.Dataset.synth(0, m, n, 20261017, 0.02)
checked = check(ds)
kept = int(ds.ld_prune(args.r2, win_end=win).sum())  # warm-up (code objects, block cache)
times = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    kept = int(ds.ld_prune(args.r2, win_end=win).sum())
    times.append(time.perf_counter() - t0)
t_prune = float(np.median(times))
band = int((win.astype(np.int64) - np.arange(m) - 1).sum())
issued = tiles_issued() * L.LD_TILE_A * L.LD_TILE_B
ops = 2 * 6 * n * issued
rec = {
    "shape": f"{n}x{m}", "window": w, "r2": args.r2, "check": checked, "kept": kept, "band_pairs": band,
    "pairs_issued": issued, "prune_seconds_per_call": round(t_prune, 6), "prune_times": [round(x, 6) for x in times],
    "int8_ops": ops, "int8_ops_per_second": ops / t_prune, "int8_peak_fraction": round(ops / t_prune / INT8_PEAK, 4),
}
if not args.no_yardstick:
    import torch

    ya = min(args.yardstick_anchors, m)
    a, b = band_pairs(0, ya)
    d_sums = torch.empty((len(a), 6), dtype=torch.int32, device="cuda")
    ytimes = []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.ld_pairs_dev(a, b, d_sums.data_ptr(), 0)
        torch.cuda.synchronize()
        if rep:
            ytimes.append(time.perf_counter() - t0)
    t_part = float(np.median(ytimes))
    t_yard = t_part * band / len(a)
    rec.update({
        "yardstick": "pgh_ld_pairs_dev", "yardstick_pairs_timed": len(a), "yardstick_fraction_of_band": len(a) / band,
        "yardstick_seconds_timed": round(t_part, 6), "yardstick_times": [round(x, 6) for x in ytimes],
        "yardstick_seconds_whole_band_scaled": round(t_yard, 4), "speedup": round(t_yard / t_prune, 2),
    })
print(json.dumps(rec), flush=True)
ds.close()
