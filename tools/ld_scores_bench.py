#!/usr/bin/env python3
"""Times pgh_ld_scores (Dataset.ld_scores) against the two other routes over the same band, on pgh_synth_create data
(2 % missing calls), in the style of tools/ld_prune_bench.py.

Shape: --samples x --variants resident, window --window variants (default 100,000 x 5,000, window 500).  Before
anything is timed, ld_scores of the first 200 variants (both flag values) is compared with a numpy evaluation of the
definition from ld_window_sums' planes: counts equal, every score within T * 2^-52 * sum |term| of math.fsum of its T
terms; the result is in the output ("check").
  scores     seconds per ld_scores call: median of --reps after one warm-up call.  The call is the class counts, the
             band kernel, the copy of the tiles' partial sums and the host's additions.
  prune      seconds per ld_prune call on the same band in the same run (same main loop, one bit per pair instead of
             224 partial sums and counts per tile): scores / prune isolates the new epilogue and the partials copy.
  host       the route there was before: ld_window_sums rectangles of --host-anchors anchors x their window and a numpy
             reduction on the host (24 bytes per pair come back), median of --reps after a warm-up, scaled to the
             whole band by the number of band pairs.
One JSON line."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=100_000)
ap.add_argument("--variants", type=int, default=5_000)
ap.add_argument("--window", type=int, default=500)
ap.add_argument("--r2", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-anchors", type=int, default=960)
ap.add_argument("--no-host", action="store_true", help="time ld_scores and ld_prune only")
args = ap.parse_args()

n, m, w = args.samples, args.variants, args.window
win = np.minimum(np.arange(m, dtype=np.int64) + w, m).astype(np.uint32)


def terms_of(planes, unbiased):
    """(defined, term) elementwise from uint32 planes (6, na, nb): the header's formula, one operation a statement."""
    s = planes.astype(np.int64)
    num, va, vb = s[0] * s[3] - s[1] * s[2], s[0] * s[4] - s[1] ** 2, s[0] * s[5] - s[2] ** 2
    ok = (s[0] >= (3 if unbiased else 2)) & (va > 0) & (vb > 0)
    with np.errstate(all="ignore"):
        dn = num.astype(np.float64)
        top = dn * dn
        bottom = va.astype(np.float64) * vb.astype(np.float64)
        term = top / bottom
        if unbiased:
            rest = 1.0 - term
            adj = rest / (s[0] - 2).astype(np.float64)
            term = term - adj
    term[~ok] = 0.0
    return ok, term


def check(ds):
    v = min(m, 200)
    sub_win = np.minimum(win[:v], v).astype(np.int64)
    planes = ds.ld_window_sums(v_begin=0, v_end=v)
    idx = np.arange(v)
    band = (idx[None, :] > idx[:, None]) & (idx[None, :] < sub_win[:, None])
    for unbiased in (False, True):
        ok, term = terms_of(planes, unbiased)
        use = band & ok
        both = use | use.T
        sym = np.where(use, term, 0.0) + np.where(use, term, 0.0).T
        got, cnt = ds.ld_scores(win_end=sub_win.astype(np.uint32), unbiased=unbiased, want_counts=True, v_begin=0,
                                v_end=v)
        if not np.array_equal(cnt, both.sum(axis=1)):
            return f"MISMATCH(counts, unbiased {unbiased})"
        for k in range(v):
            terms = [1.0 if ok[k, k] else 0.0] + sym[k, both[k]].tolist()
            exp = math.fsum(terms)
            if abs(got[k] - exp) > len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms):
                return f"MISMATCH(score {k}, unbiased {unbiased}: {got[k]!r} against {exp!r})"
    return "ok"


def tiles_issued():
    total = 0
    for k0 in range(0, m, L.LD_TILE_A):
        lo, hi = k0 + 1, int(win[min(k0 + L.LD_TILE_A, m) - 1])
        if lo < hi:
            total += (hi - 1) // L.LD_TILE_B - lo // L.LD_TILE_B + 1
    return total


def median_of(fn):
    fn()  # warm-up (code objects, block cache)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(x, 6) for x in times]


def host_route(ds, anchors):
    """LD scores' band terms of the first `anchors` anchors from ld_window_sums rectangles, reduced in numpy: what a
    caller had to do before.  Returns the number of band pairs covered."""
    score = np.zeros(m)
    pairs = 0
    for a0 in range(0, anchors, L.LD_TILE_A):
        a1 = min(a0 + L.LD_TILE_A, anchors)
        b0, b1 = a0 + 1, int(win[a1 - 1])
        if b0 >= b1:
            continue
        planes = ds.ld_window_sums(a_range=(a0, a1), b_range=(b0, b1))
        ok, term = terms_of(planes, False)
        ka, ub = np.arange(a0, a1)[:, None], np.arange(b0, b1)[None, :]
        use = ok & (ub > ka) & (ub < win[a0:a1].astype(np.int64)[:, None])
        t = np.where(use, term, 0.0)
        score[a0:a1] += t.sum(axis=1)
        score[b0:b1] += t.sum(axis=0)
        pairs += int(((ub > ka) & (ub < win[a0:a1].astype(np.int64)[:, None])).sum())
    return pairs


ds = L.Dataset.synth(0, m, n, 20261017, 0.02)
checked = check(ds)
t_scores, scores_times = median_of(lambda: ds.ld_scores(win_end=win, want_counts=True))
t_prune, prune_times = median_of(lambda: ds.ld_prune(args.r2, win_end=win))
score = ds.ld_scores(win_end=win)
band = int((win.astype(np.int64) - np.arange(m) - 1).sum())
tiles = tiles_issued()
rec = {
    "shape": f"{n}x{m}", "window": w, "check": checked, "band_pairs": band, "tiles": tiles,
    "pairs_issued": tiles * L.LD_TILE_A * L.LD_TILE_B, "mean_score": round(float(score.mean()), 6),
    "scores_seconds_per_call": round(t_scores, 6), "scores_times": scores_times,
    "prune_seconds_per_call": round(t_prune, 6), "prune_times": prune_times,
    "scores_over_prune": round(t_scores / t_prune, 3),
    "partials_bytes_copied": tiles * (L.LD_TILE_A + L.LD_TILE_B) * 12,
}
if not args.no_host:
    anchors = min(args.host_anchors, m)
    covered = [0]

    def run_host():
        covered[0] = host_route(ds, anchors)

    t_part, host_times = median_of(run_host)
    t_host = t_part * band / covered[0]
    rec.update({
        "host_route": "ld_window_sums + numpy", "host_pairs_timed": covered[0],
        "host_fraction_of_band": round(covered[0] / band, 4), "host_seconds_timed": round(t_part, 6),
        "host_times": host_times, "host_seconds_whole_band_scaled": round(t_host, 4),
        "host_over_scores": round(t_host / t_scores, 2), "host_bytes_copied_whole_band": band * 24,
    })
print(json.dumps(rec), flush=True)
ds.close()
