#!/usr/bin/env python3
"""Times pgh_grm (Dataset.grm) on pgh_synth_create data (2 % missing calls), in the style of tools/king_bench.py.

Cases (samples x variants; "small": a quick check of the tool itself):
  square10k   the full square at 10,000 x 100,000 (rel and nobs, 1.2 GB copied to pageable host memory)
  matmul10k   the route a user has without pgh_grm, same data: Z (variants x samples, float64, 8 GB) expanded on the
              device, then torch.matmul(Z.T, Z).  The expansion is not timed and the result stays on the device.
  rect8k      one 8,192 x 8,192 rectangle at 50,000 x 100,000
  band50k     the first tile row (GRM_TILE rows, the band a full square of this size is walked in) of the
              50,000 x 100,000 square as a rectangle call (every tile of that row), and
              "full_square_estimate_seconds": that time scaled by (tiles of the triangle) / (tiles of the row) -- an
              estimate, labelled as such, not a measurement of the full call
Before anything is timed a 200 x 200 rectangle over 1,000 variants is compared with a numpy float64 product of the
same rows ("check": the largest |rel nobs - num| over the bound of tests/test_grm.py, which must be below 1).  The
full square's own result is checked too ("square_check", the same ratio): its first corner, the block of the first
rows and last columns, and the block of the last rows and first columns -- which a call in several bands fills from
the first band's mirror strip -- each 200 x 200 over all variants.  Per
case: seconds per call (median of --reps after one warm-up call) and the FP64 rate by the model 2 x n_used x pairs
issued, where pairs issued counts whole 128 x 128 tiles (the triangle's for the full square; the matmul issues the
whole square), over the 78.6e12 FLOP/s FP64 matrix peak.  The rate is the whole call's (counts, transpose, kernel,
copy), not the kernel's.  One JSON line per case."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

FP64_PEAK = 78.6e12
TILE = L.GRM_TILE
CASES = {
    "square10k": ("square", 10_000, 100_000), "matmul10k": ("matmul", 10_000, 100_000),
    "rect8k": ("rect", 50_000, 100_000), "band50k": ("band", 50_000, 100_000),
    "small_square": ("square", 3_000, 20_000), "small_matmul": ("matmul", 3_000, 20_000),
    "small_rect": ("rect", 3_000, 20_000), "small_band": ("band", 3_000, 20_000),
}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cases", default="square10k,matmul10k,rect8k,band50k", help="comma list of: " + ", ".join(CASES))
args = ap.parse_args()


def unpack(rows, n):
    return ((rows[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(rows.shape[0], -1)[:, :n]


def tables(counts):
    """float64[v][4] from uint32[v][4] class counts (hom-ref, het, hom-alt, missing); skipped variants are all 0."""
    out = np.zeros((len(counts), 4))
    used = 0
    for k, c in enumerate(counts):
        p, z = L.grm_standardize(int(c[1]), int(c[2]), int(c[0]) + int(c[1]) + int(c[2]))
        if z is not None:
            out[k, :3] = z
            used += 1
    return out, used


def class_counts(codes):
    return np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)


def check(ds):
    """One small rectangle against numpy, from the dataset's own rows; the frequencies are those of all samples."""
    n, v = ds.n_samples, min(1000, ds.v_end)
    codes = unpack(ds.copy_rows_to_host(0, v), n)
    tab, used = tables(class_counts(codes))
    i0, i1, j0, j1 = 0, min(200, n), max(0, min(300, n - 200)), min(500, n)
    za = np.take_along_axis(tab, codes[:, i0:i1].astype(np.int64), axis=1)
    zb = np.take_along_axis(tab, codes[:, j0:j1].astype(np.int64), axis=1)
    num, s = za.T @ zb, np.abs(za).T @ np.abs(zb)
    rel, nobs, got_used = ds.grm(v_begin=0, v_end=v, i_range=(i0, i1), j_range=(j0, j1))
    exp_nobs = ((codes[:, i0:i1] != 3).astype(np.float64).T @ (codes[:, j0:j1] != 3).astype(np.float64))
    if got_used != used or not np.array_equal(nobs, exp_nobs.astype(np.uint32)):
        return "MISMATCH"
    lim = 2.0 * (used + 16) * 2.0 ** -53 * s + 2.0 ** -52 * np.abs(num)
    return round(float((np.abs(rel * nobs - num) / lim).max()), 4)


def block_error(ds, tab, used, rel, nobs, i0, j0, side=200):
    """largest |rel nobs - num| / bound over the block [i0, i0 + side) x [j0, j0 + side) of a whole-square result."""
    def z_of(s0):
        b0, b1 = s0 // 4, (s0 + side + 3) // 4
        zs = []
        for v0 in range(0, ds.v_end, 8192):
            rows = ds.copy_rows_to_host(v0, min(ds.v_end, v0 + 8192))[:, b0:b1]
            codes = unpack(rows, 4 * (b1 - b0))[:, s0 - 4 * b0:s0 - 4 * b0 + side]
            zs.append((np.take_along_axis(tab[v0:v0 + len(codes)], codes.astype(np.int64), axis=1), codes != 3))
        return np.concatenate([z for z, _ in zs]), np.concatenate([c for _, c in zs]).astype(np.float64)
    (za, ca), (zb, cb) = z_of(i0), z_of(j0)
    num, s = za.T @ zb, np.abs(za).T @ np.abs(zb)
    r, c = rel[i0:i0 + side, j0:j0 + side], nobs[i0:i0 + side, j0:j0 + side]
    if not np.array_equal(c, (ca.T @ cb).astype(np.uint32)):
        return math.inf
    lim = 2.0 * (used + 16) * 2.0 ** -53 * s + 2.0 ** -52 * np.abs(num)
    return float((np.abs(r * c - num) / lim).max())


def square_check(ds):
    n = ds.n_samples
    side = min(200, n)
    tab, used = tables(ds.counts_range())
    rel, nobs, got_used = ds.grm()
    if got_used != used or rel.tobytes() != np.ascontiguousarray(rel.T).tobytes():
        return "MISMATCH"
    worst = max(block_error(ds, tab, used, rel, nobs, i0, j0, side) for i0, j0 in [(0, 0), (0, n - side), (n - side, 0)])
    return round(worst, 4) if math.isfinite(worst) else "MISMATCH"


def expand_on_device(ds):
    """Z as a device float64 tensor (variants x samples), 4,096 variants at a time."""
    import torch
    n, m = ds.n_samples, ds.v_end
    dev = torch.device("cuda")
    z = torch.empty((m, n), dtype=torch.float64, device=dev)
    shifts = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=dev)
    used = 0
    for v0 in range(0, m, 4096):
        v1 = min(m, v0 + 4096)
        rows = torch.from_numpy(ds.copy_rows_to_host(v0, v1)).to(dev)
        codes = ((rows[:, :, None] >> shifts) & 3).reshape(v1 - v0, -1)[:, :n].to(torch.int64)
        counts = torch.stack([(codes == c).sum(dim=1) for c in range(4)], dim=1).cpu().numpy()
        tab, u = tables(counts)
        used += u
        z[v0:v1] = torch.gather(torch.from_numpy(tab).to(dev), 1, codes)
    return z, used


datasets = {}
for name in args.cases.split(","):
    kind, n, m = CASES[name]
    if (n, m) not in datasets:
        for d in datasets.values():
            d[0].close()
        datasets.clear()
        ds = L.Dataset.synth(0, m, n, 20261017, 0.02)
        datasets[(n, m)] = (ds, check(ds))
    ds, checked = datasets[(n, m)]
    tiles = (n + TILE - 1) // TILE
    extra = {}
    if kind == "square":
        issued = tiles * (tiles + 1) // 2 * TILE * TILE

        extra["square_check"] = square_check(ds)

        def call():
            return ds.grm()[2]
    elif kind == "matmul":
        import torch
        z, used = expand_on_device(ds)
        issued = n * n

        def call():
            g = torch.matmul(z.T, z)
            torch.cuda.synchronize()
            del g
            return used
    elif kind == "rect":
        side = min(8192, n)
        issued = ((side + TILE - 1) // TILE) ** 2 * TILE * TILE

        def call():
            return ds.grm(i_range=(0, side), j_range=(n - side, n))[2]
    else:
        band = min(TILE, n)  # one tile row: what the library walks a full square of 50,000 samples in
        band_tiles = 1
        issued = band_tiles * tiles * TILE * TILE
        extra["band_rows"] = band

        def call():
            return ds.grm(i_range=(0, band), j_range=(0, n))[2]
    n_used = call()  # warm-up (code objects, block cache)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        n_used = call()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    flop = 2 * n_used * issued
    rec = {
        "case": name, "shape": f"{n}x{m}", "kind": kind, "check": checked, "n_used": n_used,
        "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times], "pairs_issued": issued,
        "fp64_flop": flop, "fp64_flop_per_second": flop / t, "fp64_peak_fraction": round(flop / t / FP64_PEAK, 4),
    }
    if kind == "band":
        scale = (tiles * (tiles + 1) // 2) / (band_tiles * tiles)
        extra["full_square_estimate_seconds"] = round(t * scale, 3)
        extra["full_square_estimate_is"] = "tile row time x triangle tiles / row tiles: a scaled estimate, not a measurement"
    if kind == "matmul":
        del z
        torch.cuda.empty_cache()
    rec.update(extra)
    print(json.dumps(rec), flush=True)
for d in datasets.values():
    d[0].close()
