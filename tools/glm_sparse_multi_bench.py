#!/usr/bin/env python3
"""Times pgh_glm_sparse_multi on the sparse-resident dataset of a rare-variant file against the only other route for
many quantitative phenotypes over carrier lists, one pgh_glm_sparse call per phenotype, in the same process; modelled
on tools/glm_score_sparse_multi_bench.py.

The file is tools/glm_sparse_bench.py's (written straight from carrier lists, shared when --dir is the same).  Shape:
500K samples x 1M variants at about 0.1 % carriers, 10 covariates, P = 1, 8, 64 phenotypes with about 3 % missing
values each (every phenotype its own missing-value pattern).  Both routes are timed through the C entry points with
the output array allocated and touched beforehand, so a time is the library call alone.  Per P: seconds per call
(median of --reps after one warm-up call); the seconds of the same call over ONE variant, which is the staging of the
block (the means on the host, the uploads, the value block and the whole-call Grams), and its share of the whole call;
the rest of the call against the algorithmic traffic of the walk, entries x (8 P + 8 kp + 4) bytes.  The single calls
are timed for --singles phenotypes, once each after a warm-up call, and scaled to P.  Per P a handful of rows are
compared with the single calls (errcode, obs_ct and a1_freq equal, the estimates within 1e-9), and the call is
repeated and must return the same bytes.
--profile: one P = 64 call after a warm-up call of one variant and nothing else, for a kernel trace.
One JSON line per P.

usage: python tools/glm_sparse_multi_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001]
                                              [--phenotypes 1,8,64] [--reps 3] [--singles 8] [--dir DIR]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402
from tools.sparse_bench import carrier_rows, write_carrier_pfile  # noqa: E402

K = 10

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--rate", type=float, default=0.001)
ap.add_argument("--missing", type=float, default=0.03)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=8, help="single pgh_glm_sparse calls timed (0: none)")
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n = args.variants, args.samples
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))

rng = np.random.default_rng(1)
z = np.ascontiguousarray(rng.standard_normal((K, n)))
counts = [64] if args.profile else [int(p) for p in args.phenotypes.split(",")]
p_max = max(counts)
Y_all = 0.3 * z.sum(axis=0)[None, :] + rng.standard_normal((p_max, n))
Y_all[rng.random((p_max, n)) < args.missing] = np.nan

sp = L.Dataset.open(prefix + ".pgen", sparse=True)
info = sp.sparse_info()
raw = L.raw()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def call_multi(Y, rows, v0=None, v1=None):
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    v0 = sp.v_begin if v0 is None else v0
    v1 = sp.v_end if v1 is None else v1
    t0 = time.perf_counter()
    rc = raw.pgh_glm_sparse_multi(sp._h, None, v0, v1, Y.shape[0], _ptr(Y), K, _ptr(z), _ptr(rows), eb)
    t = time.perf_counter() - t0
    assert rc == L.PGH_OK, eb.value.decode()
    return t


def call_single(y, rows):
    eb = C.create_string_buffer(L.ERRBUF_LEN)
    t0 = time.perf_counter()
    rc = raw.pgh_glm_sparse(sp._h, None, sp.v_begin, sp.v_end, _ptr(y), K, _ptr(z), _ptr(rows), eb)
    t = time.perf_counter() - t0
    assert rc == L.PGH_OK, eb.value.decode()
    return t


if args.profile:
    rows = np.zeros((m, 64), dtype=L.GLM_ROW_DTYPE)
    call_multi(Y_all, rows, sp.v_begin, sp.v_begin + 1)
    call_multi(Y_all, rows)
    sp.close()
    sys.exit(0)

single_each, single_rows = None, {}
if args.singles:
    one = np.zeros(m, dtype=L.GLM_ROW_DTYPE)
    call_single(np.ascontiguousarray(Y_all[0]), one)  # warm-up
    total = 0.0
    for p in range(args.singles):
        total += call_single(np.ascontiguousarray(Y_all[p % p_max]), one)
        single_rows[p % p_max] = one.copy()
    single_each = total / args.singles

CHECK_ROWS = np.unique(np.concatenate([np.arange(0, m, max(1, m // 8)), [m - 1]]))


def rows_agree(got, want):
    """The linear contract on the handful of rows: decisions equal, estimates within 1e-9 on check_rows' scale."""
    worst = 0.0
    for key in ("errcode", "obs_ct", "firth"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True)
    se = np.nan_to_num(want["se"], nan=0.0)
    for key in ("beta", "se", "stat", "p"):
        g, e = got[key], want[key]
        assert np.array_equal(np.isnan(g), np.isnan(e)), key
        scale = np.abs(e) + (se if key == "beta" else 1.0 if key == "stat" else 0.0)
        ok = ~np.isnan(e)
        if ok.any():
            worst = max(worst, float((np.abs(g - e)[ok] / (scale[ok] + 1e-300)).max()))
    assert worst <= 1e-9, worst
    return worst


kp = next(w for w in (0, 1, 2, 4, 8, 12, 16, 20) if w >= K)
for P in counts:
    Y = np.ascontiguousarray(Y_all[:P])
    rows = np.zeros((m, P), dtype=L.GLM_ROW_DTYPE)
    call_multi(Y, rows)  # warm-up (scratch growth, code objects)
    first = rows[CHECK_ROWS].copy()
    digest = hash(rows.tobytes()) if P <= 8 else hash(rows[:: max(1, m // 4096)].tobytes())
    times = [call_multi(Y, rows) for _ in range(args.reps)]
    t = float(np.median(times))
    again = hash(rows.tobytes()) if P <= 8 else hash(rows[:: max(1, m // 4096)].tobytes())
    assert again == digest and rows[CHECK_ROWS].tobytes() == first.tobytes(), "a repeated call returned other bytes"
    t_stage = float(np.median([call_multi(Y, rows, sp.v_begin, sp.v_begin + 1) for _ in range(args.reps)]))
    worst = None
    for p, want in single_rows.items():
        if p < P:
            w = rows_agree(first[:, p], want[CHECK_ROWS])
            worst = w if worst is None else max(worst, w)
    codes, ct = np.unique(first["errcode"], return_counts=True)
    blocks = (P + 63) // 64
    walk_bytes = float(info.entry_ct) * sum(8 * min(64, P - 64 * b) + 8 * kp + 4 for b in range(blocks))
    rec = {
        "phenotypes": P, "shape": f"{m}x{n}", "entries": int(info.entry_ct), "covariates": K,
        "missing_rate": round(float(np.isnan(Y).mean()), 4),
        "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times],
        "staging_seconds": round(t_stage, 6), "staging_share": round(t_stage / t, 4),
        "single_calls_seconds": None if single_each is None else round(single_each * P, 6),
        "single_call_seconds": None if single_each is None else round(single_each, 6),
        "singles_timed": args.singles,
        "speedup": None if single_each is None else round(single_each * P / t, 2),
        "walk_bytes": walk_bytes, "walk_bytes_per_s_of_the_rest": walk_bytes / max(t - t_stage, 1e-9),
        "rows_checked_against_singles": int(len(CHECK_ROWS) * sum(p < P for p in single_rows)),
        "worst_deviation_from_singles": worst, "repeat_same_bytes": True,
        "errcodes_of_checked_rows": {str(c): int(k) for c, k in zip(codes.tolist(), ct.tolist())},
    }
    print(json.dumps(rec), flush=True)
sp.close()
