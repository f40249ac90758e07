"""Sparse-resident datasets against dense ones on REF-major rare-variant files.

The fixtures are written straight from carrier lists as type-4 records (difflists against hom-ref), never through
a dense matrix: the biobank shape is 125 GB dense.  Per shape it reports, dense against sparse:
  - pgh_open / pgh_open_sparse time (the file was just written: warm page cache)
  - resident bytes
  - the per-sample class-count kernel time (pgh_sample_counts_dev, median of --reps)
  - the end-to-end read_pfile(orient := 'sample', genotypes := 'counts') scan, the setting off and on

usage: python tools/sparse_bench.py [--shapes ref,biobank] [--dir DIR] [--reps 5]
Shapes: ref = 30,000 variants x 100,000 samples at MAF <= 0.005 (the reference's bench_sample_counts_sparse.sh);
biobank = 500,000 variants x 1,000,000 samples at ~0.1 % carriers.
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {
    "ref": dict(m=30_000, n=100_000, rate=0.005, seed=11),
    "biobank": dict(m=500_000, n=1_000_000, rate=0.001, seed=12),
}


def _varints(d: np.ndarray) -> np.ndarray:
    """LEB128 bytes of every value of d (uint64), concatenated."""
    nb = np.ones(d.size, dtype=np.int64)
    for j in range(1, 5):
        nb += d >= (1 << (7 * j))
    start = np.cumsum(nb) - nb
    out = np.zeros(int(nb.sum()), dtype=np.uint8)
    for j in range(5):
        sel = nb > j
        if not sel.any():
            break
        byte = ((d[sel] >> np.uint64(7 * j)) & np.uint64(0x7F)).astype(np.uint8)
        byte |= (nb[sel] > j + 1).astype(np.uint8) << 7
        out[start[sel] + j] = byte
    return out


def difflist_record(ids: np.ndarray, codes: np.ndarray, n: int) -> bytes:
    """A type-4 main track: ids ascending, codes 1..3 (the samples that are not hom-ref)."""
    ln = len(ids)
    head = bytearray()
    x = ln
    while x >= 0x80:
        head.append((x & 0x7F) | 0x80)
        x >>= 7
    head.append(x)
    if ln == 0:
        return bytes(head)
    w = 1 if n < 0x100 else 2 if n < 0x10000 else 3 if n < 0x1000000 else 4
    ids = ids.astype(np.uint64)
    groups = (ln + 63) // 64
    firsts = ids[::64]
    first_bytes = ((firsts[:, None] >> (8 * np.arange(w, dtype=np.uint64))) & np.uint64(0xFF)).astype(np.uint8)
    gaps = np.diff(ids)
    gaps[63::64] = 0  # placeholders at group boundaries, dropped below
    keep = np.ones(len(gaps), dtype=bool)
    keep[63::64] = False
    vb = _varints(gaps)
    # per-group byte lengths of the gap sections (for the biased length bytes between groups)
    nb = np.ones(len(gaps), dtype=np.int64)
    for j in range(1, 5):
        nb += gaps >= (1 << (7 * j))
    byte_keep = np.repeat(keep, nb)
    group_of_gap = np.arange(len(gaps)) // 64
    lens = np.bincount(group_of_gap[keep], weights=nb[keep], minlength=groups).astype(np.int64)
    pad = (-ln) % 4
    c = np.concatenate([codes.astype(np.uint8), np.zeros(pad, dtype=np.uint8)]).reshape(-1, 4)
    packed = (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)
    return (bytes(head) + first_bytes.tobytes() + ((lens[:-1] - 63) & 0xFF).astype(np.uint8).tobytes()
            + packed.tobytes() + vb[byte_keep].tobytes())


def carrier_rows(m: int, n: int, rate: float, seed: int):
    """Per variant: carriers ~ Binomial(n, U(0, 2 rate)) samples, codes mostly het, some hom-alt / missing."""
    rng = np.random.default_rng(seed)
    for _ in range(m):
        k = int(rng.binomial(n, rng.uniform(0, 2 * rate)))
        ids = np.unique(rng.integers(0, n, k))
        codes = rng.choice(np.array([1, 1, 1, 2, 3], dtype=np.uint8), len(ids))
        yield ids, codes


def write_carrier_pfile(prefix: str, m: int, n: int, rows) -> None:
    """prefix.pgen (mode 0x10, 8-bit vrtypes, 4-byte lengths, every record type 4) + .pvar + .psam."""
    body = prefix + ".pgen.body"
    lens = np.zeros(m, dtype=np.uint32)
    with open(body, "wb") as f:
        for v, (ids, codes) in enumerate(rows):
            rec = difflist_record(ids, codes, n)
            lens[v] = len(rec)
            f.write(rec)
    blocks = (m + 65535) // 65536
    head = bytearray([0x6C, 0x1B, 0x10]) + int(m).to_bytes(4, "little") + int(n).to_bytes(4, "little")
    head.append(0x40 | 4 | 3)
    table_len = blocks * 8 + m * 5
    fp = len(head) + table_len
    offsets, tables = [], bytearray()
    for b in range(blocks):
        offsets.append(fp)
        lo, hi = b * 65536, min(m, (b + 1) * 65536)
        tables += bytes([4]) * (hi - lo)
        tables += lens[lo:hi].astype("<u4").tobytes()
        fp += int(lens[lo:hi].sum())
    with open(prefix + ".pgen", "wb") as f:
        f.write(head)
        for o in offsets:
            f.write(int(o).to_bytes(8, "little"))
        f.write(tables)
        with open(body, "rb") as src:
            shutil.copyfileobj(src, f, 64 << 20)
    os.remove(body)
    with open(prefix + ".pvar", "w") as f:
        f.write("#CHROM\tPOS\tID\tREF\tALT\n")
        f.writelines(f"1\t{v + 1}\tr{v}\tA\tG\n" for v in range(m))
    with open(prefix + ".psam", "w") as f:
        f.write("#IID\tSEX\n")
        f.writelines(f"s{i}\tNA\n" for i in range(n))


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def bench_shape(name: str, shape: dict, out_dir: str, reps: int) -> dict:
    import torch

    import plinking_duck_amd.lib as L
    import plinking_duck_amd.functions as F

    m, n = shape["m"], shape["n"]
    prefix = os.path.join(out_dir, f"sparse_{name}")
    t = time.perf_counter()
    if not os.path.exists(prefix + ".pgen"):
        write_carrier_pfile(prefix, m, n, carrier_rows(m, n, shape["rate"], shape["seed"]))
    res = {"shape": name, "variants": m, "samples": n, "carrier_rate_max": 2 * shape["rate"],
           "file_bytes": os.path.getsize(prefix + ".pgen"), "write_s": round(time.perf_counter() - t, 1)}
    padded = (n + 63) // 64 * 64
    d_cls = torch.empty(3 * padded, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()

    def kernel_ms(ds):
        def once():
            ds.sample_counts_dev(0, m, d_cls.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
        once()
        return _median_ms(once, reps)

    # sparse first: a dense form that does not fit HBM is reported as such
    t = time.perf_counter()
    sp = L.Dataset.open(prefix + ".pgen", sparse=True)
    res["sparse_open_s"] = round(time.perf_counter() - t, 2)
    si = sp.sparse_info()
    res.update(sparse_resident_bytes=int(si.resident_bytes), dense_bytes=int(si.dense_bytes),
               sparse_rows=int(si.sparse_variant_ct), dense_rows=int(si.dense_variant_ct), entries=int(si.entry_ct))
    res["sparse_kernel_ms"] = round(kernel_ms(sp), 3)
    res["sparse_ns_per_entry"] = round(res["sparse_kernel_ms"] * 1e6 / max(1, si.entry_ct), 4)
    sparse_counts = sp.sample_counts()
    sp.close()
    free = torch.cuda.mem_get_info()[0]
    if si.dense_bytes < 0.8 * free:
        t = time.perf_counter()
        ds = L.Dataset.open(prefix + ".pgen")
        res["dense_open_s"] = round(time.perf_counter() - t, 2)
        res["dense_kernel_ms"] = round(kernel_ms(ds), 3)
        assert np.array_equal(ds.sample_counts(), sparse_counts), "sparse and dense sample counts differ"
        ds.close()
    else:
        res["dense_open_s"] = None
        res["dense_kernel_ms"] = None
        res["dense_note"] = f"dense form ({si.dense_bytes / 1e9:.0f} GB) exceeds the device's free memory"
    L.trim_device_cache()
    # end to end: the first query opens (and caches) the dataset, the next ones are the scan alone
    for key, settings in (("query_dense", None), ("query_sparse", {"plinking_sample_counts_sparse": True})):
        if key == "query_dense" and res["dense_open_s"] is None:
            res[key + "_first_s"] = res[key + "_s"] = None
            continue
        t = time.perf_counter()
        F.query("read_pfile", prefix, orient="sample", genotypes="counts", threads=8, settings=settings, drain=True)
        res[key + "_first_s"] = round(time.perf_counter() - t, 3)
        res[key + "_s"] = round(_median_ms(lambda: F.query("read_pfile", prefix, orient="sample", genotypes="counts",
                                                           threads=8, settings=settings, drain=True), reps) / 1e3, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ref,biobank")
    ap.add_argument("--dir", default="/tmp/sparse_bench")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        need = shape["m"] * shape["n"] * 2 * shape["rate"] * 3.5  # file bytes, roughly
        free = shutil.disk_usage(args.dir).free
        if free < 2 * need:
            print(json.dumps({"shape": name, "skipped": f"needs ~{2 * need / 1e9:.1f} GB of disk, {free / 1e9:.1f} free"}))
            continue
        print(json.dumps(bench_shape(name, shape, args.dir, args.reps)), flush=True)


if __name__ == "__main__":
    main()
