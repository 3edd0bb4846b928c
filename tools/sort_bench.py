#!/usr/bin/env python3
"""sort_bench.py — spz.sort_spz (Morton order) on 10 M SH3 points, i.i.d. and clustered-then-shuffled.

For each cloud a seeded file is written with save_spz; then, after a warm-up call of each, every case is timed --reps
times in THIS process (run it in a fresh one):
  sort     spz.sort_spz(in, out), file -> file
  naive    load_spz(in) -> the Morton order of the loaded positions with numpy (integers = p * 2^fb, exact) -> permute
           the arrays -> save_spz(out); the two outputs' streams are compared byte for byte
  device   spz_amd.device.morton_order and subset on a resident stream, event-timed
It also reports the gzip size of the unsorted and the sorted stream, save_spz's time for the unsorted and the sorted
cloud (the device deflate's speed depends on the data), and the median chunk-256 bounding-box volume as a fraction
of the scene's (spz_amd.device.chunk_bounds) before and after.  Prints one JSON line (--out: also writes it).

--trace CSV: instead, summarise a `rocprofv3 --kernel-trace` kernel_trace.csv of a `--reps 1` run: each sort kernel's
dispatches in order, with their algorithmic bytes and the rate they imply (n = --points).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FIELDS = ("positions", "scales", "rotations", "alphas", "colors", "sh")
PER = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3}
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}
COPY_CEILING = 6.3e12  # B/s, device-to-device copy on one MI355X


def morton_order_np(ints):
    """np.lexsort of the 72-bit key of (N, 3) signed 24-bit integers (tests/test_sort_host.py's restatement)."""
    u = (ints.astype(np.int64) & 0xFFFFFF).astype(np.uint64) ^ np.uint64(0x800000)
    hi = np.zeros(u.shape[0], np.uint64)
    lo = np.zeros(u.shape[0], np.uint64)
    for b in range(24):
        for a in range(3):
            k = 3 * b + a
            bit = (u[:, a] >> np.uint64(b)) & np.uint64(1)
            if k < 48:
                lo |= bit << np.uint64(k)
            else:
                hi |= bit << np.uint64(k - 48)
    return np.lexsort((lo, hi))


def naive(spz, src, dst):
    c = spz.load_spz(src)
    n = c.num_points
    p = np.asarray(c.positions).reshape(n, 3)
    order = morton_order_np(np.rint(p.astype(np.float64) * 4096.0).astype(np.int64))  # save_spz's 12 fractional bits
    g = spz.GaussianCloud()
    g.sh_degree = c.sh_degree
    for k, w in PER.items():
        setattr(g, k, np.asarray(getattr(c, k)).reshape(n, w)[order].reshape(-1))
    g.sh = np.asarray(c.sh).reshape(n, -1)[order].reshape(-1)
    spz.save_spz(g, spz.PackOptions(), dst)


def median_ms(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 2), [round(x, 2) for x in t]


def volume_fraction(D, st, hdr, chunk=256):
    b = D.chunk_bounds(st, hdr, chunk=chunk).cpu().numpy().astype(np.float64)
    ext = b[:, 1, :] - b[:, 0, :]
    scene = (b[:, 1, :].max(axis=0) - b[:, 0, :].min(axis=0)).prod()
    return float(np.median(ext.prod(axis=1)) / scene)


def bench_cloud(spz, label, cloud, n, deg, reps, tmp, device_only=False):
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, cloud[k])
    src, out, nav = (os.path.join(tmp, f"{label}_{s}.spz") for s in ("in", "sorted", "naive"))
    assert spz.save_spz(g, spz.PackOptions(), src)
    r = {"cloud": label}
    spz.sort_spz(src, out)
    with open(src, "rb") as f:
        raw = zlib.decompress(f.read(), 31)
    if not device_only:
        host_cases(spz, g, src, out, nav, reps, r)
    r.update(device_cases(raw, reps))
    return r


def host_cases(spz, g, src, out, nav, reps, r):
    naive(spz, src, nav)
    r["sort_spz_ms"], r["sort_spz_laps_ms"] = median_ms(lambda: spz.sort_spz(src, out), reps)
    r["naive_ms"], r["naive_laps_ms"] = median_ms(lambda: naive(spz, src, nav), reps)
    with open(out, "rb") as f:
        s_sort = zlib.decompress(f.read(), 31)
    with open(nav, "rb") as f:
        s_naive = zlib.decompress(f.read(), 31)
    r["outputs_differ_bytes"] = int(np.count_nonzero(np.frombuffer(s_sort, np.uint8) != np.frombuffer(s_naive, np.uint8))) \
        if len(s_sort) == len(s_naive) else f"sizes {len(s_sort)} != {len(s_naive)}"
    r["gzip_bytes_unsorted"] = os.path.getsize(src)
    r["gzip_bytes_sorted"] = os.path.getsize(out)
    # save_spz of the sorted cloud against the unsorted one
    gs = spz.load_spz(out)
    po = spz.PackOptions()
    spz.save_spz(g, po, src)
    spz.save_spz(gs, po, out)
    r["save_spz_unsorted_ms"], _ = median_ms(lambda: spz.save_spz(g, po, src), reps)
    r["save_spz_sorted_ms"], _ = median_ms(lambda: spz.save_spz(gs, po, out), reps)


def device_cases(raw, reps):
    """morton_order and subset on a resident stream, event-timed; the chunk-256 volume fractions."""
    import torch
    from spz_amd import abi, device as D
    r = {}
    st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    hdr = abi.peek_header(raw)[1]
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    order = D.morton_order(st, hdr)
    D.subset(st, hdr, order)
    t_order, t_subset = [], []
    for _ in range(max(reps, 5)):
        e[0].record()
        order = D.morton_order(st, hdr)
        e[1].record()
        D.subset(st, hdr, order)
        e[2].record()
        torch.cuda.synchronize()
        t_order.append(e[0].elapsed_time(e[1]))
        t_subset.append(e[1].elapsed_time(e[2]))
    r["device_morton_order_ms"] = round(statistics.median(t_order), 3)
    r["device_subset_ms"] = round(statistics.median(t_subset), 3)
    sorted_st = D.subset(st, hdr, order)
    r["chunk256_volume_fraction_unsorted"] = volume_fraction(D, st, hdr)
    r["chunk256_volume_fraction_sorted"] = volume_fraction(D, sorted_st, hdr)
    return r


def kernel_bytes(name, carry_planes, n, bpp, first):
    """Algorithmic bytes of one dispatch at n points (bpp: stream bytes per point)."""
    tiles = (n + 2047) // 2048
    if name == "spz_morton_key_kernel":
        return 9 * n + 12 * n
    if name == "spz_radix_hist_kernel":
        return 4 * n + 4 * 256 * tiles
    if name == "spz_radix_scan_kernel":
        return 2 * 4 * 256 * tiles
    if name == "spz_radix_scatter_kernel":
        # digit plane + index in (none on the first pass), index + carried planes out, carried planes in
        return 4 * n + (0 if first else 4 * n) + 4 * n + 2 * 4 * n * carry_planes + 4 * 256 * tiles
    if name == "spz_subset_kernel":
        return 2 * bpp * n + 4 * n
    return None


def trace_summary(path, n, bpp):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            k = r["Kernel_Name"].split("(")[0].split("::")[-1].replace("void ", "").strip()
            if k.startswith(("spz_morton", "spz_radix", "spz_subset", "spz_float_key", "spz_chunk")):
                rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    lines, q = [], 0
    carry = [3, 3, 3, 2, 2, 2, 2, 1, 0]   # key planes each Morton pass moves (spz_sort.hip radix_passes)
    for _, k, us in rows:
        if k == "spz_morton_key_kernel":
            q = 0
        label = k
        b = None
        if k == "spz_radix_scatter_kernel":
            label = f"{k} pass {q}"
            b = kernel_bytes(k, carry[q % 9], n, bpp, q == 0)
            q += 1
        else:
            b = kernel_bytes(k, 0, n, bpp, False)
        rate = f"{b / (us * 1e-6) / 1e12:5.2f} TB/s ({b / (us * 1e-6) / COPY_CEILING * 100:3.0f} % of copy)" if b else ""
        lines.append(f"{label:36s} {us:9.1f} us  {rate}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--device-only", action="store_true", help="skip the file-to-file and save_spz cases (trace runs)")
    a = ap.parse_args()
    if a.trace:
        bpp = 9 + 1 + 3 + 3 + 4 + 3 * SH_DIM[a.sh_degree]
        print(trace_summary(a.trace, a.points, bpp))
        return
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    res = {"points": a.points, "sh_degree": a.sh_degree, "reps": a.reps, "device_only": a.device_only, "clouds": []}
    with tempfile.TemporaryDirectory() as tmp:
        for label, make in (("iid", make_cloud_numpy), ("clustered_shuffled", make_cloud_clustered)):
            c = make(a.points, a.sh_degree, 2026)
            res["clouds"].append(bench_cloud(spz, label, c, a.points, a.sh_degree, a.reps, tmp,
                                             a.device_only))
            del c
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
