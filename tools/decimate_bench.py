#!/usr/bin/env python3
"""decimate_bench.py — spz.decimate_spz on 10 M SH3 points, i.i.d. (make_cloud_numpy) and clustered
(make_cloud_clustered), at target_points 1 M and 100 k.

For each cloud a seeded file is written with save_spz; then, after a warm-up call of each, every case is timed --reps
times in THIS process (run it in a fresh one):
  decimate  spz.decimate_spz(in, out, target_points=T), file -> file
  numpy     load_spz(in) -> the same contract restated with vectorised numpy in float64 (Morton order, cells at the
            chosen level, moments by np.add.reduceat, batched eigh) -> save_spz(out)
Prints one JSON line (--out: also writes it).

--trace FILE: instead, summarise a `rocprofv3 --kernel-trace` run of `--reps 1 --skip-numpy` (its kernel_trace.csv or
rocpd .db): per kernel of the decimation (and the sort and subset it runs first), the dispatch count and the median /
total duration, and per stage the time of one decimation (the run makes 8 calls: 2 clouds x 2 targets x warm-up + 1).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sort_bench import FIELDS, SH_DIM, median_ms, morton_order_np  # noqa: E402


def numpy_route(spz, src, dst, target):
    """load_spz -> the decimation contract in vectorised float64 numpy -> save_spz.  Returns the level."""
    c = spz.load_spz(src)
    n, deg = c.num_points, c.sh_degree
    fb = 12  # save_spz's fractional bits
    ints = np.rint(np.asarray(c.positions, np.float64).reshape(n, 3) * 2.0 ** fb).astype(np.int64)
    order = morton_order_np(ints)
    u = ((ints[order] & 0xFFFFFF) ^ 0x800000).astype(np.int64)
    x = np.bitwise_or.reduce(u[1:] ^ u[:-1], axis=1)
    bins = np.where(x > 0, np.floor(np.log2(np.maximum(x, 1))).astype(np.int64), 24)
    hist = np.bincount(bins, minlength=25)
    counts = [1 + int(hist[L:24].sum()) for L in range(25)]
    level = next((L for L in range(25) if counts[L] <= target), 24)
    flag = np.ones(n, bool)
    flag[1:] = np.any((u[1:] >> level) != (u[:-1] >> level), axis=1)
    starts = np.flatnonzero(flag)
    seg = np.cumsum(flag) - 1
    origin = (u[starts] >> level) << level
    ls = np.asarray(c.scales, np.float64).reshape(n, 3)[order]
    q = np.asarray(c.rotations, np.float64).reshape(n, 4)[order]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    alpha = 1.0 / (1.0 + np.exp(-np.asarray(c.alphas, np.float64)[order]))
    w = alpha * np.exp(ls.sum(1))
    W = np.add.reduceat(w, starts)
    zero = W == 0.0
    w = np.where(zero[seg], 1.0, w)
    Wn = np.add.reduceat(w, starts)
    p = (u - origin[seg]).astype(np.float64) * 2.0 ** -fb
    mu = np.add.reduceat(w[:, None] * p, starts) / Wn[:, None]
    d = p - mu[seg]
    xq, yq, zq, wq = q.T
    R = np.stack([np.stack([1 - 2 * (yq * yq + zq * zq), 2 * (xq * yq - wq * zq), 2 * (xq * zq + wq * yq)], -1),
                  np.stack([2 * (xq * yq + wq * zq), 1 - 2 * (xq * xq + zq * zq), 2 * (yq * zq - wq * xq)], -1),
                  np.stack([2 * (xq * zq - wq * yq), 2 * (yq * zq + wq * xq), 1 - 2 * (xq * xq + yq * yq)], -1)], -2)
    own = np.einsum("kab,kb,kcb->kac", R, np.exp(2 * ls), R)
    cov = np.add.reduceat(w[:, None, None] * (own + d[:, :, None] * d[:, None, :]), starts) / Wn[:, None, None]
    del R, own, d
    lam, V = np.linalg.eigh(cov)
    lam, V = np.maximum(lam[:, ::-1], np.exp(-20.0)), V[:, :, ::-1].copy()
    V[np.linalg.det(V) < 0, :, 2] *= -1
    out_ls = 0.5 * np.log(lam)
    # rotation matrix -> quaternion, branch-free (magnitudes from the diagonal, signs from the skew part)
    m00, m11, m22 = V[:, 0, 0], V[:, 1, 1], V[:, 2, 2]
    qw = 0.5 * np.sqrt(np.maximum(0.0, 1 + m00 + m11 + m22))
    qx = np.copysign(0.5 * np.sqrt(np.maximum(0.0, 1 + m00 - m11 - m22)), V[:, 2, 1] - V[:, 1, 2])
    qy = np.copysign(0.5 * np.sqrt(np.maximum(0.0, 1 - m00 + m11 - m22)), V[:, 0, 2] - V[:, 2, 0])
    qz = np.copysign(0.5 * np.sqrt(np.maximum(0.0, 1 - m00 - m11 + m22)), V[:, 1, 0] - V[:, 0, 1])
    a_out = np.where(zero, 0.0, np.minimum(1.0, W / np.exp(out_ls.sum(1))))
    a_out = np.clip(a_out, 1e-6, 1 - 1e-6)
    colors = np.add.reduceat(w[:, None] * np.asarray(c.colors, np.float64).reshape(n, 3)[order], starts) / Wn[:, None]
    dim = SH_DIM[deg]
    g = spz.GaussianCloud()
    g.sh_degree = deg
    if dim:
        sh = np.asarray(c.sh, np.float64).reshape(n, 3 * dim)[order]
        g.sh = (np.add.reduceat(w[:, None] * sh, starts) / Wn[:, None]).astype(np.float32).reshape(-1)
    pos = (origin - 0x800000 + np.clip(np.rint(mu * 2.0 ** fb), 0, (1 << level) - 1)) * 2.0 ** -fb
    g.positions = pos.astype(np.float32).reshape(-1)
    g.scales = out_ls.astype(np.float32).reshape(-1)
    g.rotations = np.stack([qx, qy, qz, qw], 1).astype(np.float32).reshape(-1)
    g.alphas = np.log(a_out / (1 - a_out)).astype(np.float32)
    g.colors = colors.astype(np.float32).reshape(-1)
    assert spz.save_spz(g, spz.PackOptions(), dst)
    return level


def bench_cloud(spz, label, cloud, deg, targets, reps, tmp, skip_numpy=False):
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, cloud[k])
    src, out, nav = (os.path.join(tmp, f"{label}_{s}.spz") for s in ("in", "dec", "numpy"))
    assert spz.save_spz(g, spz.PackOptions(), src)
    rows = []
    for t in targets:
        r = {"cloud": label, "target_points": t}
        level, points = spz.decimate_spz(src, out, target_points=t)
        r["level"], r["points"] = level, points
        r["decimate_spz_ms"], r["decimate_spz_laps_ms"] = median_ms(lambda: spz.decimate_spz(src, out, target_points=t),
                                                                    reps)
        if not skip_numpy:
            r["numpy_level"] = numpy_route(spz, src, nav, t)
            r["numpy_ms"], r["numpy_laps_ms"] = median_ms(lambda: numpy_route(spz, src, nav, t), max(1, reps // 2))
        r["gzip_bytes_in"], r["gzip_bytes_out"] = os.path.getsize(src), os.path.getsize(out)
        rows.append(r)
    return rows


PREFIXES = ("spz_dec_", "spz_morton", "spz_radix", "spz_subset")
STAGES = (("sort (Morton key + 9 radix passes)", ("spz_morton", "spz_radix")), ("subset (sorted stream)", ("spz_subset",)),
          ("level counts", ("spz_dec_hist", "spz_dec_levels")),
          ("cell ids (flags, scan, apply)", ("spz_dec_flags", "spz_dec_scan", "spz_dec_apply")),
          ("moment reduction (wave tiles)", ("spz_dec_reduce",)), ("crossing cells (combine)", ("spz_dec_combine",)))


def trace_rows(path):
    """(name, duration us) of every dispatch of a kernel trace: a rocprofv3 kernel_trace.csv or rocpd .db."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as c:
            rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    else:
        with open(path) as f:
            rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(f)]
    out = []
    for name, us in rows:
        k = name.split("(")[0].replace("void ", "").strip()
        k = k.split("spz_amd_detail::")[-1]
        if k.startswith(PREFIXES):
            out.append((k, us))
    return out


def trace_summary(path, calls):
    """Per kernel: dispatches, median and total; per stage: the total over `calls` decimations, per decimation."""
    by = {}
    for k, us in trace_rows(path):
        by.setdefault(k, []).append(us)
    lines = [f"{'kernel':48s} {'calls':>6s} {'median us':>10s} {'total us':>10s}"]
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{k[:48]:48s} {len(v):6d} {statistics.median(v):10.1f} {sum(v):10.1f}")
    lines.append(f"\nper decimation (total / {calls} calls):")
    for label, pre in STAGES:
        t = sum(sum(v) for k, v in by.items() if k.startswith(pre))
        lines.append(f"  {label:40s} {t / calls / 1e3:8.3f} ms")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--targets", default="1000000,100000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="a kernel_trace.csv or rocpd .db to summarise")
    ap.add_argument("--trace-calls", type=int, default=8, help="decimate_spz calls in the traced run (--reps 1: 8)")
    ap.add_argument("--skip-numpy", action="store_true", help="time decimate_spz only (trace runs)")
    a = ap.parse_args()
    if a.trace:
        print(trace_summary(a.trace, a.trace_calls))
        return
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    targets = [int(t) for t in a.targets.split(",")]
    res = {"points": a.points, "sh_degree": a.sh_degree, "reps": a.reps, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for label, make in (("iid", make_cloud_numpy), ("clustered", make_cloud_clustered)):
            c = make(a.points, a.sh_degree, 2026)
            res["cases"] += bench_cloud(spz, label, c, a.sh_degree, targets, a.reps, tmp, a.skip_numpy)
            del c
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
