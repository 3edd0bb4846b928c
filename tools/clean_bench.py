#!/usr/bin/env python3
"""clean_bench.py — spz.clean_spz on 10 M SH3 points, i.i.d. (make_cloud_numpy) and clustered (make_cloud_clustered),
with the statistical rule (k = 20, std_ratio = 2) and with the radius rule (radius 0.1, min_neighbors 4).

For each cloud a seeded file is written with save_spz; then, after a warm-up call of each, every case is timed --reps
times in THIS process (run it in a fresh one):
  clean   spz.clean_spz(in, out, ...), file -> file
  scipy   load_spz(in) -> scipy cKDTree(workers=16) on the stored integers (k + 1 nearest, or the ball counts) -> the
          same scores, threshold and mask -> save_spz(out) of the kept points (one timed run after a warm-up).  Skipped,
          and marked so, when scipy is missing.
Prints one JSON line (--out: also writes it).

--trace FILE: instead, summarise a `rocprofv3 --kernel-trace` run of `--reps 1 --skip-cpu` (its kernel_trace.csv or
rocpd .db): per kernel of the clean (and the sort, select and subset it runs), the dispatch count and the median / total
duration, and per stage the time of one clean (the run makes 8 calls: 2 clouds x 2 rules x warm-up + 1).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from sort_bench import FIELDS, median_ms  # noqa: E402

CASES = (("k20", dict(k=20, std_ratio=2.0)), ("radius", dict(radius=0.1, min_neighbors=4)))


def cpu_route(spz, src, dst, k=None, std_ratio=2.0, radius=None, min_neighbors=None):
    """load_spz -> cKDTree on the stored integers -> the contract's mask -> save_spz of the kept points.  Returns the
    kept count."""
    from scipy.spatial import cKDTree
    c = spz.load_spz(src)
    n = c.num_points
    fb = 12  # save_spz's fractional bits
    P = np.rint(np.asarray(c.positions, np.float64).reshape(n, 3) * 2.0 ** fb)
    tree = cKDTree(P)
    if k is not None:
        d, _ = tree.query(P, k=k + 1, workers=16)
        scores = d[:, 1:].sum(axis=1) / k * 2.0 ** -fb
        thr = scores.mean() + std_ratio * scores.std(ddof=1)
        keep = scores <= thr
    else:
        r = radius * 2.0 ** fb
        counts = tree.query_ball_point(P, r, workers=16, return_length=True) - 1
        keep = counts >= min_neighbors
    g = spz.GaussianCloud()
    g.sh_degree = c.sh_degree
    for f in FIELDS:
        a = np.asarray(getattr(c, f))
        if a.size:
            setattr(g, f, a.reshape(n, -1)[keep].reshape(-1))
    assert spz.save_spz(g, spz.PackOptions(), dst)
    return int(keep.sum())


def bench_cloud(spz, label, cloud, deg, reps, tmp, skip_cpu=False):
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for f in FIELDS:
        setattr(g, f, cloud[f])
    src, out, nav = (os.path.join(tmp, f"{label}_{s}.spz") for s in ("in", "clean", "cpu"))
    assert spz.save_spz(g, spz.PackOptions(), src)
    try:
        import scipy.spatial  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    rows = []
    for name, kw in CASES:
        r = {"cloud": label, "rule": name, **kw}
        r["kept"] = spz.clean_spz(src, out, **kw)
        r["clean_spz_ms"], r["clean_spz_laps_ms"] = median_ms(lambda: spz.clean_spz(src, out, **kw), reps)
        if skip_cpu:
            r["cpu"] = "skipped"
        elif not have_scipy:
            r["cpu"] = "skipped: scipy is not installed"
        else:
            r["cpu_kept"] = cpu_route(spz, src, nav, **kw)
            r["cpu_ms"], r["cpu_laps_ms"] = median_ms(lambda: cpu_route(spz, src, nav, **kw), 1)
        r["gzip_bytes_in"], r["gzip_bytes_out"] = os.path.getsize(src), os.path.getsize(out)
        rows.append(r)
    return rows


PREFIXES = ("spz_clean_", "spz_morton", "spz_radix", "spz_subset", "spz_select", "spz_compact")
STAGES = (("sort (Morton key + 9 radix passes)", ("spz_morton_key", "spz_radix")),
          ("gather + start levels", ("spz_morton_gather", "spz_clean_level")),
          ("k-NN search", ("spz_clean_search",)), ("radius search", ("spz_clean_radius",)),
          ("threshold + mask", ("spz_clean_sum", "spz_clean_stats", "spz_clean_mask")),
          ("select + subset", ("spz_select", "spz_compact", "spz_subset")))


def trace_rows(path):
    """(name, duration us) of every dispatch of a kernel trace: a rocprofv3 kernel_trace.csv or rocpd .db."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as c:
            rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    else:
        with open(path) as f:
            rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                    for r in csv.DictReader(f)]
    out = []
    for name, us in rows:
        k = name.split("(")[0].replace("void ", "").strip().split("spz_amd_detail::")[-1]
        if k.startswith(PREFIXES):
            out.append((k, us))
    return out


def trace_summary(path, calls):
    by = {}
    for k, us in trace_rows(path):
        by.setdefault(k, []).append(us)
    lines = [f"{'kernel':48s} {'calls':>6s} {'median us':>10s} {'total us':>10s}"]
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{k[:48]:48s} {len(v):6d} {statistics.median(v):10.1f} {sum(v):10.1f}")
    lines.append(f"\nper clean (total / {calls} calls):")
    for label, pre in STAGES:
        t = sum(sum(v) for k, v in by.items() if k.startswith(pre))
        lines.append(f"  {label:40s} {t / calls / 1e3:8.3f} ms")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="a kernel_trace.csv or rocpd .db to summarise")
    ap.add_argument("--trace-calls", type=int, default=8, help="clean_spz calls in the traced run (--reps 1: 8)")
    ap.add_argument("--skip-cpu", action="store_true", help="time clean_spz only (trace runs)")
    a = ap.parse_args()
    if a.trace:
        print(trace_summary(a.trace, a.trace_calls))
        return
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    res = {"points": a.points, "sh_degree": a.sh_degree, "reps": a.reps, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for label, make in (("iid", make_cloud_numpy), ("clustered", make_cloud_clustered)):
            c = make(a.points, a.sh_degree, 2026)
            res["cases"] += bench_cloud(spz, label, c, a.sh_degree, a.reps, tmp, a.skip_cpu)
            del c
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
