#!/usr/bin/env python3
"""align_bench.py — spz.align_spz on a synthetic clustered SH3 scene (make_cloud_clustered) against its displaced,
permuted copy (0.02 rad about (1, 2, 3), translation (0.05, -0.03, 0.04)), a fixed number of steps (tolerances 0, so
both routes run the same count).

Two seeded files are written with save_spz; then, after a warm-up call of each, in THIS process (run it in a fresh one,
several times, for the spread between processes):
  align     spz.align_spz(source, target), file -> placement, --reps times
  resident  spz_amd.device.align_packed on the two streams in device memory, --reps times: the wall time and the stages
            spz_amd_align_host reports (prepare, queries, selections + moments + solves)
  knn1      spz_amd.device.knn_scores(target, k = 1), event-timed: the parent's self-query of the same walk (it sorts the
            target too; the kernels alone are compared from a trace)
  cpu       load_spz of both files -> scipy cKDTree(target) -> per step tree.query(mapped source, workers=16) and a numpy
            Umeyama solve, the same number of steps (one timed run; skipped, and marked so, when scipy is missing)
Prints one JSON line (--out: also writes it).

--trace FILE: instead, summarise a `rocprofv3 --kernel-trace` run of `--reps 1 --device-only` (its kernel_trace.csv or
rocpd .db): every dispatch of spz_align_query_kernel in order (the steps of the runs), the other align kernels, and
spz_clean_search_kernel of the knn1 call, with the time per query of both.
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

from sort_bench import FIELDS, PER, SH_DIM, median_ms  # noqa: E402

ANGLE, AXIS, SHIFT = 0.02, (1.0, 2.0, 3.0), (0.05, -0.03, 0.04)


def rotation():
    a = np.asarray(AXIS) / np.linalg.norm(AXIS)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ANGLE) * K + (1 - np.cos(ANGLE)) * (K @ K)


def displaced_copy(cloud, n, deg, seed):
    """The cloud's points moved by the known rigid map (positions only: the other fields do not take part) and permuted."""
    perm = np.random.default_rng(seed).permutation(n)
    out = {}
    for k in FIELDS:
        w = PER.get(k, SH_DIM[deg] * 3)
        a = cloud[k].reshape(n, w) if w else cloud[k]
        if k == "positions":
            a = (a.astype(np.float64) @ rotation().T + np.asarray(SHIFT)).astype(np.float32)
        out[k] = a[perm].reshape(-1) if w else a
    return out


def save(spz, cloud, deg, path):
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, cloud[k])
    assert spz.save_spz(g, spz.PackOptions(), path)


def umeyama(a, b):
    ma, mb = a.mean(axis=0), b.mean(axis=0)
    H = (b - mb).T @ (a - ma) / a.shape[0]
    U, D, Vt = np.linalg.svd(H)
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = (U * S) @ Vt
    return R, mb - R @ ma


def cpu_route(spz, src, tgt, steps):
    """What a user does today: both files to floats, a k-d tree of the target, `steps` of query + solve.  Returns the
    last step's rmse."""
    from scipy.spatial import cKDTree
    a = spz.load_spz(src)
    b = spz.load_spz(tgt)
    A = np.asarray(a.positions, np.float64).reshape(-1, 3)
    B = np.asarray(b.positions, np.float64).reshape(-1, 3)
    tree = cKDTree(B)
    R, t = np.eye(3), np.zeros(3)
    rmse = 0.0
    for _ in range(steps):
        d, j = tree.query(A @ R.T + t, workers=16)
        rmse = float(np.sqrt(np.mean(d * d)))
        R, t = umeyama(A, B[j])
    return rmse


PREFIXES = ("spz_align_", "spz_clean_search", "spz_clean_level", "spz_morton", "spz_radix")


def trace_rows(path):
    """(name, duration us) of every dispatch of a kernel trace, in start order."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as c:
            rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    else:
        with open(path) as f:
            rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"],
                           (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in csv.DictReader(f))
            rows = [(n, us) for _, n, us in rows]
    out = []
    for name, us in rows:
        k = name.split("(")[0].replace("void ", "").strip().split("spz_amd_detail::")[-1].split("<")[0]
        if k.startswith(PREFIXES):
            out.append((k, us))
    return out


def trace_summary(path, n, steps):
    rows = trace_rows(path)
    by = {}
    for k, us in rows:
        by.setdefault(k, []).append(us)
    lines = [f"{'kernel':40s} {'calls':>6s} {'median us':>10s} {'min us':>10s} {'max us':>10s} {'total us':>11s}"]
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{k[:40]:40s} {len(v):6d} {statistics.median(v):10.1f} {min(v):10.1f} {max(v):10.1f} {sum(v):11.1f}")
    q = by.get("spz_align_query_kernel", [])
    if q:
        lines.append(f"\nspz_align_query_kernel by step of a run ({steps} steps per run, {n} queries), us:")
        for r in range(0, len(q), steps):
            lines.append("  " + " ".join(f"{x:9.1f}" for x in q[r:r + steps]))
        last = statistics.median(q[r + steps - 1] for r in range(0, len(q) - steps + 1, steps))
        first = statistics.median(q[r] for r in range(0, len(q) - steps + 1, steps))
        lines.append(f"per query: first step {first * 1e3 / n:.3f} ns, last step {last * 1e3 / n:.3f} ns")
        s = by.get("spz_clean_search_kernel", [])
        if s:
            self_ns = statistics.median(s) * 1e3 / n
            lines.append(f"spz_clean_search_kernel (k = 1, the target against itself): {self_ns:.3f} ns per query; "
                         f"ratio first {first * 1e3 / n / self_ns:.2f}, last {last * 1e3 / n / self_ns:.2f}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="a kernel_trace.csv or rocpd .db to summarise")
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="the resident run and knn1 only (trace runs)")
    a = ap.parse_args()
    if a.trace:
        print(trace_summary(a.trace, a.points, a.steps))
        return
    import torch
    import zlib
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered
    n, deg = a.points, a.sh_degree
    opts = dict(max_iterations=a.steps, relative_fitness=0.0, relative_rmse=0.0)
    res = {"points": n, "sh_degree": deg, "steps": a.steps, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp:
        src, tgt = os.path.join(tmp, "source.spz"), os.path.join(tmp, "target.spz")
        c = make_cloud_clustered(n, deg, 2026)
        save(spz, c, deg, src)
        save(spz, displaced_copy(c, n, deg, 7), deg, tgt)
        del c
        res["gzip_bytes"] = [os.path.getsize(src), os.path.getsize(tgt)]
        if not a.device_only:
            r = spz.align_spz(src, tgt, **opts)   # warm-up
            res["align"] = {k: r[k] for k in ("rotation", "translation", "scale", "fitness", "inlier_rmse", "iterations")}
            res["align_spz_ms"], res["align_spz_laps_ms"] = median_ms(lambda: spz.align_spz(src, tgt, **opts), a.reps)
        streams = []
        for p in (src, tgt):
            with open(p, "rb") as f:
                raw = zlib.decompress(f.read(), 31)
            streams += [torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda"), abi.peek_header(raw)[1]]
        D.align_packed(*streams, **opts)           # warm-up
        walls, stages = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = D.align_packed(*streams, **opts)
            walls.append(round((time.perf_counter() - t0) * 1e3, 2))
            stages.append([round(x, 3) for x in r["ms"]])
        res["resident_ms"], res["resident_laps_ms"] = round(statistics.median(walls), 2), walls
        res["resident_stage_ms"] = {"prepare": statistics.median(s[0] for s in stages),
                                    "queries": statistics.median(s[1] for s in stages),
                                    "select_moments_solve": statistics.median(s[2] for s in stages), "laps": stages}
        res["query_ms_per_step"] = round(res["resident_stage_ms"]["queries"] / a.steps, 3)
        D.knn_scores(streams[2], streams[3], 1)    # warm-up
        ev, t = [torch.cuda.Event(enable_timing=True) for _ in range(2)], []
        for _ in range(a.reps):
            ev[0].record()
            D.knn_scores(streams[2], streams[3], 1)
            ev[1].record()
            torch.cuda.synchronize()
            t.append(round(ev[0].elapsed_time(ev[1]), 3))
        res["knn1_ms"], res["knn1_laps_ms"] = statistics.median(t), t
        del streams
        if a.device_only:
            pass
        elif a.skip_cpu:
            res["cpu"] = "skipped"
        else:
            try:
                import scipy.spatial  # noqa: F401
                t0 = time.perf_counter()
                res["cpu_rmse"] = cpu_route(spz, src, tgt, a.steps)
                res["cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            except ImportError:
                res["cpu"] = "skipped: scipy is not installed"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
