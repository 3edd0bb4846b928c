#!/usr/bin/env python3
"""filter_bench.py — file -> file spz.filter_spz against the naive route (load_spz -> numpy indexing -> save_spz).

A seeded 10 M-point SH3 file is written with save_spz; then, after a warm-up call of each, every case is timed
--reps times in THIS process (run it in a fresh one):
  filter   spz.filter_spz(in, out, ...), with the per-stage laps spz::filterSpz prints under SPZ_AMD_FILTER_TIMING=1
           (inflate, select, subset, download, gzip, write; collected from a child process, whose stderr carries them)
  naive    load_spz(in) -> the same selection with numpy on the float arrays -> save_spz(out)
Cases: a seeded 50 % mask, a box (the central 60 % on every axis), SH3 -> SH0 (every point).  Prints one JSON line.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/filter_bench.py ...` run.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FIELDS = ("positions", "scales", "rotations", "alphas", "colors", "sh")
PER = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3}
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}


def cases(n, positions):
    rng = np.random.default_rng(50)
    p = positions.reshape(n, 3)
    lo, hi = np.quantile(p, 0.2, axis=0).astype(np.float32), np.quantile(p, 0.8, axis=0).astype(np.float32)
    return {
        "mask50": dict(mask=rng.random(n) < 0.5),
        "box": dict(box=np.stack([lo, hi])),
        "sh3_to_sh0": dict(sh_degree=0),
    }


def naive(spz, src, dst, kw):
    c = spz.load_spz(src)
    n = c.num_points
    p = np.asarray(c.positions).reshape(n, 3)
    if "mask" in kw:
        idx = np.nonzero(kw["mask"])[0]
    elif "box" in kw:
        b = kw["box"]
        idx = np.nonzero(np.all((b[0] <= p) & (p <= b[1]), axis=1))[0]
    else:
        idx = np.arange(n)
    deg = kw.get("sh_degree", c.sh_degree)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k, w in PER.items():
        setattr(g, k, np.asarray(getattr(c, k)).reshape(n, w)[idx].reshape(-1))
    g.sh = np.asarray(c.sh).reshape(n, SH_DIM[c.sh_degree], 3)[idx, :SH_DIM[deg], :].reshape(-1)
    spz.save_spz(g, spz.PackOptions(), dst)
    return idx.size


def child_laps(src, dst, case):
    """One filter_spz in a child process with the stage laps on; returns {stage: ms}."""
    code = (f"import sys, numpy as np; sys.path.insert(0, {ROOT!r}); import spz_amd.spz as spz; "
            f"from tools.filter_bench import cases; c = spz.load_spz({src!r}); "
            f"kw = cases(c.num_points, np.asarray(c.positions))[{case!r}]; del c; "
            f"spz.filter_spz({src!r}, {dst!r}, **kw); spz.filter_spz({src!r}, {dst!r}, **kw)")
    env = dict(os.environ, SPZ_AMD_FILTER_TIMING="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, check=True)
    laps = {}
    for m in re.finditer(r"\[filterSpz\] (\w+)\s+([0-9.]+) ms", r.stderr):
        laps[m.group(1)] = float(m.group(2))   # the second call's laps overwrite the first's (warm)
    return laps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-laps", action="store_true", help="skip the child processes that collect the stage laps")
    a = ap.parse_args()
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_numpy

    work = a.dir or tempfile.mkdtemp(prefix="filter_bench_")
    os.makedirs(work, exist_ok=True)
    src, dst = os.path.join(work, "in.spz"), os.path.join(work, "out.spz")
    n, deg = a.points, 3
    c = make_cloud_numpy(n, deg, 2024)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    po = spz.PackOptions()
    po.from_coord = spz.RDF
    assert spz.save_spz(g, po, src)
    cs = cases(n, np.asarray(spz.load_spz(src).positions))
    del g, c
    out = {"points": n, "sh_degree": deg, "input_bytes": os.path.getsize(src), "cases": {}}
    for name, kw in cs.items():
        row = {}
        for route in ("filter", "naive"):
            times = []
            for rep in range(a.reps + 1):  # the first call is the warm-up
                t0 = time.perf_counter()
                kept = spz.filter_spz(src, dst, **kw) if route == "filter" else naive(spz, src, dst, kw)
                dt = time.perf_counter() - t0
                if rep:
                    times.append(dt)
            row[route] = {"kept": int(kept), "s_min": round(min(times), 4), "s_median": round(float(np.median(times)), 4),
                          "output_bytes": os.path.getsize(dst)}
        row["speedup_median"] = round(row["naive"]["s_median"] / row["filter"]["s_median"], 2)
        if not a.no_laps:
            row["filter_laps_ms"] = child_laps(src, dst, name)
        out["cases"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
