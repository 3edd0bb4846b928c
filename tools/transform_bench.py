#!/usr/bin/env python3
"""transform_bench.py — file -> file spz.transform_spz against the naive route (load_spz -> numpy -> save_spz).

A seeded 10 M-point SH3 file is written with save_spz; then, after a warm-up call of each, every route is timed --reps
times in THIS process (run it in a fresh one):
  transform  spz.transform_spz(in, out, rotation, translation, scale), with the per-stage laps spz::transformSpz prints
             under SPZ_AMD_TRANSFORM_TIMING=1 (inflate, kernel, download, gzip, write; from a child process)
  naive      load_spz(in) -> the numpy float32 restatement of tests/test_transform_host.py (the same arithmetic, fed
             the library's parameter block) -> save_spz(out)
Both routes write the same bytes (checked: `same_bytes`).  Prints one JSON line.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/transform_bench.py ...` run.
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

FIELDS = ("positions", "scales", "rotations", "alphas", "colors", "sh")
TRANSFORM = dict(rotation=[0.3, -0.5, 0.2, 0.7], translation=[1.5, -2.0, 0.25], scale=1.7)


def naive(spz, src, dst):
    from test_transform_host import apply_transform, params
    c = spz.load_spz(src)
    cloud = {k: np.asarray(getattr(c, k)) for k in FIELDS}
    t = apply_transform(cloud, params(**TRANSFORM), c.sh_degree)
    g = spz.GaussianCloud()
    g.sh_degree = c.sh_degree
    g.antialiased = c.antialiased
    for k in FIELDS:
        setattr(g, k, t[k])
    assert spz.save_spz(g, spz.PackOptions(), dst)


def child_laps(src, dst):
    """One transform_spz in a child process with the stage laps on; returns {stage: ms} of the second (warm) call."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import spz_amd.spz as spz; "
            f"kw = {TRANSFORM!r}; spz.transform_spz({src!r}, {dst!r}, **kw); spz.transform_spz({src!r}, {dst!r}, **kw)")
    env = dict(os.environ, SPZ_AMD_TRANSFORM_TIMING="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, check=True)
    laps = {}
    for m in re.finditer(r"\[transformSpz\] (\w+)\s+([0-9.]+) ms", r.stderr):
        laps[m.group(1)] = float(m.group(2))
    return laps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-laps", action="store_true", help="skip the child process that collects the stage laps")
    a = ap.parse_args()
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_numpy

    work = a.dir or tempfile.mkdtemp(prefix="transform_bench_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "in.spz")
    dst = {"transform": os.path.join(work, "out.spz"), "naive": os.path.join(work, "naive.spz")}
    n, deg = a.points, 3
    c = make_cloud_numpy(n, deg, 2024)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    assert spz.save_spz(g, spz.PackOptions(), src)
    del g, c
    out = {"points": n, "sh_degree": deg, "params": TRANSFORM, "input_bytes": os.path.getsize(src)}
    for route in ("transform", "naive"):
        times = []
        for rep in range(a.reps + 1):  # the first call is the warm-up
            t0 = time.perf_counter()
            if route == "transform":
                spz.transform_spz(src, dst[route], **TRANSFORM)
            else:
                naive(spz, src, dst[route])
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
        out[route] = {"s_min": round(min(times), 4), "s_median": round(float(np.median(times)), 4),
                      "output_bytes": os.path.getsize(dst[route])}
    out["speedup_median"] = round(out["naive"]["s_median"] / out["transform"]["s_median"], 2)
    with open(dst["transform"], "rb") as f1, open(dst["naive"], "rb") as f2:
        out["same_bytes"] = f1.read() == f2.read()
    if not a.no_laps:
        out["transform_laps_ms"] = child_laps(src, dst["transform"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
