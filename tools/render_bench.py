#!/usr/bin/env python3
"""render_bench.py — one 1920x1080 view of a 10 M-point SH3 clustered scene (make_cloud_clustered), rendered on the
device two ways, each timed --reps times after a warm-up in THIS process (run it in a fresh one):
  resident  spz_amd_render_host over the stream already in device memory: its per-stage wall-clock times (preprocess
            with the depth order and the count scan; tile entries with their sort and the ranges; blend)
  file      spz.render_spz(path): read + inflate + the same, file -> image in host memory
Also reports the entry count and the preprocess stage's rate over the packed stream (stream bytes / stage time: a lower
bound on the preprocess kernel's own rate, which the kernel trace gives).  Prints one JSON line (--out: also writes it).

--trace DB: instead, summarise the rocpd database of a `rocprofv3 --kernel-trace --stats -- python tools/render_bench.py
--reps 2` run: per kernel the dispatch count and the median / total duration, and per render the kernel time of every
stage (the radix passes are told apart by where they run: after the depth keys, or after the tile entries), plus the
preprocess kernel's rate over the packed stream.
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


STAGE_OF = {"spz_render_preprocess_kernel": "preprocess", "spz_float_key_kernel": "depth sort",
            "spz_render_block_sums_kernel": "count scan", "spz_render_scan_sums_kernel": "count scan",
            "spz_render_emit_kernel": "tile entries", "spz_render_pad_kernel": "tile entries",
            "spz_render_ranges_kernel": "tile ranges", "spz_render_blend_kernel": "blend"}
STAGES = ("preprocess", "depth sort", "count scan", "tile entries", "tile sort", "tile ranges", "blend")


def trace_summary(path, stream_bytes):
    import sqlite3
    with sqlite3.connect(path) as c:
        rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    by, stage, renders, phase = {}, {s: 0.0 for s in STAGES}, 0, "depth sort"
    pre = []
    for name, us in rows:
        found = re.search(r"(spz_\w+_kernel)(<[^>]*Src>)?", name)
        if found is None:
            continue
        base = found.group(1)
        k = base + ("<packed>" if "PackedSrc" in name else "<float>" if "FloatSrc" in name else "")
        if not (base.startswith("spz_render_") or base.startswith("spz_radix") or base == "spz_float_key_kernel"):
            continue
        by.setdefault(k, []).append(us)
        if base == "spz_render_preprocess_kernel":
            renders += 1
            pre.append(us)
        if base == "spz_float_key_kernel":
            phase = "depth sort"
        elif base == "spz_render_pad_kernel":
            phase = "tile sort"
        stage[STAGE_OF.get(base, phase)] += us
    lines = [f"{'kernel':52s} {'calls':>6s} {'median us':>10s} {'total us':>11s}"]
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{k:52s} {len(v):6d} {statistics.median(v):10.1f} {sum(v):11.1f}")
    lines.append("")
    lines.append(f"per render (total / {renders} renders):")
    for s in STAGES:
        lines.append(f"  {s:40s} {stage[s] / max(renders, 1) / 1e3:9.3f} ms")
    if pre:
        lines.append(f"  preprocess kernel over the {stream_bytes} B packed stream: "
                     f"{stream_bytes / (statistics.median(pre) * 1e-6) / 1e9:.0f} GB/s (median dispatch)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="a rocpd .db of a traced run to summarise")
    ap.add_argument("--stream-bytes", type=int, default=650000016, help="with --trace: the packed stream's size")
    a = ap.parse_args()
    if a.trace:
        print(trace_summary(a.trace, a.stream_bytes))
        return

    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg = a.points, 3
    c = make_cloud_clustered(n, deg, 1234)
    stream = D.encode(D.to_device(c, dev), n, deg, False, abi.RUB, 3)
    torch.cuda.synchronize()
    raw = stream.cpu().numpy().tobytes()
    rc, h = abi.peek_header(raw)
    abi.check(rc, "peek_header")
    W, H = a.width, a.height
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    m = spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    p = abi.render_params(m, fy, fy, W / 2, H / 2, W, H)

    img = np.empty((H, W, 4), np.float32)
    ent = C.c_uint64(0)
    ms = (C.c_float * 3)()
    stages = {"preprocess": [], "entries_and_sort": [], "blend": [], "total": []}
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        rc = L.spz_amd_render_host(stream.data_ptr(), stream.numel(), C.byref(h), C.byref(p), 0, img.ctypes.data,
                                   C.byref(ent), ms)
        dt = (time.perf_counter() - t0) * 1e3
        abi.check(rc, "spz_amd_render_host")
        if r:
            for k, v in zip(("preprocess", "entries_and_sort", "blend"), ms):
                stages[k].append(float(v))
            stages["total"].append(dt)

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "scene.spz")
        co = zlib.compressobj(6, zlib.DEFLATED, 16 + 15)
        with open(path, "wb") as f:
            f.write(co.compress(raw) + co.flush())
        files = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            got = spz.render_spz(path, world_to_camera=m, width=W, height=H, fx=fy, fy=fy, cx=W / 2, cy=H / 2)
            if r:
                files.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(got.view(np.uint32), img.view(np.uint32)))
    med = {k: round(statistics.median(v), 3) for k, v in stages.items()}
    out = {
        "tool": "render_bench", "points": n, "sh_degree": deg, "width": W, "height": H, "reps": a.reps,
        "stream_bytes": len(raw), "entries": int(ent.value),
        "resident_median_ms": med,
        "file_to_image_median_ms": round(statistics.median(files), 3),
        "preprocess_stage_gbps": round(len(raw) / (med["preprocess"] * 1e-3) / 1e9, 1),
        "file_equals_resident": same,
        "coverage": round(float((img[..., 3] > 0).mean()), 4),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
