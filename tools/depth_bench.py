#!/usr/bin/env python3
"""depth_bench.py — the depth blend against the colour blend: one 1920x1080 view of a 10 M-point SH3 clustered scene
(render_bench.py's scene and camera) from the stream resident in device memory.

  depth  h_ms[2] of spz_amd_render_depth_host (image, depth and index all written): the depth blend step
  blend  h_ms[2] of spz_amd_render_host: the colour blend step

Both are a host clock around the one kernel, between two stream synchronisations.  A run times each --reps times after
a warm-up of both, alternating the two, in THIS process; --processes N starts N fresh processes one after another and
reports the median of their medians and the spread.  --baseline-lib PATH: the blend is timed through that
libspz_amd.so (a build of the parent commit) in processes of its own, alternating with the depth processes; without it
the blend is this build's (the same kernel source).  Prints one JSON line (--out: also writes it).
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def baseline_library(path, loader=C.CDLL):
    """The parent commit's libspz_amd.so with the one function the bench calls through it declared (abi.bind would ask
    it for functions it does not have).  loader: what opens the library."""
    from spz_amd import abi
    B = loader(path)
    B.spz_amd_render_host.restype = C.c_int
    B.spz_amd_render_host.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.Header), C.POINTER(abi.RenderParams),
                                      C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    return B


def worker(a):
    """One process: the scene, a warm-up, then the timed calls.  Prints {"depth": [...], "blend": [...], ...}."""
    import numpy as np
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered

    L = abi.load_library()  # this build: the scene's encoder, and the depth step
    B = baseline_library(a.baseline_lib) if a.baseline_lib else L
    dev = torch.device("cuda:0")
    n, deg = a.points, 3
    stream = D.encode(D.to_device(make_cloud_clustered(n, deg, 1234), dev), n, deg, False, abi.RUB, 3)
    torch.cuda.synchronize()
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    abi.check(rc, "peek_header")
    W, H = a.width, a.height
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    m = spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    p = abi.render_params(m, fy, fy, W / 2, H / 2, W, H)
    img = np.empty((H, W, 4), np.float32)
    img_d = np.empty((H, W, 4), np.float32)
    depth = np.empty((H, W, 2), np.float32)
    index = np.empty((H, W), np.uint32)
    ent = C.c_uint64(0)
    ms = (C.c_float * 3)()
    times = {"depth": [], "blend": []}

    def run(which):
        if which == "depth":
            rc = L.spz_amd_render_depth_host(stream.data_ptr(), stream.numel(), C.byref(h), C.byref(p), 0,
                                             img_d.ctypes.data, depth.ctypes.data, index.ctypes.data, C.byref(ent), ms)
        else:
            rc = B.spz_amd_render_host(stream.data_ptr(), stream.numel(), C.byref(h), C.byref(p), 0, img.ctypes.data,
                                       C.byref(ent), ms)
        abi.check(rc, which)
        return float(ms[2])

    kinds = [k for k in ("depth", "blend") if k in a.kinds]
    for r in range(a.reps + 1):
        for k in kinds:
            t = run(k)
            if r:
                times[k].append(t)
    out = {"entries": int(ent.value), "times_ms": times, "device": torch.cuda.get_device_name(0),
           "median_share": round(float((index != 0xffffffff).mean()), 4) if "depth" in kinds else None,
           "image_equal": bool(np.array_equal(img.view(np.uint32), img_d.view(np.uint32))) if len(kinds) == 2 else None}
    print("WORKER " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--baseline-lib", default=None, help="libspz_amd.so of the parent commit: times the colour blend")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kinds", default="depth,blend", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.kinds = a.kinds.split(",")
    if a.worker:
        worker(a)
        return

    def spawn(kinds, lib):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--points", str(a.points), "--reps", str(a.reps),
               "--width", str(a.width), "--height", str(a.height), "--kinds", kinds]
        if lib:
            cmd += ["--baseline-lib", lib]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"worker failed ({r.returncode}):\n{r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("WORKER ")][-1][7:])

    med = {"depth": [], "blend": []}
    info = {}
    for _ in range(a.processes):
        # this build's two kernels alternate inside one process; the parent's blend runs in processes of its own
        w = spawn("depth,blend", None)
        info = w
        med["depth"].append(statistics.median(w["times_ms"]["depth"]))
        if a.baseline_lib:
            b = spawn("blend", a.baseline_lib)
            med["blend"].append(statistics.median(b["times_ms"]["blend"]))
            med.setdefault("blend_this_build", []).append(statistics.median(w["times_ms"]["blend"]))
        else:
            med["blend"].append(statistics.median(w["times_ms"]["blend"]))
    d, b = statistics.median(med["depth"]), statistics.median(med["blend"])
    out = {"tool": "depth_bench", "points": a.points, "sh_degree": 3, "width": a.width, "height": a.height,
           "reps": a.reps, "processes": a.processes, "entries": info["entries"],
           "blend_from": "the parent commit's library" if a.baseline_lib else "this build",
           "depth_ms": round(d, 3), "blend_ms": round(b, 3), "depth_over_blend": round(d / b, 3),
           "per_process_median_ms": {k: [round(x, 3) for x in v] for k, v in med.items()},
           "median_share": info["median_share"], "image_equals_blend": info["image_equal"], "device": info["device"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
