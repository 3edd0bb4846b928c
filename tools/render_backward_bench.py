#!/usr/bin/env python3
"""render_backward_bench.py — the render backward on one 1920x1080 view of an SH3 clustered scene (make_cloud_clustered)
held as a resident float cloud, --points Gaussians (the figures in profiles/ are at 1 M and 10 M), in THIS process
(run it in a fresh one; several of them give the spread):
  the prepare step once, then --reps times after a warm-up, each between device events on one stream:
    finish    spz_amd_render_finish_device: tile entries, their sort, the ranges and the forward blend
    backward  spz_amd_render_backward_device: the zeroing of the n x 9 record gradients, the blend backward and the
              preprocess backward
The C ABI enqueues a call's kernels together, so the kernels' own times come from a kernel trace of a run of its own:
  --trace DB   summarise the rocpd database of `rocprofv3 --kernel-trace --stats -- python tools/render_backward_bench.py
               --reps 3 ...`: median dispatch time of spz_render_blend_backward_kernel, of
               spz_render_preprocess_backward_kernel and of the forward's spz_render_blend_kernel in that same process,
               and the backward / forward blend ratio.
Global atomics are counted by arithmetic: the blend backward issues at most one per (tile entry, record value), 9 per
entry, where one per used pair and value would be up to 256 times as many for a Gaussian that covers its tile.
  --tolerance  instead: the GPU test's cases (tests/test_gpu_render_grad.py), |device - ref64| / max|ref32 - ref64| per
               array (the test's bound is 8).
  --collect F... --out O   merge the JSON lines of several runs into one document: medians and ranges.
Prints one JSON line (--out: also writes it)."""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = {"spz_render_blend_backward_kernel": "blend_backward", "spz_render_preprocess_backward_kernel":
           "preprocess_backward", "spz_render_blend_kernel": "forward_blend"}


def trace_summary(path):
    import sqlite3
    with sqlite3.connect(path) as c:
        rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    by = {}
    for name, us in rows:
        found = re.search(r"(spz_render_\w+_kernel)", name)
        if found and found.group(1) in KERNELS:
            by.setdefault(KERNELS[found.group(1)], []).append(us)
    out = {"tool": "render_backward_bench", "mode": "trace"}
    for k, v in by.items():
        v = v[1:] if len(v) > 1 else v  # the first dispatch loads the code object
        out[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                          "dispatches": len(v)}
    if "blend_backward" in by and "forward_blend" in by:
        out["blend_backward_over_forward_blend"] = round(out["blend_backward_us"]["median"]
                                                         / out["forward_blend_us"]["median"], 2)
    return out


def tolerance_ratios():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import test_gpu_render_grad as T
    from spz_amd import device as D
    dev = torch.device("cuda:0")
    out = {"tool": "render_backward_bench", "mode": "tolerance", "bound": 8.0, "ratios": {}}
    for name in T.CASES:
        ref = T.reference(name)
        got = D.render_backward(D.to_device(ref["cloud"], dev), ref["n"], ref["deg"], ref["params"],
                                torch.as_tensor(ref["G"]).to(dev), antialiased=ref["aa"], return_record_grads=True)
        r = {}
        for k in T.ARRAYS + ("records",):
            want = ref["g64"][k]
            e32 = np.abs(ref["g32"][k] - want).max() if want.size else 0.0
            err = np.abs(got[k].cpu().numpy().astype(np.float64).reshape(want.shape) - want).max() if want.size else 0.0
            r[k] = round(float(err / e32), 3) if e32 else ("exact" if err == 0.0 else "inexact")
        out["ratios"][name] = r
    return out


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def collect(paths):
    runs, traces, tol = {}, {}, None
    for p in paths:
        for line in open(p):
            line = line.strip()
            if not line.startswith("{"):
                continue
            d = json.loads(line)
            if d.get("mode") == "tolerance":
                tol = d
            elif d.get("mode") == "trace":
                traces[str(d.get("points"))] = {k: v for k, v in d.items() if k not in ("tool", "mode", "points")}
            elif d.get("mode") == "events":
                runs.setdefault(str(d["points"]), []).append(d)
    out = {"tool": "render_backward_bench", "tolerance_bound": 8.0,
           "tolerance_ratios": tol["ratios"] if tol else "not measured", "sizes": {}}
    for n, rs in runs.items():
        out["sizes"][n] = {
            "processes": len(rs), "reps_per_process": rs[0]["reps"], "width": rs[0]["width"], "height": rs[0]["height"],
            "entries": rs[0]["entries"], "global_atomics_at_most": rs[0]["global_atomics_at_most"],
            "global_atomics_per_considered_pair_at_most": rs[0]["global_atomics_per_considered_pair_at_most"],
            "finish_call_ms_median_of_process_medians": spread([r["finish_call_ms"]["median"] for r in rs]),
            "backward_call_ms_median_of_process_medians": spread([r["backward_call_ms"]["median"] for r in rs]),
            "kernel_trace": traces.get(n, "not measured"), "device": rs[0]["device"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="a rocpd .db of a traced run to summarise")
    ap.add_argument("--tolerance", action="store_true")
    ap.add_argument("--collect", nargs="+", default=None)
    a = ap.parse_args()
    if a.trace:
        out = trace_summary(a.trace)
        out["points"] = a.points
    elif a.tolerance:
        out = tolerance_ratios()
    elif a.collect:
        out = collect(a.collect)
    else:
        out = events(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def events(a):
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import FIELDS, make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg = a.points, 3
    cloud = D.to_device(make_cloud_clustered(n, deg, 1234), dev)
    W, H = a.width, a.height
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    m = spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    p = abi.render_params(m, fy, fy, W / 2, H / 2, W, H)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    G = torch.empty((H, W, 4), dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=gen)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    ptrs = D._ptrs(cloud, deg, n, dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ws, entries = D._prepared_workspace(L, ("cloud", ptrs, n, deg, False), n, p, dev, None, total, st)
    image = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    grads = D.alloc_cloud(n, deg, dev)
    gp = abi.CloudPtrs(*[grads[k].data_ptr() for k in FIELDS])
    bws = torch.empty(int(L.spz_amd_render_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    fin, bwd = [], []
    for r in range(a.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(st)
        abi.check(L.spz_amd_render_finish_device(n, C.byref(p), entries, image.data_ptr(), status.data_ptr(),
                                                 ws.data_ptr(), sp), "spz_amd_render_finish_device")
        e[1].record(st)
        abi.check(L.spz_amd_render_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), entries, image.data_ptr(),
                                                   G.data_ptr(), C.byref(gp), None, status[1:].data_ptr(), ws.data_ptr(),
                                                   bws.data_ptr(), sp), "spz_amd_render_backward_device")
        e[2].record(st)
        torch.cuda.synchronize()
        if r:
            fin.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    assert status.cpu().tolist() == [0, 0]
    finite = all(bool(torch.isfinite(grads[k]).all()) for k in FIELDS)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return {"tool": "render_backward_bench", "mode": "events", "points": n, "sh_degree": deg, "width": W, "height": H,
            "reps": a.reps, "entries": int(entries), "tiles": tiles,
            "finish_call_ms": spread(fin), "backward_call_ms": spread(bwd),
            "global_atomics_at_most": 9 * int(entries),
            "global_atomics_per_considered_pair_at_most": round(9 / 256, 4),
            "gradients_finite": finite,
            "nonzero_position_gradients": int((grads["positions"].view(-1, 3) != 0).any(dim=1).sum()),
            "coverage": round(float((image[..., 3] > 0).float().mean()), 4),
            "device": torch.cuda.get_device_name(0)}


if __name__ == "__main__":
    main()
