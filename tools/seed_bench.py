#!/usr/bin/env python3
"""seed_bench.py — what seed (DESIGN §8 "Seed") costs and gives, at 1920x1080 and stride 1, in THIS process (run it in a
fresh one).  Records, not gates:
    view      one view whose every sample is valid (a rippled depth map, a random image, cover maps that cover about
              half): spz_amd_seed_view_device (select + offsets + emit) between device events, --reps times after a
              warm-up, beside the same work in torch ops on the same device (masks, nonzero, the unprojection in f64,
              cat onto the cloud): the route a Python user would otherwise take.  The bytes the select and the emit need,
              from the shapes, over the call's time: a whole-call rate (three launches), not a kernel's share of peak.
    loop      a 32-view seed of an ellipsoid of --points Gaussians (spz.seed_spz, host images in): the report's three
              stage times and the share of them that is the cover renders.
    psnr      that seeded file refined against the same images and depth maps for --iters iterations
              (device.refine_packed_images with depths): mean PSNR of the file's renders against its source images
              before and after.
The C ABI enqueues a call's three kernels together, so the kernels' own times come from a kernel trace of a run of its
own:
  --trace CSV   summarise the kernel_trace.csv of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
                tools/seed_bench.py --only view --reps 5`: the median time of each seed kernel in each of the two cases
                (the run dispatches each kernel reps + 2 times per case, the all-selected case first), and the rate the
                bytes the select needs make over its time.  With --cold in the traced run the maps come from HBM, not
                from the Infinity Cache the previous repetition left them in.
Prints one JSON line (--out: also writes it)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, F = 1920, 1080, 1400.0


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, reps, torch):
    """Milliseconds of fn() between two events on the current stream, reps times after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def look_at(eye, target, up):
    import numpy as np
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up / np.linalg.norm(up))
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R, (-(R @ eye))[:, None]], axis=1).astype(np.float32)


def trace_summary(path, reps):
    import csv
    import re
    by = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            found = re.search(r"(spz_seed_\w+_kernel)", row["Kernel_Name"])
            if found:
                by.setdefault(found.group(1), []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {"tool": "seed_bench", "mode": "trace", "width": W, "height": H, "stride": 1, "kernels_us": {}}
    per = reps + 2
    for name, spans in sorted(by.items()):
        us = [(b - a) / 1e3 for a, b in sorted(spans)]
        for case, part in (("all_selected", us[:per]), ("half_covered", us[per: 2 * per])):
            part = part[1:] if len(part) > 1 else part  # the first dispatch loads the code object or meets cold caches
            if part:
                out["kernels_us"].setdefault(case, {})[name] = {"median": round(statistics.median(part), 2),
                                                                "min": round(min(part), 2), "max": round(max(part), 2),
                                                                "dispatches": len(part)}
    samples = W * H
    for case, extra in (("all_selected", 0), ("half_covered", 8)):
        k = out["kernels_us"].get(case, {}).get("spz_seed_select_kernel")
        if k:  # depth 4 + colour 12 (+ alpha 4 + accumulated depth 4) read and a flag byte written per sample
            out.setdefault("select_gb_per_s", {})[case] = round(samples * (17 + extra) / k["median"] / 1e3, 1)
    return out


def bench_view(args, torch, np, abi, D, dev):
    L = abi.load_library()
    p = abi.render_params(look_at([0.2, -0.1, -2.5], [0, 0, 0], [0, 1, 0]), F, F, 0.5 * W, 0.5 * H, W, H, 0.2)
    g = torch.Generator(device=dev).manual_seed(3)
    vv, uu = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    depth = (2.5 + 0.3 * torch.sin(uu * 0.01) * torch.cos(vv * 0.013)).float().contiguous()
    image = torch.rand((H, W, 3), generator=g, device=dev)
    cimage = torch.rand((H, W, 4), generator=g, device=dev)                      # alpha above 0.5 for about half
    cdepth = torch.zeros((H, W, 2), device=dev)
    cdepth[..., 0] = depth * cimage[..., 3]                                       # expected depth = the measurement
    samples = W * H
    n0 = 1000
    capacity = n0 + samples
    cloud = D.alloc_cloud(capacity, 0, dev)
    for t in cloud.values():
        t.zero_()
    ptrs = D._seed_capacity_ptrs(cloud, capacity, 0, dev)
    opts = abi.seed_options()
    ws = torch.empty(int(L.spz_amd_seed_workspace_bytes(W, H, 1)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    # --cold: 1 GiB written before every call, four times the Infinity Cache, so the call's maps come from HBM (for the
    # kernel trace: between events the fill would be timed too)
    evict = torch.empty(1 << 30, dtype=torch.uint8, device=dev) if args.cold else None
    for name, ci, cd in (("all_selected", None, None), ("half_covered", cimage, cdepth)):
        def ours():
            if evict is not None:
                evict.fill_(1)
            abi.check(L.spz_amd_seed_view_device(C.byref(ptrs), n0, capacity, 0, C.byref(p), C.byref(opts),
                                                 image.data_ptr(), 3, depth.data_ptr(), None,
                                                 ci.data_ptr() if ci is not None else None,
                                                 cd.data_ptr() if cd is not None else None, counts.data_ptr(),
                                                 ws.data_ptr(), st), "spz_amd_seed_view_device")

        M = torch.tensor(np.array(list(p.world_to_camera), np.float64).reshape(3, 4), device=dev)

        def baseline():
            ok = torch.isfinite(depth) & (depth > p.near_plane) & torch.isfinite(image).all(dim=-1)
            if ci is not None:
                e = cd[..., 0] / ci[..., 3]
                ok &= ~((ci[..., 3] >= 0.5) & ((e.double() - depth.double()).abs() <= 0.05 * depth.double()))
            idx = torch.nonzero(ok.reshape(-1)).reshape(-1)
            z = depth.reshape(-1)[idx].double()
            u, v = (idx % W).double(), (idx // W).double()
            cam = torch.stack([(u + 0.5 - p.cx) / p.fx * z, (v + 0.5 - p.cy) / p.fy * z, z], dim=1)
            pos = ((cam - M[:, 3]) @ M[:, :3]).float()
            ls = torch.log(z * 0.5 * (1.0 / p.fx + 1.0 / p.fy)).float()
            k = idx.numel()
            rot = torch.zeros((k, 4), device=dev)
            rot[:, 3] = 1.0
            col = ((image.reshape(-1, 3)[idx].double() - 0.5) / 0.28209479177387814).float()
            return {"positions": torch.cat([cloud["positions"][: 3 * n0], pos.reshape(-1)]),
                    "scales": torch.cat([cloud["scales"][: 3 * n0], ls[:, None].expand(k, 3).reshape(-1)]),
                    "rotations": torch.cat([cloud["rotations"][: 4 * n0], rot.reshape(-1)]),
                    "alphas": torch.cat([cloud["alphas"][:n0], torch.zeros(k, device=dev)]),
                    "colors": torch.cat([cloud["colors"][: 3 * n0], col.reshape(-1)])}

        t_ours = timed(ours, args.reps, torch)
        got = [int(x) for x in counts.cpu()]
        t_base = timed(baseline, args.reps, torch)
        b = baseline()
        appended = got[1]
        gap = float((b["positions"][3 * n0:] - cloud["positions"][3 * n0: 3 * (n0 + appended)]).abs().max())
        # select: depth 4 + colour 12 (+ alpha 4 + accumulated depth 4) read, 1 written, per sample; emit: flag 1 per sample
        # and depth 4 + colour 12 read, 14 floats written, per appended Gaussian
        need = samples * (4 + 12 + (8 if ci is not None else 0) + 1 + 1) + appended * (16 + 56)
        med = statistics.median(t_ours)
        out[name] = {"counts": got, "seed_view_device_ms": spread(t_ours), "torch_ops_ms": spread(t_base),
                     "torch_over_ours": round(statistics.median(t_base) / med, 2), "bytes_needed": need,
                     "whole_call_gb_per_s": round(need / med / 1e6, 1), "positions_max_abs_difference_to_torch": gap}
    return out


def scene(args, torch, np, abi, D, dev):
    rng = np.random.default_rng(11)
    n = args.points
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cloud = {"positions": (0.45 * d * [1.0, 0.8, 1.2]).astype(np.float32).ravel(),
             "scales": np.full(3 * n, math.log(0.006), np.float32),
             "rotations": np.tile(np.array([0, 0, 0, 1], np.float32), n),
             "alphas": np.full(n, 3.0, np.float32),
             "colors": (np.sin(7.0 * d) * 1.2).astype(np.float32).ravel(),
             "sh": np.zeros(0, np.float32)}
    cloud_t = D.to_device(cloud, dev)
    views, images, depths = [], [], []
    for k in range(args.views):  # a Fibonacci sphere of cameras
        y = 1.0 - 2.0 * (k + 0.5) / args.views
        r, phi = math.sqrt(1.0 - y * y), k * math.pi * (3.0 - math.sqrt(5.0))
        eye = 2.5 * np.array([r * math.cos(phi), y, r * math.sin(phi)])
        up = [0, 1, 0] if abs(y) < 0.95 else [0, 0, 1]
        p = abi.render_params(look_at(eye, [0, 0, 0], up), F, F, 0.5 * W, 0.5 * H, W, H, 0.2)
        depth, image = D.render_depth(cloud_t, n, 0, p, return_image=True, return_index=False)
        z = D.expected_depth(depth, image[..., 3])
        z = torch.where(image[..., 3] >= 0.5, z, torch.full_like(z, float("inf")))
        views.append(p)
        images.append(image[..., :3].contiguous())
        depths.append(z.contiguous())
    torch.cuda.synchronize()
    return views, images, depths


def bench_loop_and_psnr(args, torch, np, abi, D, dev):
    import spz_amd.spz as spz
    views, images, depths = scene(args, torch, np, abi, D, dev)
    vd = [{"world_to_camera": np.array(list(p.world_to_camera), np.float32).reshape(3, 4), "fx": p.fx, "fy": p.fy,
           "cx": p.cx, "cy": p.cy, "width": p.width, "height": p.height} for p in views]
    rep = spz.seed_spz(vd, [t.cpu().numpy() for t in images], [t.cpu().numpy() for t in depths])
    ms = [float(x) for x in rep["ms"]]
    loop = {"views": args.views, "num_points": int(rep["num_points"]),
            "valid": sum(v["valid"] for v in rep["views"]), "refused": sum(v["refused"] for v in rep["views"]),
            "appended_per_view": [int(v["appended"]) for v in rep["views"]],
            "ms": {"cover_renders": round(ms[0], 2), "uploads_selects_emits": round(ms[1], 2), "encode": round(ms[2], 2)},
            "cover_share": round(ms[0] / max(sum(ms), 1e-9), 4)}
    stream = zlib.decompress(rep["data"], 16 + 15)
    rc, hdr = abi.peek_header(stream)
    abi.check(rc, "spz_amd_peek_header")
    stream_t = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(dev)
    with D.refine_packed_images(stream_t, hdr, views, images, args.iters, depths=depths) as res:
        r = res.report
    psnr = {"iterations": args.iters,
            "before": round(statistics.mean(m["psnr"] for m in r["before"]), 3),
            "after": round(statistics.mean(m["psnr"] for m in r["after"]), 3),
            "refine_ms": [round(float(x), 1) for x in r["ms"]]}
    return loop, psnr


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--points", type=int, default=400000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", choices=["view", "loop"], default=None)
    ap.add_argument("--cold", action="store_true", help="view: evict the Infinity Cache before every call (for --trace)")
    ap.add_argument("--trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace:
        line = json.dumps(trace_summary(args.trace, args.reps))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    import numpy as np
    import torch
    from spz_amd import abi, device as D
    if not torch.cuda.is_available():
        sys.exit("seed_bench.py needs a GPU: a time taken without one says nothing")
    dev = torch.device("cuda:0")
    doc = {"tool": "seed_bench", "width": W, "height": H, "stride": 1, "device": torch.cuda.get_device_name(0)}
    if args.only != "loop":
        doc["view"] = bench_view(args, torch, np, abi, D, dev)
    if args.only != "view":
        doc["loop"], doc["psnr"] = bench_loop_and_psnr(args, torch, np, abi, D, dev)
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
