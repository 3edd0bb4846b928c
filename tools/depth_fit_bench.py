#!/usr/bin/env python3
"""depth_fit_bench.py — what depth supervision costs (DESIGN §8 "Depth fit"), four comparisons in THIS process (run it
in a fresh one) on one 1920x1080 view of an SH3 clustered scene of --points Gaussians (make_cloud_clustered):
    backward   spz_amd_render_depth_backward_device against spz_amd_render_backward_device over the same finished
               render: after a warm-up, --reps times, each call between device events on one stream.
    blend      the depth blend backward against spz_amd_render_records_backward_device (the clear and the colour blend
               backward).  The depth blend has no entry of its own: its time is taken as the depth call minus the
               per-Gaussian chain, the chain being render_backward - records_backward of the same repetition (both
               zero the record gradients first; the depth call zeros n more floats).
    loss       spz_amd_depth_loss_device per pair (L1, with weights and a grad_image to add into).
    iteration  one iteration of device.refine_packed_images with a depth map on the view against one without: each
               loop is run for --iters-short and for --iters-long iterations and the difference of the reports' loop
               times divided by the difference of the counts.
Prints one JSON line (--out: also writes it; profiles/depth_fit_bench.json holds one line per scene size)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters-short", type=int, default=4)
    ap.add_argument("--iters-long", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg, W, H = a.points, 3, a.width, a.height
    cloud = D.to_device(make_cloud_clustered(n, deg, 1234), dev)
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    p = abi.render_params(spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), fy, fy, W / 2, H / 2, W, H)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)

    # ---- one finished render, its workspace kept
    ptrs = D._ptrs(cloud, deg, n, dev)
    image, ws, entries = D._rendered_workspace(L, ("cloud", ptrs, n, deg, False), n, p, dev, None, st)
    depth = D.render_depth(cloud, n, deg, p, return_index=False)
    grad_image = torch.empty((H, W, 4), device=dev).normal_(0.0, 1.0, generator=gen)
    grad_depth = torch.empty((H, W), device=dev).normal_(0.0, 1.0, generator=gen)
    grads = D.alloc_cloud(n, deg, dev)
    gp = abi.CloudPtrs(*[grads[k].data_ptr() if grads[k].numel() else None for k in D.FIELDS])
    rec = torch.empty((n, 9), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    bws = torch.empty(int(L.spz_amd_render_depth_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    target = (depth[..., 0] / image[..., 3].clamp_min(1e-6) * 1.05).contiguous()
    target[image[..., 3] < 0.5] = float("inf")
    weight = torch.empty((H, W), device=dev).uniform_(0.0, 1.0, generator=gen)
    loss = torch.zeros(2, dtype=torch.float64, device=dev)
    gd = torch.empty((H, W), dtype=torch.float32, device=dev)
    gi = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    lws = torch.empty(int(L.spz_amd_depth_loss_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
    calls = {
        "render_backward": lambda: L.spz_amd_render_backward_device(
            C.byref(ptrs), n, deg, 0, C.byref(p), entries, image.data_ptr(), grad_image.data_ptr(), C.byref(gp), None,
            status.data_ptr(), ws.data_ptr(), bws.data_ptr(), sp),
        "render_depth_backward": lambda: L.spz_amd_render_depth_backward_device(
            C.byref(ptrs), n, deg, 0, C.byref(p), entries, grad_image.data_ptr(), grad_depth.data_ptr(), C.byref(gp), None,
            None, status.data_ptr(), ws.data_ptr(), bws.data_ptr(), sp),
        "records_backward": lambda: L.spz_amd_render_records_backward_device(
            n, C.byref(p), entries, grad_image.data_ptr(), rec.data_ptr(), status.data_ptr(), ws.data_ptr(), sp),
        "depth_loss": lambda: L.spz_amd_depth_loss_device(
            depth.data_ptr(), image.data_ptr(), target.data_ptr(), weight.data_ptr(), W, H, abi.DEPTH_L1, 0.5, 1.0,
            loss.data_ptr(), gd.data_ptr(), gi.data_ptr(), lws.data_ptr(), sp),
    }
    times = {k: [] for k in calls}
    for r in range(a.reps + 1):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            abi.check(f(), k)
            e1.record(st)
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
    assert int(status.cpu()[0]) == 0
    out = {"tool": "depth_fit_bench", "points": n, "sh_degree": deg, "width": W, "height": H, "reps": a.reps,
           "entries": int(entries), "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        out[k + "_call_ms"] = spread(v)
    med = {k: statistics.median(v) for k, v in times.items()}
    out["depth_over_colour_backward"] = round(med["render_depth_backward"] / med["render_backward"], 3)
    chain = [x - y for x, y in zip(times["render_backward"], times["records_backward"])]
    blend = [x - y for x, y in zip(times["render_depth_backward"], chain)]
    out["chain_ms"] = spread(chain)
    out["depth_blend_backward_ms"] = spread(blend)
    out["depth_over_colour_blend_backward"] = round(statistics.median(blend) / med["records_backward"], 3)
    del grads, rec, bws, ws, grad_image, grad_depth, gd, gi
    torch.cuda.empty_cache()

    # ---- the loops: the difference of two lengths leaves the iterations alone
    stream_b = D.encode(cloud, n, deg, False, abi.RUB, 3)
    cloud["positions"] += torch.empty_like(cloud["positions"]).normal_(0.0, 0.02, generator=gen)
    cloud["colors"] += torch.empty_like(cloud["colors"]).normal_(0.0, 0.3, generator=gen)
    stream_a = D.encode(cloud, n, deg, False, abi.RUB, 3)
    del cloud
    hdr = D.make_header(n, deg)
    picture = D.render_packed(stream_b, hdr, p)
    zmap, _, zimage = D.render_depth_packed(stream_b, hdr, p, return_image=True)
    ztarget = D.expected_depth(zmap, zimage[..., 3]).contiguous()
    ztarget[zimage[..., 3] < 0.5] = float("inf")
    del zmap, zimage
    torch.cuda.synchronize()
    lrs = list(abi.refine_options(0).lr)
    lrs[0] *= 17.3  # the scene's bounding-sphere radius
    loops = {
        "refine_images": lambda k: D.refine_packed_images(stream_a, hdr, [p], [picture], k, lrs=lrs),
        "refine_images_depth": lambda k: D.refine_packed_images(stream_a, hdr, [p], [picture], k, lrs=lrs,
                                                                depths=[ztarget]),
    }
    per = {k: [] for k in loops}
    for r in range(a.reps + 1):
        for k, f in loops.items():
            ms = []
            for count in (a.iters_short, a.iters_long):
                with f(count) as res:
                    ms.append(res.report["ms"][1])
            if r:
                per[k].append((ms[1] - ms[0]) / (a.iters_long - a.iters_short))
    for k, v in per.items():
        out[k + "_iteration_ms"] = spread(v)
    out["depth_over_plain_iteration"] = round(statistics.median(per["refine_images_depth"])
                                              / statistics.median(per["refine_images"]), 3)
    out["iterations_short_long"] = [a.iters_short, a.iters_long]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
