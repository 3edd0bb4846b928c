#!/usr/bin/env python3
"""photo_bench.py — what fitting to photographs costs beside fitting to renders (DESIGN §8 "Fit"), two comparisons in
THIS process (run it in a fresh one; several of them give the spread):
    loss       spz_amd_photo_loss_device with weights and an exposure on, and with neither, against
               spz_amd_image_loss_device on the same 1920x1080 pair: after a warm-up, --reps times, each call between
               device events on one stream.  The exposure path reads the render's three channels for each channel it
               forms, once more than the loss reads them, and adds one reduction of 12 sums.
    iteration  one iteration of device.refine_packed_images (weights and fit_exposure on) against one of
               device.refine_packed, on one 1920x1080 view of an SH3 clustered scene of --points Gaussians
               (make_cloud_clustered), the images being the target's renders: each loop is run for --iters-short and for
               --iters-long iterations and the difference of the reports' loop times divided by the difference of the
               counts, which leaves out the decode before the loop and the encode after it.
Prints one JSON line (--out: also writes it; profiles/photo_bench.json holds one)."""
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

    import numpy as np
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg, lam, W, H = a.points, 3, 0.2, a.width, a.height
    cloud = D.to_device(make_cloud_clustered(n, deg, 1234), dev)
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    p = abi.render_params(spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), fy, fy, W / 2, H / 2, W, H)
    stream_b = D.encode(cloud, n, deg, False, abi.RUB, 3)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    cloud["colors"] += torch.empty_like(cloud["colors"]).normal_(0.0, 0.3, generator=gen)
    cloud["alphas"] += torch.empty_like(cloud["alphas"]).normal_(0.0, 0.5, generator=gen)
    stream_a = D.encode(cloud, n, deg, False, abi.RUB, 3)
    del cloud
    torch.cuda.synchronize()
    hdr = D.make_header(n, deg)
    target = D.render_packed(stream_b, hdr, p)
    image = D.render_packed(stream_a, hdr, p)
    weight = torch.empty((H, W), device=dev).uniform_(0.0, 1.0, generator=gen)
    exposure = np.array([[0.9, 0.02, 0.0, 0.03], [0.0, 1.1, 0.01, -0.02], [0.01, 0.0, 0.95, 0.0]])
    ex = abi.exposure_values(exposure)

    # ---- the loss calls
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    loss = torch.zeros(3, dtype=torch.float64, device=dev)
    grad = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    egrad = torch.zeros(12, dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.spz_amd_photo_loss_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
    calls = {
        "image_loss": lambda: L.spz_amd_image_loss_device(image.data_ptr(), 4, target.data_ptr(), 4, W, H, lam,
                                                          loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), sp),
        "photo_loss_plain": lambda: L.spz_amd_photo_loss_device(image.data_ptr(), 4, target.data_ptr(), 4, None, None, W,
                                                                H, lam, loss.data_ptr(), grad.data_ptr(), None,
                                                                ws.data_ptr(), sp),
        "photo_loss_weights_exposure": lambda: L.spz_amd_photo_loss_device(
            image.data_ptr(), 4, target.data_ptr(), 4, weight.data_ptr(), ex, W, H, lam, loss.data_ptr(), grad.data_ptr(),
            egrad.data_ptr(), ws.data_ptr(), sp),
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
    out = {"tool": "photo_bench", "points": n, "sh_degree": deg, "width": W, "height": H, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        out[k + "_call_ms"] = spread(v)
    out["photo_over_image_loss"] = round(statistics.median(times["photo_loss_weights_exposure"])
                                         / statistics.median(times["image_loss"]), 3)
    out["photo_plain_over_image_loss"] = round(statistics.median(times["photo_loss_plain"])
                                               / statistics.median(times["image_loss"]), 3)
    del grad, ws, image
    torch.cuda.empty_cache()

    # ---- the loops: the difference of two lengths leaves the iterations alone
    lrs = list(abi.refine_options(0).lr)
    lrs[0] *= 17.3  # the scene's bounding-sphere radius
    loops = {
        "refine_packed": lambda k: D.refine_packed(stream_a, hdr, stream_b, hdr, [p], k, lrs=lrs),
        "refine_packed_images": lambda k: D.refine_packed_images(stream_a, hdr, [p], [target], k, weights=[weight],
                                                                 fit_exposure=True, lrs=lrs),
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
    out["images_over_packed_iteration"] = round(statistics.median(per["refine_packed_images"])
                                                / statistics.median(per["refine_packed"]), 3)
    out["iterations_short_long"] = [a.iters_short, a.iters_long]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
