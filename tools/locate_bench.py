#!/usr/bin/env python3
"""locate_bench.py — the pieces of locate (DESIGN §8 "Locate") on one 1920x1080 view of an SH3 clustered scene
(make_cloud_clustered) held as a resident float cloud, --points Gaussians (the figures in profiles/ are at 1 M and 10 M),
in THIS process (run it in a fresh one).  After a warm-up, --reps times, each call between device events on one stream:
    view_backward     spz_amd_render_view_backward_device: the per-Gaussian f64 chain with its in-workgroup sum, and the
                      one-workgroup sum of the rows
    records_backward  spz_amd_render_records_backward_device: the clear and the blend backward
    render_backward   spz_amd_render_backward_device: the blend backward and the preprocess backward; the preprocess
                      backward's own time is taken as render_backward - records_backward of the same repetition (both
                      run the same blend backward on the same workspace)
    iteration         one locate iteration by the wall clock: prepare, the total read back, finish, image loss, records
                      backward, view backward, the 12 doubles read back
    baseline          the route a Python user takes: device.render_autograd(world_to_camera=W) + an SSIM loss of torch
                      convolutions + backward + W.grad read back, by the wall clock
  --collect F... --out O   the lines of several sizes as one document (profiles/locate_bench.json).
Prints one JSON line (--out: also writes it)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.refine_bench import spread, torch_ssim_loss  # noqa: E402


def events(a):
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import FIELDS, make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg, lam = a.points, 3, 0.2
    cloud = D.to_device(make_cloud_clustered(n, deg, 1234), dev)
    W, H = a.width, a.height
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    truth = spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    rough = spz.look_at([4.3, 6.2, -27.5], [0.2, -0.1, 0.0], [0.0, 1.0, 0.0])
    target = D.render(cloud, n, deg, abi.render_params(truth, fy, fy, W / 2, H / 2, W, H))
    p = abi.render_params(rough, fy, fy, W / 2, H / 2, W, H)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    ptrs = D._ptrs(cloud, deg, n, dev)
    image, ws, entries = D._rendered_workspace(L, ("cloud", ptrs, n, deg, False), n, p, dev, None, st)
    _, grad_image = D.image_loss(image, target, lam)
    grads = D.alloc_cloud(n, deg, dev)
    gp = abi.CloudPtrs(*[grads[k].data_ptr() for k in FIELDS])
    bws = torch.empty(int(L.spz_amd_render_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    vws = torch.empty(int(L.spz_amd_render_view_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    lws = torch.empty(int(L.spz_amd_image_loss_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 9), dtype=torch.float32, device=dev)
    view = torch.empty((3, 4), dtype=torch.float64, device=dev)
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    loss = torch.zeros(3, dtype=torch.float64, device=dev)
    steps = {k: [] for k in ("render_backward", "records_backward", "view_backward")}
    for r in range(a.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(st)
        abi.check(L.spz_amd_render_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), entries, image.data_ptr(),
                                                   grad_image.data_ptr(), C.byref(gp), None, status.data_ptr(),
                                                   ws.data_ptr(), bws.data_ptr(), sp), "spz_amd_render_backward_device")
        e[1].record(st)
        abi.check(L.spz_amd_render_records_backward_device(n, C.byref(p), entries, grad_image.data_ptr(), rec.data_ptr(),
                                                           status[1:].data_ptr(), ws.data_ptr(), sp),
                  "spz_amd_render_records_backward_device")
        e[2].record(st)
        abi.check(L.spz_amd_render_view_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), entries, rec.data_ptr(),
                                                        view.data_ptr(), status[2:].data_ptr(), ws.data_ptr(),
                                                        vws.data_ptr(), sp), "spz_amd_render_view_backward_device")
        e[3].record(st)
        torch.cuda.synchronize()
        if r:
            for j, k in enumerate(("render_backward", "records_backward", "view_backward")):
                steps[k].append(e[j].elapsed_time(e[j + 1]))
    assert status.cpu().tolist() == [0, 0, 0]
    pre = [x - y for x, y in zip(steps["render_backward"], steps["records_backward"])]
    # one iteration as spz_amd_locate_*_host runs it, by the wall clock
    iteration = []
    ws0 = torch.empty(int(L.spz_amd_render_workspace_bytes(n, int(1.2 * entries) + 1024)), dtype=torch.uint8, device=dev)
    room = int(1.2 * entries) + 1024
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        abi.check(L.spz_amd_render_prepare_cloud_device(C.byref(ptrs), n, deg, 0, C.byref(p), total.data_ptr(), None,
                                                        ws0.data_ptr(), sp), "spz_amd_render_prepare_cloud_device")
        m = int(total.cpu()[0])
        assert m <= room
        abi.check(L.spz_amd_render_finish_device(n, C.byref(p), room, image.data_ptr(), status.data_ptr(), ws0.data_ptr(),
                                                 sp), "spz_amd_render_finish_device")
        abi.check(L.spz_amd_image_loss_device(image.data_ptr(), 4, target.data_ptr(), 4, W, H, lam, loss.data_ptr(),
                                              grad_image.data_ptr(), lws.data_ptr(), sp), "spz_amd_image_loss_device")
        abi.check(L.spz_amd_render_records_backward_device(n, C.byref(p), room, grad_image.data_ptr(), rec.data_ptr(),
                                                           status[1:].data_ptr(), ws0.data_ptr(), sp),
                  "spz_amd_render_records_backward_device")
        abi.check(L.spz_amd_render_view_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), room, rec.data_ptr(),
                                                        view.data_ptr(), status[2:].data_ptr(), ws0.data_ptr(),
                                                        vws.data_ptr(), sp), "spz_amd_render_view_backward_device")
        g = view.cpu()
        if r:
            iteration.append(1e3 * (time.perf_counter() - t0))
    out = {"tool": "locate_bench", "points": n, "sh_degree": deg, "width": W, "height": H, "reps": a.reps,
           "entries": int(entries), "view_backward_call_ms": spread(steps["view_backward"]),
           "records_backward_call_ms": spread(steps["records_backward"]),
           "render_backward_call_ms": spread(steps["render_backward"]),
           "preprocess_backward_ms_by_difference": spread(pre), "iteration_wall_ms": spread(iteration),
           "view_grad_abs_max": float(g.abs().max()), "device": torch.cuda.get_device_name(0)}
    if not a.no_baseline:
        del grads, bws, ws0
        torch.cuda.empty_cache()
        w1 = torch.tensor([math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)], device=dev)
        w1 = w1 / w1.sum()
        window = (w1[:, None] * w1[None, :])[None, None].repeat(3, 1, 1, 1).contiguous()
        base = []
        for r in range(a.reps + 1):
            Wt = torch.tensor(rough, dtype=torch.float64, device=dev, requires_grad=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = torch_ssim_loss(D.render_autograd(cloud, n, deg, p, world_to_camera=Wt), target, lam, window)
            val.backward()
            gb = Wt.grad.cpu()
            if r:
                base.append(1e3 * (time.perf_counter() - t0))
        out["baseline_iteration_wall_ms"] = spread(base)
        out["baseline_view_grad_abs_max"] = float(gb.abs().max())
    return out


def collect(paths):
    sizes = {}
    for path in paths:
        for line in open(path):
            line = line.strip()
            if line.startswith("{") and json.loads(line).get("tool") == "locate_bench":
                d = json.loads(line)
                sizes[str(d["points"])] = {k: v for k, v in d.items() if k not in ("tool", "points")}
    return {"tool": "locate_bench", "sizes": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--collect", nargs="+", default=None)
    a = ap.parse_args()
    out = collect(a.collect) if a.collect else events(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
