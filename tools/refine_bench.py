#!/usr/bin/env python3
"""refine_bench.py — the pieces of refine (DESIGN §8 "Refine") on one 1920x1080 view of an SH3 clustered scene
(make_cloud_clustered) held as a resident float cloud, --points Gaussians (the figures in profiles/ are at 1 M and 10 M),
in THIS process (run it in a fresh one; several of them give the spread).  After a warm-up, --reps times, each step
between device events on one stream:
    loss      spz_amd_image_loss_device on a render against a second render, beside spz_amd_image_metrics_device on
              the same pair
    adam      spz_amd_adam_step_device over all six arrays: 28 bytes per parameter (g, m, v, p read; m, v, p written),
              and the rate that makes
    iteration prepare (spz_amd_render_prepare_cloud_device), finish, loss, backward, adam: one refine iteration but
              for the read-back of the total, which is taken once here
    baseline  the route refine replaces, in the same process: device.render_autograd + an SSIM loss of torch
              convolutions + torch.optim.Adam over the six tensors, one iteration between two events
The C ABI enqueues a call's kernels together, so the kernels' own times come from a kernel trace of a run of its own:
  --trace DB   summarise the rocpd database of `rocprofv3 --kernel-trace --stats -- python tools/refine_bench.py
               --reps 3 --no-baseline ...`: median dispatch time of every kernel of an iteration.
  --tolerance  instead: the GPU test's image-loss cases (tests/test_gpu_refine.py), |device - ref64| / max|ref32 - ref64|
               of the gradient per case (the test's bound is 8), and the largest.
  --e2e        instead: spz_refine file -> file.  The --points scene is saved, decimated (spz.decimate_spz to a tenth)
               and the copy refined against the original over 8 orbit views of --width x --height for --iters
               iterations; wall clock of the tool, and its report's mean PSNR and SSIM before and after.
  --collect F... --out O   merge the JSON lines of several runs into one document: medians and ranges.
  --densify    instead: the densify round (DESIGN §8 "Densify") at --points SH3 Gaussians with planted statistics (about
               a fifth cloned, a fifth split, a few culled): spz_amd_densify_apply_device (one launch for the 18 arrays
               of parameters and both moments) against torch.index_select over the same 18 arrays with the same parent
               list, the route a Python user would otherwise take (it copies moments where apply writes zeros, and
               leaves the children where the parents are); one whole round (plan, the read-back of the count, apply) by
               the wall clock; and one refine iteration at the same size beside it.
  --collect-densify F... --out O   the --densify lines of several sizes as one document (profiles/densify_bench.json).
Prints one JSON line (--out: also writes it)."""
import argparse
import ctypes as C
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNEL = re.compile(r"(spz_\w+_kernel)")
COPY_CEILING_TBS = 6.29  # a float4 copy on this chip, measured


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def trace_summary(path):
    import sqlite3
    with sqlite3.connect(path) as c:
        rows = [(n, d / 1e3) for n, d in c.execute("select name, duration from kernels order by start")]
    by = {}
    for name, us in rows:
        found = KERNEL.search(name)
        if found:
            by.setdefault(found.group(1), []).append(us)
    out = {"tool": "refine_bench", "mode": "trace", "kernels_us": {}}
    for k, v in sorted(by.items()):
        v = v[1:] if len(v) > 1 else v  # the first dispatch loads the code object
        out["kernels_us"][k] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                "max": round(max(v), 1), "dispatches": len(v)}
    return out


def tolerance_ratios():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import test_gpu_refine as T
    from spz_amd import device as D
    dev = torch.device("cuda:0")
    out = {"tool": "refine_bench", "mode": "tolerance", "bound": 8.0, "ratios": {}}
    worst = 0.0
    for size in T.SIZES:
        for ca, cb in ((4, 3), (3, 4)):
            for lam in T.LAMBDAS:
                ref = T.loss_reference(size, ca, cb, lam)
                _, g = D.image_loss(torch.as_tensor(ref["a"]).to(dev), torch.as_tensor(ref["b"]).to(dev), lam)
                e32 = np.abs(ref["r32"]["grad"] - ref["r64"]["grad"]).max()
                err = np.abs(g.cpu().numpy().astype(np.float64) - ref["r64"]["grad"]).max()
                r = float(err / e32)
                worst = max(worst, r)
                out["ratios"][f"{size} {ca}/{cb} lambda {lam}"] = round(r, 4)
    out["largest_ratio"] = round(worst, 4)
    return out


def collect(paths):
    runs, traces, tol, e2e = {}, {}, None, None
    for p in paths:
        for line in open(p):
            line = line.strip()
            if not line.startswith("{"):
                continue
            d = json.loads(line)
            if d.get("mode") == "tolerance":
                tol = d
            elif d.get("mode") == "trace":
                traces[str(d.get("points"))] = d["kernels_us"]
            elif d.get("mode") == "e2e":
                e2e = {k: v for k, v in d.items() if k not in ("tool", "mode")}
            elif d.get("mode") == "events":
                runs.setdefault(str(d["points"]), []).append(d)
    out = {"tool": "refine_bench", "copy_ceiling_tb_per_s": COPY_CEILING_TBS, "tolerance_bound": 8.0,
           "tolerance": {k: tol[k] for k in ("largest_ratio", "ratios")} if tol else "not measured", "sizes": {},
           "end_to_end": e2e or "not measured"}
    for n, rs in runs.items():
        size = {"processes": len(rs), "reps_per_process": rs[0]["reps"], "width": rs[0]["width"],
                "height": rs[0]["height"], "entries": rs[0]["entries"], "adam_bytes": rs[0]["adam_bytes"],
                "kernel_trace": traces.get(n, "not measured"), "device": rs[0]["device"]}
        for key in sorted({k for r in rs for k in r if k.endswith("_ms") or k.endswith("_tb_per_s")}):
            vals = [r[key]["median"] for r in rs if key in r]
            if vals:
                size[key + "_median_of_process_medians"] = spread(vals)
        if all("baseline_iteration_ms" in r for r in rs):
            size["baseline_over_iteration"] = round(
                statistics.median([r["baseline_iteration_ms"]["median"] for r in rs])
                / statistics.median([r["iteration_ms"]["median"] for r in rs]), 2)
        out["sizes"][n] = size
    return out


def torch_ssim_loss(img, target, lam, window):
    """The loss as a Python user writes it today: torch.clamp, conv2d with an 11x11 Gaussian window, padding 5."""
    import torch
    import torch.nn.functional as F
    a = torch.clamp(img[..., :3], 0.0, 1.0).permute(2, 0, 1)[None]
    b = torch.clamp(target[..., :3], 0.0, 1.0).permute(2, 0, 1)[None]
    mu_a, mu_b = F.conv2d(a, window, padding=5, groups=3), F.conv2d(b, window, padding=5, groups=3)
    s_a = F.conv2d(a * a, window, padding=5, groups=3) - mu_a * mu_a
    s_b = F.conv2d(b * b, window, padding=5, groups=3) - mu_b * mu_b
    s_ab = F.conv2d(a * b, window, padding=5, groups=3) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu_a * mu_b + c1) * (2 * s_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_a + s_b + c2))).mean()
    return (1.0 - lam) * (a - b).abs().mean() + lam * (1.0 - ssim)


def events(a):
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import FIELDS, make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg, lam = a.points, 3, 0.2
    host = make_cloud_clustered(n, deg, 1234)
    cloud = D.to_device(host, dev)
    W, H = a.width, a.height
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    p = abi.render_params(spz.look_at([4.0, 6.0, -28.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), fy, fy, W / 2, H / 2, W, H)
    # the target: the scene itself; the trained cloud: its colours and alphas disturbed
    target = D.render(cloud, n, deg, p)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    cloud["colors"] += torch.empty_like(cloud["colors"]).normal_(0.0, 0.3, generator=gen)
    cloud["alphas"] += torch.empty_like(cloud["alphas"]).normal_(0.0, 0.5, generator=gen)
    start = {k: v.clone() for k, v in cloud.items()}
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    ptrs = D._ptrs(cloud, deg, n, dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    _, total0 = D._prepared_workspace(L, ("cloud", ptrs, n, deg, False), n, p, dev, None, total, st)
    entries = int(1.3 * total0) + 1024  # the steps move the total: room for it
    ws, _ = D._prepared_workspace(L, ("cloud", ptrs, n, deg, False), n, p, dev, entries, total, st)
    image = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    grad_image = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    grads, m, v = (D.alloc_cloud(n, deg, dev) for _ in range(3))
    for c in (m, v):
        for t in c.values():
            t.zero_()
    cp = [abi.CloudPtrs(*[c[k].data_ptr() for k in FIELDS]) for c in (cloud, grads, m, v)]
    bws = torch.empty(int(L.spz_amd_render_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    lws = torch.empty(int(L.spz_amd_image_loss_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
    mws = torch.empty(int(L.spz_amd_image_metrics_workspace_bytes(W, H)), dtype=torch.uint8, device=dev)
    loss = torch.zeros(3, dtype=torch.float64, device=dev)
    metrics = torch.zeros(5, dtype=torch.float64, device=dev)
    skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    lrs = list(abi.refine_options(0).lr)
    lrs[0] *= 17.3  # the scene's bounding-sphere radius
    params = sum(t.numel() for t in cloud.values())
    steps = {k: [] for k in ("metrics", "prepare", "finish", "loss", "backward", "adam")}
    losses = []
    for r in range(a.reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        e[0].record(st)
        abi.check(L.spz_amd_image_metrics_device(image.data_ptr(), 4, target.data_ptr(), 4, W, H, metrics.data_ptr(), None,
                                                 mws.data_ptr(), sp), "spz_amd_image_metrics_device")
        e[1].record(st)
        abi.check(L.spz_amd_render_prepare_cloud_device(C.byref(ptrs), n, deg, 0, C.byref(p), total.data_ptr(), None,
                                                        ws.data_ptr(), sp), "spz_amd_render_prepare_cloud_device")
        e[2].record(st)
        abi.check(L.spz_amd_render_finish_device(n, C.byref(p), entries, image.data_ptr(), status.data_ptr(),
                                                 ws.data_ptr(), sp), "spz_amd_render_finish_device")
        e[3].record(st)
        abi.check(L.spz_amd_image_loss_device(image.data_ptr(), 4, target.data_ptr(), 4, W, H, lam, loss.data_ptr(),
                                              grad_image.data_ptr(), lws.data_ptr(), sp), "spz_amd_image_loss_device")
        e[4].record(st)
        abi.check(L.spz_amd_render_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), entries, image.data_ptr(),
                                                   grad_image.data_ptr(), C.byref(cp[1]), None, status[1:].data_ptr(),
                                                   ws.data_ptr(), bws.data_ptr(), sp), "spz_amd_render_backward_device")
        e[5].record(st)
        abi.check(L.spz_amd_adam_step_device(C.byref(cp[0]), C.byref(cp[1]), C.byref(cp[2]), C.byref(cp[3]), n, deg, 63,
                                             abi.adam_scalars(r + 1, lrs), skipped.data_ptr(), sp),
                  "spz_amd_adam_step_device")
        e[6].record(st)
        torch.cuda.synchronize()
        assert int(total.cpu()[0]) <= entries, "the step moved the total past the workspace: give more room"
        losses.append(float(loss.cpu()[0]))
        if r:
            for j, k in enumerate(("metrics", "prepare", "finish", "loss", "backward", "adam")):
                steps[k].append(e[j].elapsed_time(e[j + 1]))
    assert status.cpu().tolist() == [0, 0]
    adam_bytes = 28 * params
    out = {"tool": "refine_bench", "mode": "events", "points": n, "sh_degree": deg, "width": W, "height": H,
           "reps": a.reps, "entries": int(total0), "parameters": params, "adam_bytes": adam_bytes,
           "metrics_call_ms": spread(steps["metrics"]), "loss_call_ms": spread(steps["loss"]),
           "prepare_call_ms": spread(steps["prepare"]), "finish_call_ms": spread(steps["finish"]),
           "backward_call_ms": spread(steps["backward"]), "adam_call_ms": spread(steps["adam"]),
           "adam_tb_per_s": spread([adam_bytes / (ms * 1e-3) / 1e12 for ms in steps["adam"]]),
           "iteration_ms": spread([sum(steps[k][i] for k in ("prepare", "finish", "loss", "backward", "adam"))
                                   for i in range(a.reps)]),
           "loss_first_last": [losses[0], losses[-1]], "skipped": int(skipped.cpu()[0]),
           "device": torch.cuda.get_device_name(0)}
    out["adam_fraction_of_copy_ceiling"] = round(out["adam_tb_per_s"]["median"] / COPY_CEILING_TBS, 3)
    if not a.no_baseline:
        del grads, m, v, bws
        torch.cuda.empty_cache()
        leaves = {k: start[k].clone().requires_grad_(True) for k in FIELDS}
        opt = torch.optim.Adam([{"params": [leaves[k]], "lr": lr} for k, lr in zip(FIELDS, lrs)], betas=(0.9, 0.999),
                               eps=1e-15)
        w1 = torch.tensor([math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)], device=dev)
        w1 = w1 / w1.sum()
        window = (w1[:, None] * w1[None, :])[None, None].repeat(3, 1, 1, 1).contiguous()
        base, base_losses = [], []
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            opt.zero_grad(set_to_none=True)
            val = torch_ssim_loss(D.render_autograd(leaves, n, deg, p), target, lam, window)
            val.backward()
            opt.step()
            e1.record(st)
            torch.cuda.synchronize()
            base_losses.append(float(val.detach()))
            if r:
                base.append(e0.elapsed_time(e1))
        out["baseline_iteration_ms"] = spread(base)
        out["baseline_loss_first_last"] = [base_losses[0], base_losses[-1]]
    return out


def densify(a):
    import numpy as np
    import torch
    from spz_amd import abi, device as D
    from spz_amd.synth import FIELDS, floats_per_point, make_cloud_clustered

    dev = torch.device("cuda:0")
    L = abi.load_library()
    n, deg = a.points, 3
    cloud = D.to_device(make_cloud_clustered(n, deg, 1234), dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    m = {k: torch.empty_like(t).normal_(0.0, 0.1, generator=gen) for k, t in cloud.items()}
    v = {k: torch.empty_like(t).uniform_(0.0, 0.01, generator=gen) for k, t in cloud.items()}
    # planted statistics: g uniform in [0, 2.5 thr), so 60 % are candidates; the budget grants 40 % of n
    lim = abi.densify_thresholds(abi.densify_options(interval=1, extent=1.0, grad_threshold=2.0 ** -12))
    med = float(cloud["scales"].view(-1, 3).max(dim=1).values.median())
    lim.log_dense = med  # half of the candidates split
    denom = torch.randint(1, 5, (n,), generator=gen, device=dev, dtype=torch.int32)
    accum = torch.empty(n, device=dev).uniform_(0.0, 2.5 * 2.0 ** -12, generator=gen) * denom
    max_points = int(1.4 * n)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    plan = D.densify_plan(accum, denom, cloud["scales"], cloud["alphas"], lim, max_points)
    n_new = plan["num_points"]
    parent, child = plan["parent"].contiguous(), plan["child"].contiguous()
    dst = [D.alloc_cloud(n_new, deg, dev) for _ in range(3)]
    src_p = [D._ptrs(c, deg, n, dev) for c in (cloud, m, v)]
    dst_p = [D._ptrs(c, deg, n_new, dev) for c in dst]
    apply_ms, select_ms, round_ms = [], [], []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        abi.check(L.spz_amd_densify_apply_device(C.byref(src_p[0]), C.byref(src_p[1]), C.byref(src_p[2]),
                                                 C.byref(dst_p[0]), C.byref(dst_p[1]), C.byref(dst_p[2]),
                                                 parent.data_ptr(), child.data_ptr(), n, n_new, n_new, deg, 7, r, sp),
                  "spz_amd_densify_apply_device")
        e1.record(st)
        torch.cuda.synchronize()
        if r:
            apply_ms.append(e0.elapsed_time(e1))
    index = parent.to(torch.int64)
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for c, d in zip((cloud, m, v), dst):
            for k in FIELDS:
                w = floats_per_point(k, deg)
                torch.index_select(c[k].view(-1, w), 0, index, out=d[k].view(-1, w))
        e1.record(st)
        torch.cuda.synchronize()
        if r:
            select_ms.append(e0.elapsed_time(e1))
    # one whole round by the wall clock: plan (with its read-back of the counts), then apply
    cap = min(2 * n, max(max_points, n))
    action = torch.empty(n, dtype=torch.uint8, device=dev)
    par = torch.empty(cap, dtype=torch.int32, device=dev)
    chi = torch.empty(cap, dtype=torch.uint8, device=dev)
    counts = torch.empty(5, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.spz_amd_densify_plan_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    h = (C.c_uint64 * 5)()
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        abi.check(L.spz_amd_densify_plan_host(accum.data_ptr(), denom.data_ptr(), cloud["scales"].data_ptr(),
                                              cloud["alphas"].data_ptr(), n, C.byref(lim), max_points, cap,
                                              action.data_ptr(), par.data_ptr(), chi.data_ptr(), counts.data_ptr(),
                                              ws.data_ptr(), h, sp), "spz_amd_densify_plan_host")
        abi.check(L.spz_amd_densify_apply_device(C.byref(src_p[0]), C.byref(src_p[1]), C.byref(src_p[2]),
                                                 C.byref(dst_p[0]), C.byref(dst_p[1]), C.byref(dst_p[2]), par.data_ptr(),
                                                 chi.data_ptr(), n, int(h[0]), n_new, deg, 7, r, sp),
                  "spz_amd_densify_apply_device")
        torch.cuda.synchronize()
        if r:
            round_ms.append(1e3 * (time.perf_counter() - t0))
    assert int(h[0]) == n_new
    floats = sum(floats_per_point(k, deg) for k in FIELDS)
    # every output float of the 18 arrays read and written: an upper bound, zeroed moments are not read
    moved = 2 * 3 * 4 * floats * n_new
    out = {"tool": "refine_bench", "mode": "densify", "points": n, "sh_degree": deg, "reps": a.reps,
           "new_points": n_new, "cloned": plan["cloned"], "split": plan["split"], "culled": plan["culled"],
           "refused": plan["refused"], "apply_ms": spread(apply_ms), "index_select_18_arrays_ms": spread(select_ms),
           "apply_bytes_upper_bound": moved,
           "apply_tb_per_s": spread([moved / (ms * 1e-3) / 1e12 for ms in apply_ms]),
           "index_select_tb_per_s": spread([moved / (ms * 1e-3) / 1e12 for ms in select_ms]),
           "index_select_over_apply": round(statistics.median(select_ms) / statistics.median(apply_ms), 3),
           "round_wall_ms": spread(round_ms), "device": torch.cuda.get_device_name(0)}
    del cloud, m, v, dst, accum, denom, parent, child, index, par, chi, ws, action
    torch.cuda.empty_cache()
    a.no_baseline = True
    it = events(a)
    out["iteration_ms"] = it["iteration_ms"]
    out["iteration_view"] = [it["width"], it["height"]]
    out["round_over_iteration"] = round(out["round_wall_ms"]["median"] / it["iteration_ms"]["median"], 3)
    return out


def collect_densify(paths):
    sizes = {}
    for p in paths:
        for line in open(p):
            line = line.strip()
            if line.startswith("{") and json.loads(line).get("mode") == "densify":
                d = json.loads(line)
                sizes[str(d["points"])] = {k: v for k, v in d.items() if k not in ("tool", "mode", "points")}
    return {"tool": "refine_bench", "mode": "densify", "copy_ceiling_tb_per_s": COPY_CEILING_TBS, "sizes": sizes}


def e2e(a):
    import spz_amd.spz as spz
    from spz_amd.synth import make_cloud_clustered
    n = a.points
    with tempfile.TemporaryDirectory() as td:
        big, dec, out = (os.path.join(td, x) for x in ("scene.spz", "decimated.spz", "refined.spz"))
        import gzip
        import torch
        from spz_amd import abi, device as D
        stream = D.encode(D.to_device(make_cloud_clustered(n, 3, 1234), torch.device("cuda:0")), n, 3, False, abi.RUB, 3)
        torch.cuda.synchronize()
        with open(big, "wb") as f:
            f.write(gzip.compress(stream.cpu().numpy().tobytes(), 1))
        del stream
        torch.cuda.empty_cache()
        _, kept = spz.decimate_spz(big, dec, target_points=n // 10)
        tool = os.path.join(ROOT, "spz_amd", "bin", "spz_refine")
        cmd = [tool, dec, big, out, "--orbit", "8", "--size", str(a.width), str(a.height), "--fov-y", "50", "--center",
               "0", "0", "0", "--radius", "11.6", "--iters", str(a.iters)]
        times, last = [], ""
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            times.append(time.perf_counter() - t0)
            assert r.returncode == 0, (r.stdout, r.stderr)
            last = r.stdout
        mean = [ln for ln in last.split("\n") if ln.startswith("mean psnr")][0].split()
        loss = [ln for ln in last.split("\n") if ln.startswith("loss ")][0].split()
        return {"tool": "refine_bench", "mode": "e2e", "points": n, "decimated_points": int(kept), "views": 8,
                "width": a.width, "height": a.height, "iterations": a.iters, "runs": a.reps,
                "wall_s": spread(times), "mean_psnr_before": round(float(mean[2]), 3),
                "mean_psnr_after": round(float(mean[4]), 3), "mean_ssim_before": round(float(mean[6]), 4),
                "mean_ssim_after": round(float(mean[8]), 4), "loss_first": float(loss[1]), "loss_last": float(loss[3]),
                "bytes": {"scene": os.path.getsize(big), "decimated": os.path.getsize(dec),
                          "refined": os.path.getsize(out)},
                "note": "a synthetic scene ranks the edits here; it does not predict a capture's gain"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--trace", default=None, help="a rocpd .db of a traced run to summarise")
    ap.add_argument("--tolerance", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--collect", nargs="+", default=None)
    ap.add_argument("--densify", action="store_true")
    ap.add_argument("--collect-densify", nargs="+", default=None)
    a = ap.parse_args()
    if a.trace:
        out = trace_summary(a.trace)
        out["points"] = a.points
    elif a.tolerance:
        out = tolerance_ratios()
    elif a.e2e:
        out = e2e(a)
    elif a.collect:
        out = collect(a.collect)
    elif a.collect_densify:
        out = collect_densify(a.collect_densify)
    elif a.densify:
        out = densify(a)
    else:
        out = events(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
