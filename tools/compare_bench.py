#!/usr/bin/env python3
"""compare_bench.py — image metrics and compare (DESIGN §8 "Compare") measured in THIS process (run it in a fresh one).

Timing:
  kernel     spz_amd.device.image_metrics (the tile kernel + the slab reduction, map written) on two RGBA images at
             1920x1080 and 3840x2160, device events, median over --reps;
  file       spz.compare_spz of a 10 M-point SH3 clustered scene (make_cloud_clustered) against its decimate_spz copy at
             1 M points, 32 orbit views at 1920x1080: read, inflate both, 2 x 32 renders, 32 metrics, wall clock, median;
  host route per view render_spz x 2 (images downloaded), then the float64 numpy restatement (tests/metrics_ref.py),
             over --host-views views, wall clock per view.
Quality, on a 200 k-point SH3 clustered scene: 8 orbit views at 640x360; mean PSNR and SSIM of decimate_spz (target
points), prune_spz (keep_fraction, scored over 24 other views) and filter_spz to SH0 against the full file.
Prints one JSON line (--out: also writes it).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def gz(raw):
    co = zlib.compressobj(6, zlib.DEFLATED, 16 + 15)
    return co.compress(raw) + co.flush()


def make_file(td, name, n, seed):
    import torch
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered
    c = make_cloud_clustered(n, 3, seed)
    stream = D.encode(D.to_device(c, torch.device("cuda:0")), n, 3, False, abi.RUB, 3)
    torch.cuda.synchronize()
    path = os.path.join(td, name)
    with open(path, "wb") as f:
        f.write(gz(stream.cpu().numpy().tobytes()))
    del stream
    torch.cuda.empty_cache()
    return path


def kernel_ms(w, h, reps):
    import torch
    from spz_amd import device as D
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.rand((h, w, 4), device=dev, generator=g)
    b = (a + 0.05 * torch.randn((h, w, 4), device=dev, generator=g)).contiguous()
    m = torch.empty((h, w), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)
    out = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        D.image_metrics(a, b, ssim_map=m)
        e1.record(st)
        e1.synchronize()
        if r >= 3:
            out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def timing(td, a):
    import spz_amd.spz as spz
    import metrics_ref as MR
    n = a.points
    big = make_file(td, "big.spz", n, 1234)
    dec = os.path.join(td, "big_dec.spz")
    used = spz.decimate_spz(big, dec, target_points=n // 10)
    views = spz.orbit_views(32, width=1920, height=1080, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=11.6,
                            distance=2.5)
    files = []
    for r in range(a.file_reps + 1):
        t0 = time.perf_counter()
        got = spz.compare_spz(big, dec, views, coord=spz.RUB)
        if r:
            files.append((time.perf_counter() - t0) * 1e3)
    host = []
    for v in views[: a.host_views]:
        t0 = time.perf_counter()
        kw = dict(v, coord=spz.RUB)
        ia, ib = spz.render_spz(big, **kw), spz.render_spz(dec, **kw)
        MR.metrics(ia, ib)
        host.append((time.perf_counter() - t0) * 1e3)
    fm = statistics.median(files)
    return {
        "kernel_1920x1080_median_ms": kernel_ms(1920, 1080, a.reps),
        "kernel_3840x2160_median_ms": kernel_ms(3840, 2160, a.reps),
        "points": n, "decimated_points": int(used[1]), "sh_degree": 3, "views": len(views), "width": 1920,
        "height": 1080,
        "compare_spz_file_to_metrics_median_ms": round(fm, 1),
        "compare_spz_per_view_ms": round(fm / len(views), 2),
        "mean_psnr_db": round(statistics.mean(m["psnr"] for m in got), 3),
        "mean_ssim": round(statistics.mean(m["ssim"] for m in got), 5),
        "host_route_views": len(host),
        "host_route_per_view_median_ms": round(statistics.median(host), 1),
        "host_route_note": "render_spz x 2 (download), then tests/metrics_ref.py in float64 numpy; file reads and "
                           "inflates are inside each render_spz call",
    }


def quality(td, a):
    import spz_amd.spz as spz
    n = a.quality_points
    path = make_file(td, "small.spz", n, 77)
    kw = dict(width=640, height=360, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=11.6)
    scoring = spz.orbit_views(24, distance=2.5, **kw)
    held = spz.orbit_views(8, distance=2.8, **kw)
    out = os.path.join(td, "edited.spz")

    def score(label, kept):
        m = spz.compare_spz(path, out, held, coord=spz.RUB)
        return {"edit": label, "kept": int(kept), "psnr_db": round(statistics.mean(x["psnr"] for x in m), 2),
                "ssim": round(statistics.mean(x["ssim"] for x in m), 4)}

    rows = []
    for frac in (0.5, 0.34, 0.2):
        _, pts = spz.decimate_spz(path, out, target_points=int(n * frac))
        rows.append(score(f"decimate target {frac}", pts))
        kept = spz.prune_spz(path, out, scoring, keep_fraction=frac, coord=spz.RUB)
        rows.append(score(f"prune keep_fraction {frac}", kept))
    spz.filter_spz(path, out, sh_degree=0)
    rows.append(score("filter sh_degree 0", n))
    return {"points": n, "sh_degree": 3, "views": len(held), "width": 640, "height": 360, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--quality-points", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--file-reps", type=int, default=2)
    ap.add_argument("--host-views", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    out = {"tool": "compare_bench", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as td:
        out["timing"] = timing(td, a)
        out["quality"] = quality(td, a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
