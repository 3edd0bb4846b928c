#!/usr/bin/env python3
"""prune_bench.py — significance pruning (DESIGN §8 "Prune") measured in THIS process (run it in a fresh one).

Timing, on a 10 M-point SH3 clustered scene (make_cloud_clustered) and 32 orbit views at 1920x1080:
  per view   from one prepared state (spz_amd_render_prepare_packed_device), the plain render's finish step
             (spz_amd_render_finish_device: tile entries, their sort, ranges, blend) against the score step
             (spz_amd_render_score_device: the same entries, sort and ranges, then the scoring blend), each timed with
             device events, median over the views;
  file       spz.prune_spz(path -> path, 32 views, keep_fraction 0.34): read, inflate, 32 scored views, rank, subset,
             gzip, write;
  host route load -> numpy -> a renderer -> save is not run: render_cloud returns pixels, not per-Gaussian weights, so a
             host route needs a third-party rasteriser with weight accumulation; only its load + save (the requantising
             round trip) is timed, for scale.
Quality, on a 200 k-point SH3 clustered scene: 24 orbit views score it, 8 other orbit views (another Fibonacci set, at
another distance) are held out; the PSNR (RGB clamped to [0, 1]) of the held-out renders of the pruned file against the
full one after pruning 50 / 66 / 80 %, against random pruning and the filter's opacity rule (min_alpha) at the same kept
count (8-bit alphas tie, so that rule is applied as its ranking: the top K by alpha, ties by index, as a filter_spz mask).
Prints one JSON line (--out: also writes it).  --timing-only / --quality-only run one half.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

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
    raw = stream.cpu().numpy().tobytes()
    path = os.path.join(td, name)
    with open(path, "wb") as f:
        f.write(gz(raw))
    return path, stream, raw


def params_of(views, coord):
    from spz_amd import abi
    return [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"],
                              max_sh_degree=0, coord=coord) for v in views]


def timing(td, a):
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    L = abi.load_library()
    dev = torch.device("cuda:0")
    n = a.points
    path, stream, raw = make_file(td, "big.spz", n, 1234)
    rc, h = abi.peek_header(raw)
    abi.check(rc, "peek_header")
    views = spz.orbit_views(32, width=1920, height=1080, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=11.6,
                            distance=2.5)
    ps = params_of(views, abi.RUB)
    st = torch.cuda.current_stream(dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsum = torch.zeros(n, dtype=torch.int64, device=dev)
    wmax = torch.zeros(n, dtype=torch.float32, device=dev)
    prefix = int(L.spz_amd_render_workspace_bytes(n, 0)) - 256
    ws = torch.empty(prefix + 256, dtype=torch.uint8, device=dev)
    finish, score, entries = [], [], []
    for k, p in enumerate(ps):
        img = torch.empty((p.height, p.width, 4), dtype=torch.float32, device=dev)
        abi.check(L.spz_amd_render_prepare_packed_device(stream.data_ptr(), stream.numel(), C.byref(h), C.byref(p),
                                                         total.data_ptr(), None, ws.data_ptr(),
                                                         C.c_void_p(st.cuda_stream)), "prepare")
        m = int(total.cpu()[0])
        need = int(L.spz_amd_render_workspace_bytes(n, m))
        if need > ws.numel():
            bigger = torch.empty(need, dtype=torch.uint8, device=dev)
            off_a, off_b = (-ws.data_ptr()) % 256, (-bigger.data_ptr()) % 256
            bigger[off_b:off_b + prefix].copy_(ws[off_a:off_a + prefix])
            ws = bigger
        entries.append(m)
        for r in range(a.reps + 1):
            for which, out in (("finish", finish), ("score", score)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                if which == "finish":
                    rc = L.spz_amd_render_finish_device(n, C.byref(p), m, img.data_ptr(), status.data_ptr(),
                                                        ws.data_ptr(), C.c_void_p(st.cuda_stream))
                else:
                    rc = L.spz_amd_render_score_device(n, C.byref(p), m, None, wsum.data_ptr(), wmax.data_ptr(),
                                                       status.data_ptr(), ws.data_ptr(), C.c_void_p(st.cuda_stream))
                e1.record(st)
                abi.check(rc, which)
                e1.synchronize()
                if r:
                    out.append(e0.elapsed_time(e1))
    del ws
    torch.cuda.empty_cache()
    files = []
    for r in range(a.file_reps + 1):
        t0 = time.perf_counter()
        kept = spz.prune_spz(path, os.path.join(td, "big_pruned.spz"), views, keep_fraction=0.34, coord=spz.RUB)
        if r:
            files.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    g = spz.load_spz(path, spz.UnpackOptions())
    t_load = time.perf_counter() - t0
    t0 = time.perf_counter()
    spz.save_spz(g, spz.PackOptions(), os.path.join(td, "big_roundtrip.spz"))
    t_save = time.perf_counter() - t0
    fm, sm = statistics.median(finish), statistics.median(score)
    return {
        "points": n, "sh_degree": 3, "views": len(views), "width": 1920, "height": 1080, "reps": a.reps,
        "entries_per_view_median": int(statistics.median(entries)), "entries_per_view_max": int(max(entries)),
        "render_finish_per_view_median_ms": round(fm, 3),
        "score_per_view_median_ms": round(sm, 3),
        "score_over_render_finish": round(sm / fm, 3),
        "prune_spz_file_to_file_median_ms": round(statistics.median(files), 1),
        "prune_spz_kept": int(kept),
        "host_route": "not run: render_cloud returns pixels, not per-Gaussian weights; a host route needs a third-party "
                      "rasteriser that accumulates them",
        "host_route_load_plus_save_s": round(t_load + t_save, 3),
    }


def psnr(a, b):
    x = np.clip(a[..., :3], 0, 1).astype(np.float64)
    y = np.clip(b[..., :3], 0, 1).astype(np.float64)
    mse = float(((x - y) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(1.0 / mse)


def quality(td, a):
    import spz_amd.spz as spz
    n = a.quality_points
    path, _, _ = make_file(td, "small.spz", n, 77)
    W, H = 640, 360
    kw = dict(width=W, height=H, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=11.6)
    scoring = spz.orbit_views(24, distance=2.5, **kw)
    held = spz.orbit_views(8, distance=2.8, **kw)

    def renders(p):
        return [spz.render_spz(p, coord=spz.RUB, **{k: v[k] for k in ("world_to_camera", "fx", "fy", "cx", "cy",
                                                                          "width", "height")}) for v in held]

    full = renders(path)
    g = spz.load_spz(path, spz.UnpackOptions())
    alphas = np.asarray(g.alphas)
    rng = np.random.default_rng(3)
    rows = []
    for frac in (0.5, 0.34, 0.2):
        out = os.path.join(td, "pruned.spz")
        kept, mask, s, _ = spz.prune_spz(path, out, scoring, keep_fraction=frac, coord=spz.RUB, return_scores=True)
        q_sig = statistics.mean(psnr(x, y) for x, y in zip(renders(out), full))
        rmask = np.zeros(n, dtype=bool)
        rmask[rng.choice(n, kept, replace=False)] = True
        spz.filter_spz(path, out, mask=rmask)
        q_rand = statistics.mean(psnr(x, y) for x, y in zip(renders(out), full))
        order = np.lexsort((np.arange(n), -alphas))
        amask = np.zeros(n, dtype=bool)
        amask[order[:kept]] = True
        spz.filter_spz(path, out, mask=amask)
        q_alpha = statistics.mean(psnr(x, y) for x, y in zip(renders(out), full))
        rows.append({"pruned_fraction": round(1 - kept / n, 3), "kept": int(kept),
                     "psnr_significance_db": round(q_sig, 2), "psnr_random_db": round(q_rand, 2),
                     "psnr_min_alpha_db": round(q_alpha, 2)})
    return {"points": n, "sh_degree": 3, "scoring_views": len(scoring), "held_out_views": len(held), "width": W,
            "height": H, "zero_score_fraction": round(float((s == 0).mean()), 4), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--quality-points", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--file-reps", type=int, default=2)
    ap.add_argument("--timing-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    out = {"tool": "prune_bench", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as td:
        if not a.quality_only:
            out["timing"] = timing(td, a)
        if not a.timing_only:
            out["quality"] = quality(td, a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
