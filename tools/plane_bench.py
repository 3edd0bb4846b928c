#!/usr/bin/env python3
"""plane_bench.py — the plane detector (DESIGN §8 "Level") on a synthetic room: half of the points on a tilted floor with
+-2 grid steps of noise, the rest clutter above it, SH0, 12 fractional bits, seeded.

After a warm-up of each, in THIS process (device events around work on the current stream):
  score     spz_amd_plane_score_device alone (planes already in device memory): the score kernel and its small reduce,
            at --hypotheses planes x --points, --reps times; the achieved vector-operation rate is points x planes x
            --valu-per-test (the instruction count of one point-plane test in the kernel's .s, 8.5 as built: three
            v_fma_f64, one v_cmp, three v_cndmask, half a v_add3_u32, one v_add_f64) over that time
  torch     the same scoring as torch int64 tensor operations on the same device, on --torch-planes planes (64 planes x
            the points are 512 MB of int64 at 1 M points), scaled to --hypotheses and marked as scaled; its K and S are
            compared with the kernel's on those planes
  resident  spz_amd.device.detect_planes_packed on the stream in device memory: wall time and the stages
  level     spz.level_spz(file) -> placement, wall time (inflate + the run)
  cpu       what a user does today: load_spz -> numpy RANSAC (f64 distances of every point to --cpu-hypotheses planes of
            random triples, count and sum of the inliers), one timed run, scaled to --hypotheses and marked as scaled
Prints one JSON line (--out: also appends it)."""
import argparse
import json
import math
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MAGIC = 0x5053474E
TAU = 0.001


def room_stream(n, seed):
    """A raw v3 SH0 stream of n points and the floor's true normal."""
    rng = np.random.default_rng(seed)
    half, step = 2.0, 2.0 ** -12
    nf = n // 2
    floor = np.stack([rng.uniform(-half, half, nf), rng.integers(-2, 3, nf) * step, rng.uniform(-half, half, nf)], 1)
    clutter = np.stack([rng.uniform(-half, half, n - nf), rng.uniform(0.05, 2.5, n - nf),
                        rng.uniform(-half, half, n - nf)], 1)
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(0.6) * K + (1 - math.cos(0.6)) * (K @ K)
    pts = np.concatenate([floor, clutter])[rng.permutation(n)] @ Rm.T
    f = np.rint(pts * 4096.0).astype(np.int64) & 0xFFFFFF
    pos = np.stack([(f >> s) & 0xFF for s in (0, 8, 16)], axis=2).astype(np.uint8).reshape(-1)
    rest = rng.integers(0, 256, n * (1 + 3 + 3 + 4), dtype=np.uint8)
    raw = struct.pack("<IIIBBBB", MAGIC, 3, n, 0, 12, 0, 0) + pos.tobytes() + rest.tobytes()
    return raw, Rm @ np.array([0.0, 1.0, 0.0])


def event_ms(torch, fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(round(ev[0].elapsed_time(ev[1]), 4))
    return statistics.median(out), out


def torch_score(torch, P, planes, T):
    """K and S of every plane as int64 tensor operations, 32 planes at a time."""
    Ks, Ss = [], []
    for s in range(0, planes.shape[0], 32):
        q = planes[s:s + 32]
        d = (P[:, 0:1] * q[:, 0] + P[:, 1:2] * q[:, 1] + P[:, 2:3] * q[:, 2] - q[:, 3]).abs()
        inl = d <= T
        Ks.append(inl.sum(0))
        Ss.append((d * inl).sum(0))
    return torch.cat(Ks), torch.cat(Ss)


def cpu_ransac(P, hypotheses, tau, seed):
    rng = np.random.default_rng(seed)
    best = (math.inf, None)
    for _ in range(hypotheses):
        a, b, c = P[rng.integers(0, P.shape[0], 3)]
        nrm = np.cross(b - a, c - a)
        L = np.linalg.norm(nrm)
        if L == 0.0:
            continue
        nrm = nrm / L
        d = np.abs(P @ nrm - a @ nrm)
        inl = d <= tau
        K = int(inl.sum())
        cost = float(d[inl].sum()) + tau * (P.shape[0] - K)
        if cost < best[0]:
            best = (cost, nrm)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--hypotheses", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valu-per-test", type=float, default=8.5)
    ap.add_argument("--torch-planes", type=int, default=64)
    ap.add_argument("--cpu-hypotheses", type=int, default=16)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    if not torch.cuda.is_available():
        raise SystemExit("plane_bench.py needs a GPU")
    L = abi.load_library()
    n, H = a.points, a.hypotheses
    res = {"points": n, "hypotheses": H, "reps": a.reps, "threshold": TAU, "valu_per_test": a.valu_per_test}
    raw, normal = room_stream(n, 2026)
    stream_t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    hdr = abi.peek_header(raw)[1]
    T = D.plane_threshold(TAU, 12)
    # ---- the score kernel ----
    prep = D.plane_prepare(stream_t, hdr)
    ws, m = prep
    idx = np.zeros(3 * H, np.uint32)
    abi.check(L.spz_amd_plane_hypotheses(0, 0, H, m, None, None, 0.0, idx.ctypes.data, None), "indices")
    sampled = D.plane_gather(prep, hdr, idx.astype(np.int64)).cpu().numpy()
    planes_c = (abi.Plane * H)()
    abi.check(L.spz_amd_plane_hypotheses(0, 0, H, m, np.ascontiguousarray(sampled).ctypes.data, None, 0.0, None,
                                         planes_c), "hypotheses")
    planes_t = torch.frombuffer(bytearray(bytes(planes_c)), dtype=torch.uint8).to("cuda")
    scores = torch.empty((H, 3), dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def score():
        abi.check(L.spz_amd_plane_score_device(ws.data_ptr(), n, m, planes_t.data_ptr(), H, T, scores.data_ptr(), st),
                  "score")
    score()
    torch.cuda.synchronize()
    res["score_ms"], res["score_laps_ms"] = event_ms(torch, score, a.reps)
    tests = float(m) * H
    res["score_tests_per_s"] = tests / (res["score_ms"] * 1e-3)
    res["score_valu_ops_per_s"] = tests * a.valu_per_test / (res["score_ms"] * 1e-3)
    cost = torch.where(scores[:, 2] < 0, torch.iinfo(torch.int64).max, scores[:, 2])   # UINT64_MAX: invalid
    best = int(torch.argmin(cost).item())
    res["best"] = {"h": best, "K": int(scores[best, 0]), "S": int(scores[best, 1])}
    # ---- the same scoring as torch integer ops ----
    Ht = min(a.torch_planes, H)
    planes_np = np.array([(p.a, p.b, p.c, p.e) for p in planes_c[:Ht]], np.int64)
    f = np.frombuffer(raw, np.uint8, 9 * n, 16).reshape(n, 3, 3).astype(np.int64)
    P_np = f[:, :, 0] | (f[:, :, 1] << 8) | (f[:, :, 2] << 16)
    P_np = np.where(P_np >= 1 << 23, P_np - (1 << 24), P_np)
    P_t, q_t = torch.from_numpy(P_np).to("cuda"), torch.from_numpy(planes_np).to("cuda")
    Kt, St = torch_score(torch, P_t, q_t, T)
    valid = (q_t[:, :3] != 0).any(1)
    same = bool(torch.equal(Kt[valid], scores[:Ht, 0][valid]) and torch.equal(St[valid], scores[:Ht, 1][valid]))
    res["torch_agrees"] = same
    ms, laps = event_ms(torch, lambda: torch_score(torch, P_t, q_t, T), max(2, a.reps // 2))
    res["torch_planes"], res["torch_ms"], res["torch_laps_ms"] = Ht, ms, laps
    res["torch_ms_scaled_to_hypotheses"] = {"value": ms * H / Ht, "scaled": True, "from_planes": Ht}
    del P_t, q_t
    # ---- the resident run ----
    D.detect_planes_packed(stream_t, hdr, threshold=TAU, hypotheses=H)
    walls, stages, r = [], [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = D.detect_planes_packed(stream_t, hdr, threshold=TAU, hypotheses=H)
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        stages.append([round(x, 3) for x in r["ms"]])
    p = r["planes"][0]
    res["resident_ms"], res["resident_laps_ms"] = statistics.median(walls), walls
    res["resident_stage_ms"] = {"prepare_gather": statistics.median(s[0] for s in stages),
                                "score": statistics.median(s[1] for s in stages),
                                "moments_solves_marks": statistics.median(s[2] for s in stages), "laps": stages}
    res["plane"] = {"integers": p["integers"], "inliers": p["inliers"], "fitness": p["fitness"],
                    "refinements": p["refinements"],
                    "angle_to_truth_rad": math.acos(min(1.0, abs(float(np.array(p["normal"]) @ normal))))}
    del stream_t
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "room.spz")
        if not a.skip_file or not a.skip_cpu:
            co = zlib.compressobj(1, zlib.DEFLATED, 31)
            with open(path, "wb") as fh:
                fh.write(co.compress(raw) + co.flush())
            res["gzip_bytes"] = os.path.getsize(path)
        # ---- file -> placement ----
        if not a.skip_file:
            spz.level_spz(path, threshold=TAU, hypotheses=H)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                lr = spz.level_spz(path, threshold=TAU, hypotheses=H)
                t.append(round((time.perf_counter() - t0) * 1e3, 3))
            res["level_spz_ms"], res["level_spz_laps_ms"] = statistics.median(t), t
            res["level_spz_stage_ms"] = [round(x, 3) for x in lr["ms"]]
        # ---- load -> numpy RANSAC on the host ----
        if a.skip_cpu:
            res["cpu"] = "skipped"
        else:
            t0 = time.perf_counter()
            cloud = spz.load_spz(path)
            P = np.asarray(cloud.positions, np.float64).reshape(-1, 3)
            load_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            cost, nrm = cpu_ransac(P, a.cpu_hypotheses, TAU, 1)
            ransac_ms = (time.perf_counter() - t0) * 1e3
            res["cpu_load_ms"], res["cpu_hypotheses"], res["cpu_ransac_ms"] = round(load_ms, 1), a.cpu_hypotheses, round(ransac_ms, 1)
            res["cpu_ms_scaled_to_hypotheses"] = {"value": round(load_ms + ransac_ms * H / a.cpu_hypotheses, 1),
                                                  "scaled": True, "from_hypotheses": a.cpu_hypotheses}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
