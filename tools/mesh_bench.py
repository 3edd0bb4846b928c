#!/usr/bin/env python3
"""mesh_bench.py — the mesh feature's kernels and its file-to-mesh route (DESIGN §8 "Mesh").

  integrate  one 1920x1080 view fused into a lattice of --sizes^3 points (spz_amd_tsdf_integrate_device), timed with
             device events, against a torch restatement of the same arithmetic on the same device (what a Python user
             would otherwise write).  The maps are the analytic depth of a unit sphere, the lattice spans [-1.3, 1.3]^3.
             bytes/s counts 40 bytes per UPDATED lattice point (five planes read and written): the traffic floor.
  extract    the six-view fused sphere of the same lattice extracted (count, the read-back, emit): ms and vertices/s.
  scene      spz_amd_mesh_open on a resident synthetic SH3 clustered scene of --points points over 32 orbit views at
             1920x1080, resolution 256: wall clock and the three h_ms parts; and spz.mesh_spz + spz.save_mesh_ply of the
             same scene as a file (the gzip member inflated, the PLY written).
  quality    20 000 opaque discs on the unit sphere, 32 views, resolution 128: mean and maximum distance of the
             vertices to the sphere in voxels.  A synthetic scene ranks settings; it does not predict a capture.

Every section runs --reps laps after a warm-up in a fresh process, --processes times; the medians of the processes'
medians and their spread are reported.  Prints one JSON line (--out: also writes it).
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 1920, 1080


def sphere_maps(torch, p, dev):
    """Median and accumulated depth (H, W, 2) and an image (H, W, 4) of the unit sphere at the origin for view p."""
    M = torch.tensor(list(p.world_to_camera), dtype=torch.float64, device=dev).reshape(3, 4)
    v, u = torch.meshgrid(torch.arange(p.height, dtype=torch.float64, device=dev),
                          torch.arange(p.width, dtype=torch.float64, device=dev), indexing="ij")
    d = torch.stack([(u + 0.5 - p.cx) / p.fx, (v + 0.5 - p.cy) / p.fy, torch.ones_like(u)], dim=-1)
    c = M[:, 3]
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ c), float(c @ c) - 1.0
    disc = b * b - 4 * a * cc
    hit = disc > 0
    t = torch.where(hit, (-b - torch.sqrt(disc.clamp(min=0))) / (2 * a), torch.full_like(a, math.inf))
    depth = torch.stack([torch.where(hit, t, torch.zeros_like(t)), t], dim=-1).float().contiguous()
    world = (torch.where(hit, t, torch.zeros_like(t))[..., None] * d - c) @ M[:, :3]
    image = torch.cat([torch.where(hit[..., None], 0.5 + 0.5 * world, torch.zeros_like(world)), hit[..., None].double()],
                      dim=-1).float().contiguous()
    return depth, image


def torch_integrate(torch, grid, vol, p, depth, image):
    """The fuse of include/spz_amd.h "mesh" (median depth) in torch on the grid's device: the same operations in f64."""
    dev = grid.device
    nx, ny, nz = (int(x) for x in vol.dims)
    s = float(vol.voxel_size)
    f64 = torch.float64
    px = (float(vol.lo[0]) + torch.arange(nx, dtype=f64, device=dev) * s)[None, None, :]
    py = (float(vol.lo[1]) + torch.arange(ny, dtype=f64, device=dev) * s)[None, :, None]
    pz = (float(vol.lo[2]) + torch.arange(nz, dtype=f64, device=dev) * s)[:, None, None]
    M = [float(x) for x in p.world_to_camera]
    x = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3]
    y = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7]
    z = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11]
    ok = z > float(p.near_plane)
    u = torch.floor(float(p.fx) * (x / z) + float(p.cx))
    v = torch.floor(float(p.fy) * (y / z) + float(p.cy))
    ok &= (u >= 0) & (u < p.width) & (v >= 0) & (v < p.height)
    pix = torch.where(ok, v * p.width + u, torch.zeros_like(u)).long()
    D = depth.reshape(-1, 2)[:, 1][pix]
    ok &= torch.isfinite(D) & (D > 0)
    sdf = D.double() - z
    trunc = float(vol.truncation)
    ok &= ~(sdf < -trunc)
    d = torch.clamp(sdf / trunc, max=1.0).float()
    grid[0] += ok.float()
    grid[1] += torch.where(ok, d, torch.zeros_like(d))
    rgb = image.reshape(-1, 4)
    for c in range(3):
        grid[2 + c] += torch.where(ok, rgb[:, c][pix], torch.zeros_like(d))
    return ok


def laps(torch, fn, reps):
    fn()                                            # the warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def six_views(abi, spz):
    fy = 0.5 * H / math.tan(math.radians(50.0) / 2)
    eyes = [(3, 0.2, -0.1), (-3, 0.1, 0.2), (0.15, 3, 0.1), (-0.1, -3, 0.2), (0.2, -0.1, 3), (0.1, 0.15, -3)]
    return [abi.render_params(spz.look_at(list(map(float, e)), [0.0, 0.0, 0.0],
                                          [0.0, 0.0, 1.0] if k in (2, 3) else [0.0, 1.0, 0.0]), fy, fy, W / 2, H / 2, W, H)
            for k, e in enumerate(eyes)]


def worker_kernels(a):
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    dev = torch.device("cuda:0")
    n = a.size
    s = 2.6 / (n - 1)
    vol = abi.tsdf_volume((-1.3, -1.3, -1.3), (n, n, n), s, 4 * s)
    views = six_views(abi, spz)
    maps = [sphere_maps(torch, p, dev) for p in views]
    grid = D.tsdf_alloc(vol, dev)
    t_dev = laps(torch, lambda: D.tsdf_integrate(grid, vol, views[0], *maps[0]), a.reps)
    t_torch = laps(torch, lambda: torch_integrate(torch, grid, vol, views[0], *maps[0]), max(2, a.reps // 2))
    # the two agree: one view into fresh grids
    g1, g2 = D.tsdf_alloc(vol, dev), D.tsdf_alloc(vol, dev)
    D.tsdf_integrate(g1, vol, views[0], *maps[0])
    updated = int(torch_integrate(torch, g2, vol, views[0], *maps[0]).sum())
    equal = bool(torch.equal(g1.view(torch.int32), g2.view(torch.int32)))
    del g2
    for p, m in zip(views[1:], maps[1:]):
        D.tsdf_integrate(g1, vol, p, *m)
    t_ext = laps(torch, lambda: D.tsdf_extract(g1, vol), a.reps)
    v, _, t = D.tsdf_extract(g1, vol)
    print("WORKER " + json.dumps({"integrate_ms": t_dev, "torch_ms": t_torch, "extract_ms": t_ext, "updated": updated,
                                  "equal": equal, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]),
                                  "device": torch.cuda.get_device_name(0)}))


def worker_scene(a):
    import numpy as np
    import torch
    import zlib
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered
    dev = torch.device("cuda:0")
    n, deg = a.points, 3
    stream = D.encode(D.to_device(make_cloud_clustered(n, deg, 1234), dev), n, deg, False, abi.RUB, 3)
    torch.cuda.synchronize()
    h = D.make_header(n, deg)
    vd = spz.orbit_views(32, width=W, height=H, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=12.0)
    views = [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], W, H) for v in vd]
    wall, parts, counts = [], [], None
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        m = D.mesh_packed(stream, h, views, resolution=256)
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
            parts.append(list(m["ms"]))
        counts = (len(m["vertices"]), len(m["triangles"]), m["volume"]["dims"])
    out = {"open_wall_ms": wall, "parts_ms": parts, "vertices": counts[0], "triangles": counts[1], "dims": counts[2]}
    if a.file_route:
        with tempfile.TemporaryDirectory() as tmp:
            path, ply = os.path.join(tmp, "scene.spz"), os.path.join(tmp, "scene.ply")
            co = zlib.compressobj(1, zlib.DEFLATED, 16 + 15)
            with open(path, "wb") as f:
                f.write(co.compress(stream.cpu().numpy().tobytes()) + co.flush())
            file_ms = []
            for r in range(2):
                t0 = time.perf_counter()
                m = spz.mesh_spz(path, vd, resolution=256)
                spz.save_mesh_ply(ply, m["vertices"], m["colors"], m["triangles"])
                if r:
                    file_ms.append((time.perf_counter() - t0) * 1e3)
            out["file_to_ply_ms"] = file_ms
            out["ply_bytes"] = os.path.getsize(ply)
    print("WORKER " + json.dumps(out))


def worker_quality(a):
    import numpy as np
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    dev = torch.device("cuda:0")
    n = 20000
    k = np.arange(n) + 0.5
    zc = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - zc * zc)
    nrm = np.stack([r * np.cos(phi), r * np.sin(phi), zc], axis=1)
    axis = np.cross([0.0, 0.0, 1.0], nrm)
    sn = np.linalg.norm(axis, axis=1)
    theta = np.arctan2(sn, nrm[:, 2])
    axis = axis / np.maximum(sn, 1e-12)[:, None]
    q = np.concatenate([axis * np.sin(theta / 2)[:, None], np.cos(theta / 2)[:, None]], axis=1)
    cloud = {"positions": nrm.astype(np.float32).reshape(-1),
             "scales": np.tile(np.log(np.float32([0.02, 0.02, 0.002])), n).astype(np.float32),
             "rotations": q.astype(np.float32).reshape(-1), "alphas": np.full(n, 6.0, np.float32),
             "colors": (nrm * 1.2).astype(np.float32).reshape(-1), "sh": np.zeros(0, np.float32)}
    stream = D.encode(D.to_device(cloud, dev), n, 0, False, abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    abi.check(rc, "peek_header")
    vd = spz.orbit_views(32, width=640, height=480, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=1.0)
    views = [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], 640, 480) for v in vd]
    out = {}
    for kind in ("median", "expected"):
        m = D.mesh_packed(stream, h, views, resolution=128, depth=kind)
        off = np.abs(np.linalg.norm(m["vertices"].astype(np.float64), axis=1) - 1.0) / m["volume"]["voxel_size"]
        out[kind] = {"vertices": len(off), "triangles": len(m["triangles"]), "mean_voxels": round(float(off.mean()), 4),
                     "max_voxels": round(float(off.max()), 4)}
    print("WORKER " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--scene-points", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--no-file-route", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=256, help=argparse.SUPPRESS)
    ap.add_argument("--points", type=int, default=1_000_000, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.file_route = not a.no_file_route
    if a.worker:
        {"kernels": worker_kernels, "scene": worker_scene, "quality": worker_quality}[a.worker](a)
        return

    def spawn(which, *extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--reps", str(a.reps), *extra]
        if a.no_file_route:
            cmd.append("--no-file-route")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            raise SystemExit(f"worker {which} failed ({r.returncode}):\n{r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("WORKER ")][-1][7:])

    med = statistics.median
    spread = lambda xs: {"median": round(med(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    out = {"tool": "mesh_bench", "width": W, "height": H, "reps": a.reps, "processes": a.processes, "kernels": {},
           "scene": {}}
    for size in [int(x) for x in a.sizes.split(",") if x]:
        ws = [spawn("kernels", "--size", str(size)) for _ in range(a.processes)]
        i_ms, t_ms, e_ms = ([med(w[k]) for w in ws] for k in ("integrate_ms", "torch_ms", "extract_ms"))
        w = ws[-1]
        out["device"] = w["device"]
        out["kernels"][str(size)] = {
            "lattice_points": size ** 3, "updated_points": w["updated"], "integrate_ms": spread(i_ms),
            "integrate_GBps_at_40B_per_updated_point": round(40.0 * w["updated"] / med(i_ms) / 1e6, 1),
            "integrate_lattice_points_per_s": round(size ** 3 / med(i_ms) * 1e3),
            "torch_ms": spread(t_ms), "torch_over_device": round(med(t_ms) / med(i_ms), 2),
            "device_equals_torch_bits": all(x["equal"] for x in ws),
            "extract_ms": spread(e_ms), "vertices": w["vertices"], "triangles": w["triangles"],
            "extract_vertices_per_s": round(w["vertices"] / med(e_ms) * 1e3)}
    for points in [int(x) for x in a.scene_points.split(",") if x]:
        ws = [spawn("scene", "--points", str(points)) for _ in range(a.processes)]
        w = ws[-1]
        parts = [[med([p[k] for p in x["parts_ms"]]) for x in ws] for k in range(3)]
        entry = {"views": 32, "resolution": 256, "dims": w["dims"], "vertices": w["vertices"], "triangles": w["triangles"],
                 "open_wall_ms": spread([med(x["open_wall_ms"]) for x in ws]), "render_ms": spread(parts[0]),
                 "integrate_ms": spread(parts[1]), "extract_ms": spread(parts[2])}
        if a.file_route:
            entry["file_to_ply_ms"] = spread([med(x["file_to_ply_ms"]) for x in ws])
            entry["ply_bytes"] = w["ply_bytes"]
        out["scene"][str(points)] = entry
    out["quality"] = spawn("quality")
    out["quality"]["note"] = "a synthetic scene ranks settings; it does not predict a capture"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
