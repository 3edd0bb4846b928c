"""Measurements of the tile operation (DESIGN §8 "Tile") on one GPU -> one JSON object (--out FILE, else stdout).

  tree:  a seeded 10 M-point SH3 clustered scene, caps 4096 and 65536: tile count, leaves, depth, distinct content
         levels, and spz_amd_tile_open's wall-clock laps (sort / tree / decimates / bounds + emit), median of --reps.
  emit:  the batched bounds + emit of the leaves (one spz_amd_tile_content_device call: work list, bounds, emit) against
         the loop it replaces, one spz_amd_subset_device launch per leaf over the same ranges; HIP events, median of 20.
  files: spz_tile file -> directory in a fresh process per run with SPZ_AMD_TILE_TIMING=1: wall time and the stages
         (inflate; sort / tree / decimates / emit; download; gzip; write), at both caps, and at cap 4096 once more with
         the container stage held to one thread.  Cap 4096 gives members of 0.27 MB (zlib on 16 threads), cap 65536
         members of 4 MB (compressGzipped's routes, one after the other).
  host:  the route without this operation: zlib inflate, the numpy Morton order, then per tile filter_spz with the
         tile's indices (a leaf) or decimate_spz + filter_spz (a coarse tile), each a file -> file call.  A sample of
         tiles is timed and scaled to the tile count; the json says how many.
  cuts:  a 200 k-point SH3 clustered scene, cap 4096, 8 orbit views at 640x360: for max_pixel_error 1, 2, 4, 8, 16 the
         fraction of points in each view's cut and compare_spz PSNR / SSIM of merge_spz(cut) against the full file.
  --trace-workload runs only two spz_amd_tile_open calls per cap (under rocprofv3 --kernel-trace --stats);
  --format-trace FILE prints the kernel table of that run's *_results.db (or *_kernel_stats.csv)."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from oracle.pyoracle import Oracle  # noqa: E402
from spz_amd import abi, device as D  # noqa: E402
from spz_amd.synth import make_cloud_clustered  # noqa: E402


def events_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


ROOT = __file__.rsplit("/tools/", 1)[0]


def gz(raw):
    co = zlib.compressobj(6, zlib.DEFLATED, 16 + 15)
    return co.compress(raw) + co.flush()


def write_scene(td, name, n, seed):
    raw = Oracle().pack(make_cloud_clustered(n, 3, seed), n, 3, False, 0).tobytes()
    path = os.path.join(td, name)
    with open(path, "wb") as f:
        f.write(gz(raw))
    return path, raw


def run_tool(src, out, cap, threads=None):
    env = dict(os.environ, SPZ_AMD_TILE_TIMING="1")
    if threads:
        env["SPZ_AMD_TILE_GZIP_THREADS"] = str(threads)
    t0 = time.perf_counter()
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tile"), src, out, "--max-points", str(cap),
                        "--max-tiles", str(1 << 20)], capture_output=True, text=True, env=env, timeout=900)
    wall = (time.perf_counter() - t0) * 1e3
    assert r.returncode == 0, r.stderr
    stages = {m.group(1): float(m.group(2)) for m in re.finditer(r"\[tileSpz\] (\S+)\s+([0-9.]+) ms", r.stderr)}
    nbytes = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    return {"wall_ms": round(wall, 1), "stages_ms": stages, "files": len(os.listdir(out)), "bytes_written": nbytes}


def files_section(td, src):
    out = {}
    for cap, threads in ((4096, None), (65536, None), (4096, 1)):
        d = os.path.join(td, f"tiles_{cap}_{threads or 16}")
        if cap == 4096 and threads is None:
            run_tool(src, d + "_warm", cap)   # the process start, the page cache
        e = run_tool(src, d, cap, threads)
        e["container_threads"] = threads or 16
        out[f"cap_{cap}" + ("_one_thread" if threads else "")] = e
    return out


def morton_order_numpy(raw, n):
    p = np.frombuffer(raw, np.uint8, 9 * n, 16).reshape(n, 9).astype(np.uint64)
    hi, lo = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for a in range(3):
        u = (p[:, 3 * a] | (p[:, 3 * a + 1] << np.uint64(8)) | (p[:, 3 * a + 2] << np.uint64(16))) ^ np.uint64(0x800000)
        for b in range(24):
            k = 3 * b + a
            bit = (u >> np.uint64(b)) & np.uint64(1)
            if k < 48:
                lo |= bit << np.uint64(k)
            else:
                hi |= bit << np.uint64(k - 48)
    return np.lexsort((lo, hi)).astype(np.uint32)


def host_section(td, src, table, sample):
    import spz_amd.spz as spz
    t0 = time.perf_counter()
    with open(src, "rb") as f:
        raw = zlib.decompress(f.read(), 31)
    inflate_ms = (time.perf_counter() - t0) * 1e3
    n = int(np.frombuffer(raw, "<u4", 1, 8)[0])
    t0 = time.perf_counter()
    order = morton_order_numpy(raw, n)
    sort_ms = (time.perf_counter() - t0) * 1e3
    leaves = table[table["content_level"] < 0]
    inner = table[table["content_level"] >= 0]
    pick = lambda rows: rows[np.linspace(0, len(rows) - 1, min(sample, len(rows))).astype(int)]
    out_file, dec_file = os.path.join(td, "host_tile.spz"), os.path.join(td, "host_dec.spz")
    leaf_ms, inner_ms = [], []
    for r in pick(leaves):
        t0 = time.perf_counter()
        spz.filter_spz(src, out_file, indices=order[int(r["range_begin"]):int(r["range_end"])])
        leaf_ms.append((time.perf_counter() - t0) * 1e3)
    for r in pick(inner):
        t0 = time.perf_counter()
        spz.decimate_spz(src, dec_file, level=int(r["content_level"]))
        b = int(r["content_begin"])
        spz.filter_spz(dec_file, out_file, indices=np.arange(b, b + int(r["num_points"]), dtype=np.uint32))
        inner_ms.append((time.perf_counter() - t0) * 1e3)
    lm, im = statistics.median(leaf_ms), statistics.median(inner_ms) if inner_ms else 0.0
    return {"inflate_ms": round(inflate_ms, 1), "numpy_morton_order_ms": round(sort_ms, 1),
            "leaves_timed": len(leaf_ms), "coarse_tiles_timed": len(inner_ms),
            "per_leaf_filter_spz_median_ms": round(lm, 1), "per_coarse_tile_decimate_filter_median_ms": round(im, 1),
            "scaled_total_ms": round(inflate_ms + sort_ms + lm * len(leaves) + im * len(inner), 1),
            "note": "a sample of tiles timed and scaled to the tile count; every call reads the 10 M-point file again, as "
                    "a script over the file tools would; the tree itself (which ranges, which levels) is taken from the "
                    "device's table and not charged"}


def cuts_section(td, n):
    import spz_amd.spz as spz
    path, _ = write_scene(td, "small.spz", n, 77)
    ts = spz.tile_spz(path, os.path.join(td, "small_tiles"), max_points=4096)
    views = spz.orbit_views(8, width=640, height=360, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=11.6, distance=2.8)
    merged = os.path.join(td, "cut.spz")
    rows = []
    for err in (1.0, 2.0, 4.0, 8.0, 16.0):
        frac, psnr, ssim, count = [], [], [], []
        for v in views:
            cut = spz.select_tiles(ts, v["world_to_camera"], v["fx"], v["fy"], err)
            spz.merge_spz([os.path.join(td, "small_tiles", ts["tiles"][i]["file"]) for i in cut], merged)
            m = spz.compare_spz(path, merged, [v], coord=spz.RUB)[0]
            frac.append(sum(ts["tiles"][i]["num_points"] for i in cut) / n)
            count.append(len(cut))
            psnr.append(m["psnr"])
            ssim.append(m["ssim"])
        rows.append({"max_pixel_error": err, "tiles_in_cut": round(statistics.mean(count), 1),
                     "fraction_of_points": round(statistics.mean(frac), 4),
                     "psnr_db": round(statistics.mean(min(p, 99.0) for p in psnr), 2), "ssim": round(statistics.mean(ssim), 4)})
    return {"points": n, "sh_degree": 3, "cap": 4096, "tiles": len(ts["tiles"]), "views": len(views), "width": 640,
            "height": 360, "psnr_note": "an identical image counts as 99 dB in the mean", "rows": rows,
            "caveat": "a synthetic scene does not predict a capture's loss; coarse tiles inherit the decimate's quality"}


def format_trace(path):
    """The kernel table of a rocprofv3 run: its *_results.db (the `kernels` view) or its *_kernel_stats.csv."""
    if path.endswith(".db"):
        import sqlite3
        q = "select name, count(*), sum(end - start) from kernels group by name"
        rows = [(n, c, float(t)) for n, c, t in sqlite3.connect(path).execute(q)]
    else:
        with open(path, newline="") as f:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: -r[2])
    total = sum(r[2] for r in rows)
    print(f"{'kernel':<52}{'calls':>7}{'avg us':>11}{'total ms':>11}{'%':>7}")
    for name, c, t in rows:
        name = re.sub(r"\(.*$", "", name).replace("spz_amd_detail::", "").replace("void ", "")[:50]
        print(f"{name:<52}{c:>7}{t / c / 1e3:>11.1f}{t / 1e6:>11.2f}{100 * t / total:>7.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--quality-points", type=int, default=200_000)
    ap.add_argument("--host-sample", type=int, default=6)
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--format-trace")
    args = ap.parse_args()
    if args.format_trace:
        return format_trace(args.format_trace)
    L = abi.load_library()
    n = args.points
    td = tempfile.mkdtemp(prefix="tile_bench_")
    src, raw = write_scene(td, "big.spz", n, 21)
    st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    hdr = abi.peek_header(raw)[1]
    tables = {}
    res = {"points": n, "sh_degree": 3, "scene": "make_cloud_clustered seed 21", "caps": {}}
    for cap in (4096, 65536):
        laps = []
        for _ in range(2 if args.trace_workload else args.reps + 1):
            ctx, tiles, arena = C.c_void_p(), C.c_uint64(), C.c_uint64()
            ms = (C.c_float * 4)()
            rc = L.spz_amd_tile_open(st.data_ptr(), st.numel(), C.byref(hdr), cap, 1 << 20, 0, C.byref(ctx),
                                     C.byref(tiles), C.byref(arena), ms)
            abi.check(rc, "spz_amd_tile_open")
            table = np.zeros(tiles.value, np.dtype(abi.TileInfo))
            L.spz_amd_tile_table(ctx, table.ctypes.data)
            L.spz_amd_tile_close(ctx)
            laps.append(list(ms))
        laps = np.median(np.array(laps[1:]), axis=0)   # the first call warms up
        depth = np.zeros(len(table), np.int64)
        for i in range(1, len(table)):
            depth[i] = depth[table["parent"][i]] + 1
        leaves = table[table["content_level"] < 0]
        entry = {"tiles": int(len(table)), "leaves": int(len(leaves)), "depth": int(depth.max()),
                 "content_levels": sorted(set(int(l) for l in table["content_level"] if l >= 0)),
                 "arena_bytes": int(arena.value),
                 "open_ms": {"sort": float(laps[0]), "tree": float(laps[1]), "decimates": float(laps[2]),
                             "bounds_emit": float(laps[3])}}
        if args.trace_workload:
            continue
        tables[cap] = table
        # the batched emit against the per-leaf subset loop, same ranges
        table_t, summary = D.tile_tree(st, hdr, cap, 1 << 20)
        count = int(D.tile_summary(summary).num_tiles)
        order = D.morton_order(st, hdr)
        srt = D.subset(st, hdr, order)
        arena_t = torch.zeros(int(arena.value), dtype=torch.uint8, device="cuda")
        ws = torch.empty(int(L.spz_amd_tile_content_workspace_bytes(count)), dtype=torch.uint8, device="cuda")
        h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def batched():
            abi.check(L.spz_amd_tile_content_device(table_t.data_ptr(), count, -1, srt.data_ptr(), srt.numel(),
                                                    arena_t.data_ptr(), arena_t.numel(), ws.data_ptr(), h), "content")

        jobs = [(int(r["range_begin"]), int(r["num_points"]), int(r["offset"]), int(r["bytes"])) for r in leaves]
        base_o, base_a = order.data_ptr(), arena_t.data_ptr()

        def loop():
            for s, m, off, nb in jobs:
                L.spz_amd_subset_device(st.data_ptr(), st.numel(), C.byref(hdr), base_o + 4 * s, m, -1, base_a + off, nb, h)

        batched()
        want = arena_t.clone()
        arena_t.zero_()
        loop()
        torch.cuda.synchronize()
        entry["emit_same_bytes"] = bool(torch.equal(want, arena_t))
        entry["emit_ms"] = {"batched_bounds_and_emit": events_ms(batched, 20), "per_leaf_subset_loop": events_ms(loop, 20)}
        res["caps"][str(cap)] = entry
    if args.trace_workload:
        shutil.rmtree(td, ignore_errors=True)
        return
    del st
    torch.cuda.empty_cache()
    res["files"] = files_section(td, src)
    res["host_route"] = host_section(td, src, tables[65536], args.host_sample)
    res["host_route"]["ratio_to_spz_tile_cap_65536"] = round(
        res["host_route"]["scaled_total_ms"] / res["files"]["cap_65536"]["wall_ms"], 1)
    res["cuts"] = cuts_section(td, args.quality_points)
    shutil.rmtree(td, ignore_errors=True)
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
