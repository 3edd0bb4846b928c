"""Merge bench (DESIGN "Merge"): two seeded 5 M-point SH3 files from save_spz merged into one 10 M-point file.

  * file -> file: spz.merge_spz against load_spz x 2 -> np.concatenate -> save_spz, medians of --reps runs after a
    warm-up, and how many bytes of the two output streams differ;
  * the copy-only kernel (both inputs v3 at 12 bits and SH3, no placement: every slice is a copy) through
    spz_amd.device.merge_packed, against hipMemcpyAsync device-to-device copies of the same 12 section slices (torch's
    copy_ of contiguous uint8 tensors), timed with events over --iters launches.

Writes one JSON line to stdout (and to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("positions", "scales", "rotations", "alphas", "colors", "sh")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5_000_000, help="points per input")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import spz_amd.spz as spz
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_numpy

    tmp = tempfile.mkdtemp(prefix="merge_bench_")
    paths = []
    for i in range(2):
        c = make_cloud_numpy(a.points, 3, 2025 + i)
        g = spz.GaussianCloud()
        g.sh_degree = 3
        for k in FIELDS:
            setattr(g, k, c[k])
        del c
        p = os.path.join(tmp, f"in{i}.spz")
        assert spz.save_spz(g, spz.PackOptions(), p)
        paths.append(p)
        del g
    dev_out, host_out = os.path.join(tmp, "merged.spz"), os.path.join(tmp, "host.spz")

    def device_route():
        t0 = time.perf_counter()
        spz.merge_spz(paths, dev_out)
        return time.perf_counter() - t0

    def host_route():
        t0 = time.perf_counter()
        cs = [spz.load_spz(p, spz.UnpackOptions()) for p in paths]
        g = spz.GaussianCloud()
        g.sh_degree = 3
        for k in FIELDS:
            setattr(g, k, np.concatenate([np.asarray(getattr(c, k)) for c in cs]))
        spz.save_spz(g, spz.PackOptions(), host_out)
        return time.perf_counter() - t0

    device_route()
    host_route()
    dev_s = [device_route() for _ in range(a.reps)]
    host_s = [host_route() for _ in range(a.reps)]
    with open(dev_out, "rb") as f:
        s_dev = np.frombuffer(zlib.decompress(f.read(), 31), np.uint8)
    with open(host_out, "rb") as f:
        s_host = np.frombuffer(zlib.decompress(f.read(), 31), np.uint8)
    diff = int(np.count_nonzero(s_dev != s_host)) if s_dev.size == s_host.size else -1
    lay = abi.stream_layout(2 * a.points, 3, 3)
    names = ("positions", "alphas", "colors", "scales", "rotations", "sh")
    diff_by_section = {names[s]: int(np.count_nonzero(s_dev[lay.offset[s]:lay.offset[s] + lay.bytes[s]] !=
                                                      s_host[lay.offset[s]:lay.offset[s] + lay.bytes[s]]))
                       for s in range(6)} if diff >= 0 else {}
    del s_host

    # the kernel against device-to-device copies of the same slices
    cuda = torch.device("cuda:0")
    ins = []
    for p in paths:
        with open(p, "rb") as f:
            ins.append(torch.frombuffer(bytearray(zlib.decompress(f.read(), 31)), dtype=torch.uint8).to(cuda))
    heads = [D.make_header(a.points, 3) for _ in ins]
    out, hdr, bad = D.merge_packed(ins, heads)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and torch.equal(out.cpu(), torch.from_numpy(s_dev.copy()))
    lin = abi.stream_layout(a.points, 3, 3)
    slices = []
    for s in range(6):
        for i in range(2):
            o = lay.offset[s] + i * lin.bytes[s]
            slices.append((out[o:o + lin.bytes[s]], ins[i][lin.offset[s]:lin.offset[s] + lin.bytes[s]]))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    ws_out = torch.empty_like(out)
    kernel_ms = timed(lambda: D.merge_packed(ins, heads, out=ws_out))
    copy_ms = timed(lambda: [d.copy_(s) for d, s in slices])
    moved = 2 * (lay.total_bytes - 16)   # read + written
    r = dict(points_per_input=a.points, sh_degree=3, reps=a.reps, stream_bytes=int(lay.total_bytes),
             merge_spz_s=statistics.median(dev_s), merge_spz_all_s=dev_s,
             host_route_s=statistics.median(host_s), host_route_all_s=host_s,
             speedup=statistics.median(host_s) / statistics.median(dev_s),
             bytes_differ_vs_host_route=diff, bytes_differ_by_section=diff_by_section,
             kernel_ms_event=kernel_ms, memcpy_12_slices_ms_event=copy_ms,
             kernel_tb_s=moved / kernel_ms / 1e9, memcpy_tb_s=moved / copy_ms / 1e9,
             note="event-timed medians include the host-side table build + upload for merge_packed")
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
