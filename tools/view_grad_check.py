"""Driver of `make view-grad-check`: writes the scenes of tests/test_gpu_render_grad.CASES for the host build of the
view backward's one-Gaussian chain (tools/view_grad_check.cpp, built with -fsanitize=address,undefined), runs it and
compares its 12 sums with tests/view_grad_ref.py's chain on the same float32 record gradients: 1e-12 relative.  CPU
only; the program is a stand-alone executable, nothing is preloaded into Python."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import render_grad_ref as GR  # noqa: E402
import render_ref as RR  # noqa: E402
import view_grad_ref as VR  # noqa: E402
from test_gpu_render import view_of  # noqa: E402
from spz_amd import abi  # noqa: E402

W, H = 40, 36
BG = (0.1, 0.2, 0.3)
CASES = {"sh3": (1, 3, False, 3, 4), "sh3_aa": (6, 3, True, 3, 0), "sh1_max0": (5, 1, False, 0, 0),
         "sh0": (6, 0, False, 3, 0)}


def main(binary):
    worst = 0.0
    for name, (seed, deg, aa, max_sh, hits) in CASES.items():
        cloud = GR.scene(seed, deg, clamp_hits=hits)
        n = cloud["alphas"].size
        m, fx, fy, cx, cy = view_of(cloud["positions"], width=W, height=H)
        params = abi.render_params(m, fx, fy, cx, cy, W, H, 0.2, BG, max_sh, 0)
        cam = RR.camera(m, fx, fy, cx, cy, W, H, 0.2, BG, max_sh)
        dec = GR.decisions(cloud, deg, cam, aa)
        G = np.random.default_rng(100 + seed).standard_normal((H, W, 4)).astype(np.float32)
        rg = VR.view_gradient(cloud, deg, cam, dec, G, aa)["records"].astype(np.float32)
        per = VR.chain(cloud, deg, cam, dec, rg, aa)
        want, mag = per.sum(axis=0).reshape(-1), np.abs(per).sum(axis=0).reshape(-1)
        rec = dec["rec"]
        records = np.zeros((n, 12), dtype=np.float32)
        records[:, 0:2], records[:, 2:5], records[:, 5] = rec["mean"], rec["conic"], rec["opacity"]
        records[:, 6:9], records[:, 9] = rec["rgb"], rec["depth"]
        records[:, 10:12] = rec["rect"].astype(np.uint16).view(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "scene.bin")
            with open(path, "wb") as f:
                f.write(np.array([n, deg, 1 if aa else 0, 0], dtype=np.int32).tobytes())
                f.write(bytes(params))
                for k in ("positions", "scales", "rotations", "alphas", "colors", "sh"):
                    f.write(np.asarray(cloud[k], dtype=np.float32).tobytes())
                f.write(records.tobytes())
                f.write(rg.tobytes())
            out = subprocess.run([binary, path], check=True, capture_output=True, text=True)
        if out.stderr.strip():
            print(out.stderr)
            raise SystemExit(f"{name}: the sanitizers reported")
        got = np.array([[float(x) for x in line.split()] for line in out.stdout.splitlines()])
        rel = np.abs(got[:, 0] - want) / np.abs(want)
        print(f"{name}: n = {n}, largest relative difference of the 12 sums {rel.max():.3e}; "
              f"of the sums of magnitudes {(np.abs(got[:, 1] - mag) / mag).max():.3e}")
        worst = max(worst, rel.max())
        assert np.all(rel <= 1e-12), (name, rel)
    print(f"view_grad_check ok: {len(CASES)} scenes clean under ASan + UBSan, worst relative difference {worst:.3e}")


if __name__ == "__main__":
    assert C.sizeof(abi.RenderParams) == 96
    main(sys.argv[1])
