"""The depth contract without a GPU (include/spz_amd.h "render depth"; DESIGN §8 "Render"): the C ABI's signatures and
argument checks, spz_render's new usage errors, tests/depth_ref.py's tiled loop against its brute-force loop, and
spz.unproject_depth."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_ref as DR
import render_ref as RR
from conftest import ROOT


def good_params():
    from spz_amd import abi
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    return abi.render_params(m, 100.0, 100.0, 50.0, 40.0, 100, 80)


def test_signatures_resolve():
    from spz_amd import abi
    L = abi.load_library()
    for name, nargs in (("spz_amd_render_depth_device", 9), ("spz_amd_render_depth_host", 10),
                        ("spz_amd_render_depth_cloud_host", 11)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs, name


def test_bad_arguments_are_refused_before_any_device_call():
    """Every refusal below comes before the first HIP call, so it is the same with and without a device.  The pointers
    that are not NULL are never dereferenced."""
    from spz_amd import abi
    L = abi.load_library()
    p = good_params()
    some = C.c_void_p(4096)
    dev = L.spz_amd_render_depth_device
    assert dev(10, C.byref(p), 100, None, None, None, some, some, None) == abi.ERR_INVALID_ARG    # NULL depth
    assert dev(10, C.byref(p), 100, None, some, None, None, some, None) == abi.ERR_INVALID_ARG    # NULL status
    assert dev(10, C.byref(p), 100, None, some, None, some, None, None) == abi.ERR_INVALID_ARG    # NULL workspace
    assert dev(10, None, 100, None, some, None, some, some, None) == abi.ERR_INVALID_ARG
    assert dev(2 ** 31, C.byref(p), 100, None, some, None, some, some, None) == abi.ERR_INVALID_ARG
    assert dev(10, C.byref(p), 2 ** 31, None, some, None, some, some, None) == abi.ERR_CAPACITY
    for kw in (dict(fx=0.0), dict(width=0), dict(height=16385), dict(near_plane=0.0), dict(max_sh_degree=4),
               dict(coord=9)):
        q = good_params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert dev(10, C.byref(q), 100, None, some, None, some, some, None) == abi.ERR_INVALID_ARG, kw
        assert L.spz_amd_render_depth_host(some, 1 << 20, None, C.byref(q), 0, None, some, None, None,
                                           None) == abi.ERR_INVALID_ARG, kw
    # the host forms: a stream that fits its header and a cloud with its arrays, but nowhere to put the depth
    h = abi.Header(3, 100, 0, 12, 0, 0)
    size = 1 << 20
    assert L.spz_amd_render_depth_host(some, size, C.byref(h), C.byref(p), 0, None, None, None, None,
                                       None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_render_depth_host(None, size, C.byref(h), C.byref(p), 0, None, some, None, None,
                                       None) == abi.ERR_INVALID_ARG
    cl = abi.CloudPtrs(*([4096] * 6))
    assert L.spz_amd_render_depth_cloud_host(C.byref(cl), 100, 0, 0, C.byref(p), 0, None, None, None, None,
                                             None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_render_depth_cloud_host(None, 100, 0, 0, C.byref(p), 0, None, some, None, None,
                                             None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_render_depth_cloud_host(C.byref(cl), 100, 4, 0, C.byref(p), 0, None, some, None, None,
                                             None) == abi.ERR_INVALID_ARG


def test_python_layer_refuses_a_bad_camera_before_reading_the_file(tmp_path):
    import spz_amd.spz as spz
    m = RR.look_at([0, 0, -30], [0, 0, 0], [0, 1, 0])
    bad = m.copy()
    bad[0, 0] *= 1.01
    for kw in (dict(world_to_camera=bad), dict(fx=-1.0), dict(width=0), dict(height=16385), dict(near=0.0),
               dict(max_sh_degree=4)):
        args = dict(world_to_camera=m, fx=100.0, fy=100.0, cx=50.0, cy=50.0, width=100, height=100)
        args.update(kw)
        with pytest.raises(ValueError):
            spz.render_depth_spz(str(tmp_path / "missing.spz"), **args)
        with pytest.raises(ValueError):
            spz.render_depth_cloud(spz.GaussianCloud(), **args)


def test_cli_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_render")
    src, out = str(tmp_path / "missing.spz"), str(tmp_path / "o.ppm")
    base = [src, out, "--size", "64", "48", "--fov-y", "60", "--eye", "0", "0", "-5", "--target", "0", "0", "0"]
    cases = [
        base + ["--depth", str(tmp_path / "d.png")],                    # not a .pfm
        base + ["--depth"],
        base + ["--depth", str(tmp_path / "d.pfm"), "--depth-kind", "mean"],
        base + ["--depth-kind", "median"],                              # no --depth
        base + ["--depth", str(tmp_path / "d.pfm"), "--depth", str(tmp_path / "e.pfm")],
        base + ["--ids"],
        base + ["--pick", "64", "0"],                                   # outside the 64 x 48 image
        base + ["--pick", "0", "48"],
        base + ["--pick", "3", "3", "--pick", "-1", "0"],
        base + ["--pick", "3"],
        base + ["--pick", "3.5", "2"],
    ]
    for args in cases:
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "Usage: spz_render" in r.stderr and "--depth FILE.pfm" in r.stderr, args
        assert r.stdout == ""


def test_tiled_loop_equals_the_bruteforce_loop():
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(40, 1, 9)
    c["positions"] = (c["positions"] * 0.08).astype(np.float32)                  # stacked closely: medians exist
    c["scales"] = (c["scales"] * 0.25 - 1.2).astype(np.float32)
    c["alphas"] = np.minimum(c["alphas"] * 0.5 + 1.5, -1.0).astype(np.float32)  # opacity < 0.27: beyond 3 sigma a < 1/255
    m = RR.look_at([0.5, 0.8, -8.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    for aa in (False, True):
        cam = RR.camera(m, 70.0, 66.0, 41.0, 27.0, 83, 50, max_sh_degree=1)
        t, b = DR.render_depth(c, 1, cam, aa), DR.render_depth_bruteforce(c, 1, cam, aa)
        assert (t["alpha"] > 0).mean() > 0.05
        assert np.array_equal(t["index"], b["index"]) and np.array_equal(t["median"], b["median"])
        for k in ("accumulated", "alpha", "gap"):
            assert np.allclose(t[k], b[k], rtol=0, atol=1e-12), k
        # the colour blend's alpha, and the maps' own invariants
        assert np.allclose(t["alpha"], RR.render(c, 1, cam, aa)[..., 3], rtol=0, atol=1e-12)
        has = t["index"] >= 0
        assert np.unique(t["index"][has]).size >= 10
        assert np.all(np.isposinf(t["median"][~has])) and np.all(t["alpha"][has] > 0.5)
        rec = RR.preprocess(c, 1, cam, aa)
        assert np.array_equal(t["median"][has], rec["depth"][t["index"][has]])
        e = DR.expected(t)
        seen = t["alpha"] > 0
        z = rec["depth"][rec["visible"]].astype(np.float64)
        assert np.all(np.isposinf(e[~seen])) and e[seen].min() >= z.min() - 1e-9 and e[seen].max() <= z.max() + 1e-9


def test_median_of_two_stacked_gaussians():
    """Opacity 0.4 in front of opacity 0.6 at the pixel under both centres: T' = 0.6 after the first (no median yet),
    0.24 after the second, which is the median; D = 0.4 z0 + 0.6 * 0.6 z1."""
    def one(z, opacity):
        return {"positions": np.float32([0, 0, z]), "scales": np.float32([-1.0] * 3), "rotations": np.float32([0, 0, 0, 1]),
                "alphas": np.float32([np.log(opacity / (1 - opacity))]), "colors": np.float32([0, 0, 0]),
                "sh": np.zeros(0, np.float32)}
    a, b = one(8.0, 0.6), one(5.0, 0.4)
    c = {k: np.concatenate([a[k], b[k]]) for k in a}
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    cam = RR.camera(m, 50.0, 50.0, 32.5, 24.5, 64, 48)
    t = DR.render_depth(c, 0, cam)
    assert t["index"][24, 32] == 0 and t["median"][24, 32] == np.float32(8.0)
    assert np.isclose(t["accumulated"][24, 32], 0.4 * 5.0 + 0.6 * 0.6 * 8.0, atol=1e-6)
    assert np.isclose(t["gap"][24, 32], 0.1, atol=1e-6)
    assert t["index"][0, 0] == -1 and t["accumulated"][0, 0] == 0


def test_unproject_depth_round_trips_projected_points():
    import spz_amd.spz as spz
    rng = np.random.default_rng(3)
    m = RR.look_at([1.0, -2.0, -9.0], [0.2, 0.1, 0.0], [0.0, 1.0, 0.0]).astype(np.float64)
    fx, fy, cx, cy, w, h = 90.0, 85.0, 31.0, 22.5, 64, 48
    # one world point on the ray through the centre of each chosen pixel
    v, u = np.nonzero(rng.random((h, w)) < 0.1)
    z = rng.uniform(2.0, 20.0, u.size)
    cam = np.stack([(u + 0.5 - cx) / fx * z, (v + 0.5 - cy) / fy * z, z], axis=1)
    world = (cam - m[:, 3]) @ m[:, :3]
    # project them as the render contract does: the mean in pixel-index units is fx x / z + cx - 0.5
    pc = world @ m[:, :3].T + m[:, 3]
    assert np.allclose(fx * pc[:, 0] / pc[:, 2] + cx - 0.5, u, atol=1e-3)  # R is float32: orthonormal to 1e-7
    assert np.allclose(fy * pc[:, 1] / pc[:, 2] + cy - 0.5, v, atol=1e-3)
    depth = np.full((h, w), np.inf, np.float32)
    depth[v, u] = pc[:, 2]
    got = spz.unproject_depth(depth, m, fx, fy, cx, cy)
    assert got.shape == (u.size, 3) and got.dtype == np.float64
    assert np.allclose(got, world, rtol=0, atol=1e-5)  # the depths went through float32
    assert spz.unproject_depth(np.full((3, 4), np.inf), m, fx, fy, cx, cy).shape == (0, 3)
    assert spz.unproject_depth(np.full((3, 4), np.nan), m, fx, fy, cx, cy).shape == (0, 3)
    with pytest.raises(ValueError):
        spz.unproject_depth(np.zeros(5), m, fx, fy, cx, cy)
    with pytest.raises(ValueError):
        spz.unproject_depth(np.zeros((3, 4)), np.eye(3), fx, fy, cx, cy)


def test_depth_bench_declares_only_what_a_baseline_library_has():
    """tools/depth_bench.py times the colour blend through another build's library, which may lack the depth functions:
    its loader asks the library for spz_amd_render_host alone."""
    import importlib.util
    from spz_amd import abi
    spec = importlib.util.spec_from_file_location("depth_bench", os.path.join(ROOT, "tools", "depth_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class OnlyRenderHost:
        def __init__(self, lib):
            self.spz_amd_render_host = lib.spz_amd_render_host

    # any other attribute of the handle raises AttributeError
    B = bench.baseline_library(abi.LIB_PATH, loader=lambda path: OnlyRenderHost(C.CDLL(path)))
    assert B.spz_amd_render_host.restype is C.c_int and len(B.spz_amd_render_host.argtypes) == 8
    assert B.spz_amd_render_host(None, 0, None, None, 0, None, None, None) == abi.ERR_INVALID_ARG
