"""Image metrics and compare without a GPU (DESIGN §8 "Compare"): tests/metrics_ref.py against a brute-force window sum
and on analytic cases (equal images, black against white, the clamping rules), the C ABI's argument checks and
workspace size, the Python layer's argument checks, and spz_compare's usage errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import metrics_ref as MR
import render_ref as RR
from conftest import ROOT


@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


def a_view(**kw):
    v = {"world_to_camera": RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), "fx": 50.0, "fy": 50.0, "cx": 32.0,
         "cy": 24.0, "width": 64, "height": 48}
    v.update(kw)
    return v


def test_window_is_a_normalised_symmetric_gaussian():
    w = MR.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15
    assert np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert math.isclose(w[4] / w[5], math.exp(-1.0 / 4.5), rel_tol=1e-15)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 17), (11, 11), (12, 5), (40, 33)])
def test_separable_equals_bruteforce(h, w):
    rng = np.random.default_rng(h * 100 + w)
    for _ in range(2):
        x = rng.random((h, w))
        assert np.allclose(MR.blur(x), MR.blur_bruteforce(x), rtol=0, atol=1e-12)
    a = rng.random((h, w, 3)).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.1, a.shape), -0.2, 1.2).astype(np.float32)
    got, gmap = MR.metrics(a, b)
    want, wmap = MR.metrics(a, b, blur_fn=MR.blur_bruteforce)
    assert abs(got["ssim"] - want["ssim"]) <= 1e-12
    assert np.max(np.abs(gmap - wmap)) <= 1e-12
    for k in ("mse", "l1", "max_abs"):
        assert got[k] == want[k]


def test_equal_images():
    rng = np.random.default_rng(3)
    a = rng.random((29, 41, 4)).astype(np.float32)
    m, s = MR.metrics(a, a[..., :3].copy())
    assert m["ssim"] == 1.0 and m["mse"] == 0.0 and m["l1"] == 0.0 and m["max_abs"] == 0.0
    assert m["psnr"] == math.inf
    assert np.all(s == 1.0)


def test_black_against_white():
    a = np.zeros((9, 14, 3), np.float32)
    b = np.ones((9, 14, 4), np.float32)
    m, _ = MR.metrics(a, b)
    assert m["mse"] == 1.0 and m["l1"] == 1.0 and m["max_abs"] == 1.0 and m["psnr"] == 0.0
    assert 0.0 < m["ssim"] < 1e-3  # (C1)(C2) / ((1 + C1)(C2)): only the luminance term survives


def test_clamping_rules():
    vals = np.float32([np.nan, np.inf, -np.inf, -3.0, 7.5, 0.25, -0.0, 1.0])
    got = MR.clamp(vals)
    assert np.array_equal(got, [0.0, 1.0, 0.0, 0.0, 1.0, 0.25, 0.0, 1.0])
    # an image of such values compares as its clamped copy, and the alpha channel is ignored
    rng = np.random.default_rng(8)
    a = rng.choice(vals, size=(13, 19, 4)).astype(np.float32)
    b = rng.random((13, 19, 3)).astype(np.float32)
    clamped = np.concatenate([MR.clamp(a[..., :3]).astype(np.float32), np.full((13, 19, 1), np.nan, np.float32)], -1)
    m1, s1 = MR.metrics(a, b)
    m2, s2 = MR.metrics(clamped, b)
    assert m1 == m2 and np.array_equal(s1, s2)
    # NaN against 0 and +inf against 1 are no difference at all
    x = np.full((5, 6, 3), np.nan, np.float32)
    x[0, 0] = np.inf
    y = np.zeros((5, 6, 3), np.float32)
    y[0, 0] = 1.0
    m, _ = MR.metrics(x, y)
    assert m["mse"] == 0.0 and m["ssim"] == 1.0


def test_swapping_is_symmetric_in_the_reference():
    rng = np.random.default_rng(4)
    a = rng.random((17, 23, 3)).astype(np.float32)
    b = rng.random((17, 23, 4)).astype(np.float32)
    mab, sab = MR.metrics(a, b)
    mba, sba = MR.metrics(b, a)
    assert mab == mba and np.array_equal(sab, sba)


def test_c_abi_checks_and_workspace():
    from spz_amd import abi
    L = abi.load_library()
    ok = L.spz_amd_image_metrics_check
    assert ok(1, 1, 3, 3) == abi.OK and ok(16384, 16384, 4, 3) == abi.OK and ok(7, 300, 3, 4) == abi.OK
    for args in ((0, 5, 3, 3), (5, 0, 3, 3), (16385, 5, 3, 3), (5, 16385, 3, 3), (-1, 5, 3, 3), (5, 5, 2, 3),
                 (5, 5, 3, 5), (5, 5, 1, 1), (5, 5, 4, 0)):
        assert ok(*args) == abi.ERR_INVALID_ARG, args
    ws = L.spz_amd_image_metrics_workspace_bytes
    assert ws(1, 1) == 32 and ws(32, 16) == 32 and ws(33, 16) == 64 and ws(32, 17) == 64
    assert ws(1920, 1080) == 60 * 68 * 32
    assert ws(0, 5) == 0 and ws(16385, 1) == 0
    # the device and host forms check their arguments before touching a device
    buf = (C.c_float * 64)()
    out = abi.ImageMetrics()
    assert L.spz_amd_image_metrics_host(buf, 3, buf, 2, 2, 2, 0, C.byref(out), None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_metrics_host(None, 3, buf, 3, 2, 2, 0, C.byref(out), None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_metrics_device(buf, 3, buf, 3, 0, 2, None, None, None, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_metrics_device(buf, 3, buf, 3, 2, 2, None, None, None, None) == abi.ERR_INVALID_ARG


def test_c_abi_compare_checks_the_views_first():
    from spz_amd import abi
    L = abi.load_library()
    h = abi.Header()
    h.num_points, h.sh_degree, h.version, h.fractional_bits = 10, 0, 3, 12
    buf = (C.c_uint8 * 4096)()
    good = abi.render_params(RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), 50, 50, 32, 24, 64, 48, coord=abi.RUB)

    def call(views, a=buf, b=buf, ha=h, hb=h):
        arr = (abi.RenderParams * max(1, len(views)))(*views)
        out = (abi.ImageMetrics * max(1, len(views)))()
        bad = C.c_int32(7)
        rc = L.spz_amd_compare_host(a, 4096, C.byref(ha), b, 4096, C.byref(hb), arr, len(views), 0, out, None, None,
                                    None, C.byref(bad))
        return rc, bad.value

    assert call([]) == (abi.ERR_INVALID_ARG, -1)
    assert call([good] * 1025) == (abi.ERR_INVALID_ARG, -1)
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.near_plane = 0.0
    assert call([good, good, worse]) == (abi.ERR_INVALID_ARG, 2)
    assert call([worse, good, good]) == (abi.ERR_INVALID_ARG, 0)
    other = abi.RenderParams.from_buffer_copy(good)
    other.coord = abi.RDF
    assert call([good, other]) == (abi.ERR_INVALID_ARG, 1)
    # the views before the inputs: no streams, a header the render refuses
    assert call([good, other], a=None, b=None) == (abi.ERR_INVALID_ARG, 1)
    assert call([good], a=None) == (abi.ERR_INVALID_ARG, -1) and call([good], b=None) == (abi.ERR_INVALID_ARG, -1)
    big = abi.Header.from_buffer_copy(h)
    big.num_points = 0x80000000
    assert call([good, good, worse], ha=big) == (abi.ERR_INVALID_ARG, 2)
    # an input: the version, the degree, the point count, the stream's length, in this order; A before B
    assert call([good], ha=big)[0] == abi.ERR_TOO_MANY_POINTS and call([good], hb=big)[0] == abi.ERR_TOO_MANY_POINTS
    big.sh_degree = 4
    assert call([good], hb=big)[0] == abi.ERR_SH_DEGREE
    big.version = 0
    assert call([good], hb=big)[0] == abi.ERR_VERSION
    long = abi.Header.from_buffer_copy(h)
    long.num_points = 1000
    assert call([good], ha=long, hb=big)[0] == abi.ERR_SHORT_STREAM


def test_compare_spz_arguments_are_checked_first(spz, tmp_path):
    missing = str(tmp_path / "missing.spz")
    with pytest.raises(ValueError, match="1..1024"):
        spz.compare_spz(missing, missing, [])
    with pytest.raises(ValueError, match="1..1024"):
        spz.compare_spz(missing, missing, [a_view()] * 1025)
    with pytest.raises(ValueError, match="view 1: bad camera"):
        spz.compare_spz(missing, missing, [a_view(), a_view(fx=-1.0)])
    with pytest.raises(ValueError, match="view 1: its coord differs"):
        spz.compare_spz(missing, missing, [a_view(coord=spz.RDF), a_view(coord=spz.RUB)], coord=spz.RDF)
    with pytest.raises(ValueError, match="views must be a sequence"):
        spz.compare_spz(missing, missing, a_view())
    with pytest.raises(ValueError, match="max_sh_degree"):
        spz.compare_spz(missing, missing, [a_view()], max_sh_degree=4)
    with pytest.raises(ValueError, match="near"):
        spz.compare_spz(missing, missing, [a_view()], near=0.0)
    with pytest.raises(ValueError, match="background"):
        spz.compare_spz(missing, missing, [a_view()], background=(0, 0))
    with pytest.raises(ValueError, match="return_maps"):
        spz.compare_spz(missing, missing, [a_view()], return_maps=1)


def test_compare_images_arguments_are_checked_first(spz):
    a = np.zeros((4, 5, 3), np.float32)
    with pytest.raises(ValueError, match="float32"):
        spz.compare_images(a.astype(np.float64), a)
    with pytest.raises(ValueError, match="3 or 4"):
        spz.compare_images(a[..., :2].copy(), a)
    with pytest.raises(ValueError, match="3 or 4"):
        spz.compare_images(a[..., 0].copy(), a)
    with pytest.raises(ValueError, match="same height and width"):
        spz.compare_images(a, np.zeros((4, 6, 3), np.float32))
    with pytest.raises(ValueError, match="1..16384"):
        spz.compare_images(np.zeros((0, 5, 3), np.float32), np.zeros((0, 5, 3), np.float32))
    with pytest.raises(ValueError, match="numpy array"):
        spz.compare_images([[[0.0, 0.0, 0.0]]], a)


def test_cli_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_compare")
    views = tmp_path / "v.txt"
    views.write_text("64 48 50 50 32 24 1 0 0 0 0 1 0 0 0 0 1 5\n")
    bad_views = tmp_path / "bad.txt"
    bad_views.write_text("64 48 50 50 32 24 1 0 0\n")
    base = ["a.spz", "b.spz"]
    v = ["--views", str(views)]
    orbit = ["--orbit", "4", "--size", "64", "48", "--fov-y", "50"]
    for args in [[], ["a.spz"], base, ["-a.spz", "b.spz"] + v, base + v + orbit,
                 base + ["--orbit", "4", "--size", "64", "48"],
                 base + ["--orbit", "0", "--size", "64", "48", "--fov-y", "50"],
                 base + ["--orbit", "1025", "--size", "64", "48", "--fov-y", "50"],
                 base + orbit + ["--center", "0", "0", "0"],
                 base + orbit + ["--radius", "-1", "--center", "0", "0", "0"],
                 base + v + ["--size", "64", "48"],
                 base + v + ["--coord", "XYZ"],
                 base + v + ["--max-sh-degree", "4"],
                 base + v + ["--near", "0"],
                 base + v + ["--background", "0", "0"],
                 base + v + ["--min-psnr", "nan"],
                 base + v + ["--min-ssim", "x"],
                 base + v + ["--ssim-maps", ""],
                 base + v + ["--min-psnr", "20", "--min-psnr", "30"],
                 base + v + ["--bogus"],
                 base + ["--views", str(bad_views)],
                 base + ["--views", str(tmp_path / "none.txt")]]:
        r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "Usage: spz_compare" in r.stderr, (args, r.stderr)
    # a file that does not load is a failure (1), not a usage error
    r = subprocess.run([tool, *base, *v], capture_output=True, text=True, timeout=60, cwd=str(tmp_path),
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and "Usage" not in r.stderr
