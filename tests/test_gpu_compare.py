"""spz.compare_spz / compare_images / spz_compare / spz_amd_image_metrics_* / spz_amd.device.image_metrics (DESIGN §8
"Compare") on the GPU: the metrics against the float64 restatement of tests/metrics_ref.py within the contract's bounds
(mse, l1, max_abs 1e-12 relative, ssim 1e-7, map 1e-6), the device, host and C++ forms bit for bit, two runs and a
swap of the inputs bit for bit, a file against itself and its sorted copy, against its decimated, pruned and SH0 copies
(each view equal to compare_images of the two renders), golden v1/v2/v3 inputs, an empty file, and the CLI."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import metrics_ref as MR
import render_ref as RR
from conftest import ROOT
from test_filter_host import golden_streams
from test_gpu_prune import gz, scene, to_np

pytestmark = pytest.mark.gpu

KEYS = ("mse", "psnr", "ssim", "l1", "max_abs")


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def noisy_image(rng, h, w, c):
    """Values in [-0.3, 1.3], with NaN, +-inf and denormals sprinkled in."""
    x = rng.uniform(-0.3, 1.3, size=(h, w, c)).astype(np.float32)
    flat = x.reshape(-1)
    k = max(1, flat.size // 50)
    for v in (np.nan, np.inf, -np.inf, np.float32(1e-40), -0.0):
        flat[rng.integers(0, flat.size, k)] = v
    return x


def blurred_pair(rng, h, w, ca, cb):
    """A smooth image and a noisy copy of it, so that SSIM is far from 0 and 1."""
    base = rng.random((h, w, 3))
    for _ in range(2):
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1)) / 3.0
    a = np.concatenate([base, rng.random((h, w, 1))], -1)[..., :ca].astype(np.float32)
    b = np.concatenate([base + rng.normal(0, 0.05, base.shape), rng.random((h, w, 1))], -1)[..., :cb]
    return a, b.astype(np.float32)


def check_against_reference(got, gmap, a, b, what=""):
    want, wmap = MR.metrics(a, b)
    for k in ("mse", "l1", "max_abs"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (what, k, got[k], want[k])
    if want["mse"] == 0.0:
        assert got["psnr"] == math.inf, what
    else:
        assert abs(got["psnr"] - want["psnr"]) <= 1e-9, (what, got["psnr"], want["psnr"])
    assert abs(got["ssim"] - want["ssim"]) <= 1e-7, (what, got["ssim"], want["ssim"])
    if gmap is not None:
        err = np.abs(gmap.astype(np.float64) - wmap)
        assert err.max() <= 1e-6, (what, float(err.max()))


def host_form(a, b, with_map=True):
    """spz_amd_image_metrics_host through ctypes."""
    from spz_amd import abi
    L = abi.load_library()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    h, w = a.shape[:2]
    out = abi.ImageMetrics()
    m = np.empty((h, w), np.float32) if with_map else None
    rc = L.spz_amd_image_metrics_host(a.ctypes.data, a.shape[2], b.ctypes.data, b.shape[2], w, h, 0, C.byref(out),
                                      m.ctypes.data if with_map else None)
    assert rc == abi.OK
    return np.float64([getattr(out, k) for k in KEYS]), m


def as_vec(d):
    return np.float64([d[k] for k in KEYS])


@pytest.mark.parametrize("h,w", [(1, 1), (7, 300), (250, 190), (1080, 1920)])
def test_image_metrics_match_the_reference(cuda, spz, h, w):
    import torch
    from spz_amd import device as D
    rng = np.random.default_rng(h * 7 + w)
    for ca, cb in ((3, 3), (3, 4), (4, 3), (4, 4)):
        for a, b in (blurred_pair(rng, h, w, ca, cb), (noisy_image(rng, h, w, ca), noisy_image(rng, h, w, cb))):
            what = f"{h}x{w} {ca}/{cb}"
            got = spz.compare_images(a, b, return_map=True)
            check_against_reference(got, got["ssim_map"], a, b, what)
            # the C++ form (compare_images), the host C form and the device tensor form give the same bits
            hv, hmap = host_form(a, b)
            assert np.array_equal(hv.view(np.uint64), as_vec(got).view(np.uint64)), what
            assert np.array_equal(hmap.view(np.uint32), got["ssim_map"].view(np.uint32)), what
            at, bt = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
            dmap = torch.empty((h, w), dtype=torch.float32, device=cuda)
            dv = D.image_metrics(at, bt, ssim_map=dmap)
            assert dv.dtype == torch.float64 and dv.device == at.device
            assert np.array_equal(dv.cpu().numpy().view(np.uint64), as_vec(got).view(np.uint64)), what
            assert np.array_equal(dmap.cpu().numpy().view(np.uint32), got["ssim_map"].view(np.uint32)), what


def test_runs_repeat_and_swapping_is_bit_identical(cuda, spz):
    import torch
    from spz_amd import device as D
    rng = np.random.default_rng(11)
    for h, w in ((37, 61), (513, 700)):
        a, b = blurred_pair(rng, h, w, 4, 3)
        b[3, 5, 0] = np.nan
        first = spz.compare_images(a, b, return_map=True)
        again = spz.compare_images(a, b, return_map=True)
        swapped = spz.compare_images(b, a, return_map=True)
        for other in (again, swapped):
            assert np.array_equal(as_vec(other).view(np.uint64), as_vec(first).view(np.uint64))
            assert np.array_equal(other["ssim_map"].view(np.uint32), first["ssim_map"].view(np.uint32))
        # on a side stream too
        at, bt = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
        side = torch.cuda.Stream(cuda)
        dv = D.image_metrics(bt, at, stream=side)
        side.synchronize()
        assert np.array_equal(dv.cpu().numpy().view(np.uint64), as_vec(first).view(np.uint64))


def test_analytic_cases_on_the_device(cuda, spz):
    z = np.zeros((20, 33, 3), np.float32)
    o = np.ones((20, 33, 4), np.float32)
    m = spz.compare_images(z, o)
    assert m["mse"] == 1.0 and m["l1"] == 1.0 and m["max_abs"] == 1.0 and m["psnr"] == 0.0
    e = spz.compare_images(o, o[..., :3].copy(), return_map=True)
    assert e["ssim"] == 1.0 and e["mse"] == 0.0 and e["psnr"] == math.inf and np.all(e["ssim_map"] == 1.0)
    # NaN against 0, +inf against 1, -inf against 0: no difference at all
    x = np.full((9, 40, 3), np.nan, np.float32)
    x[:, :10] = np.inf
    x[:, 10:20] = -np.inf
    y = np.zeros((9, 40, 3), np.float32)
    y[:, :10] = 1.0
    n = spz.compare_images(x, y)
    assert n["mse"] == 0.0 and n["ssim"] == 1.0 and n["max_abs"] == 0.0


def orbit(spz, src, k, w, h, coord):
    return spz.orbit_views(k, width=w, height=h, fov_y=50.0, scene=str(src), coord=coord, distance=2.0)


def render_pair(spz, fa, fb, v, coord, bg, deg=3):
    kw = dict(v, coord=coord, background=bg, max_sh_degree=deg)
    return spz.render_spz(str(fa), **kw), spz.render_spz(str(fb), **kw)


def check_views(spz, fa, fb, views, coord, bg=(0.0, 0.0, 0.0), deg=3, reference=True):
    got = spz.compare_spz(str(fa), str(fb), views, coord=coord, background=bg, max_sh_degree=deg, return_maps=True)
    assert len(got) == len(views)
    for j, v in enumerate(views):
        ia, ib = render_pair(spz, fa, fb, v, coord, bg, deg)
        want = spz.compare_images(ia, ib, return_map=True)
        assert np.array_equal(as_vec(got[j]).view(np.uint64), as_vec(want).view(np.uint64)), j
        assert np.array_equal(got[j]["ssim_map"].view(np.uint32), want["ssim_map"].view(np.uint32)), j
        if reference:
            check_against_reference(got[j], got[j]["ssim_map"], ia, ib, f"view {j}")
    return got


def test_a_file_against_itself_and_its_sorted_copy(cuda, spz, tmp_path):
    from spz_amd import device as D
    _, (stream, hdr) = scene(cuda, 2000, 3, 21, False)
    src, srt = tmp_path / "in.spz", tmp_path / "sorted.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    spz.sort_spz(str(src), str(srt))
    floats = to_np(D.decode(stream, hdr, 4))
    views = []
    for v in spz.orbit_views(16, width=71, height=53, fov_y=25.0, scene=str(src), coord=spz.RUB, distance=6.0):
        # only views with distinct depths, where the sorted file blends in the same order
        rec = RR.preprocess(floats, 3, RR.camera(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                                                  v["height"]))
        d = rec["depth"][rec["visible"]]
        if np.unique(d).size == d.size:
            views.append(v)
    assert len(views) >= 3
    for other in (src, srt):
        for m in spz.compare_spz(str(src), str(other), views, coord=spz.RUB, background=(0.2, 0.3, 0.4)):
            assert m["ssim"] == 1.0 and m["mse"] == 0.0 and m["psnr"] == math.inf and m["max_abs"] == 0.0


@pytest.mark.parametrize("edit", ["decimate", "prune", "filter_sh0"])
def test_lossy_copies_equal_compare_images_of_the_renders(cuda, spz, tmp_path, edit):
    _, (stream, hdr) = scene(cuda, 4000, 3, 19, False)
    src, out = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    views = orbit(spz, src, 4, 83, 61, spz.RDF)
    if edit == "decimate":
        spz.decimate_spz(str(src), str(out), target_points=1000)
    elif edit == "prune":
        spz.prune_spz(str(src), str(out), views, keep_fraction=0.4, coord=spz.RDF)
    else:
        spz.filter_spz(str(src), str(out), sh_degree=0)
    got = check_views(spz, src, out, views, spz.RDF, bg=(0.1, 0.1, 0.1))
    assert all(0.0 < m["mse"] and m["ssim"] < 1.0 for m in got), got
    # the bytes form gives the same bits as the paths form
    again = spz.compare_spz(src.read_bytes(), out.read_bytes(), views, coord=spz.RDF, background=(0.1, 0.1, 0.1))
    for x, y in zip(got, again):
        assert np.array_equal(as_vec(x).view(np.uint64), as_vec(y).view(np.uint64))


def test_golden_and_mixed_versions(cuda, spz, tmp_path):
    import torch
    from spz_amd import abi, device as D
    files = {}
    for name in ("v1", "v2", "v3_sh3", "v3_sh0"):
        f = tmp_path / f"{name}.spz"
        f.write_bytes(gz(golden_streams()[name]))
        files[name] = f
    raw = golden_streams()["v3_sh3"]
    rc, h = abi.peek_header(raw)
    st = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(cuda)
    pos = D.decode(st, h, abi.RUB)["positions"].cpu().numpy().reshape(-1, 3)
    pos = pos[np.isfinite(pos).all(axis=1)]
    lo, hi = np.percentile(pos, 25, axis=0), np.percentile(pos, 75, axis=0)
    views = spz.orbit_views(3, width=71, height=37, fov_y=60.0, center=(0.5 * (lo + hi)).tolist(),
                            radius=float(np.linalg.norm(hi - lo)) * 0.5 + 1e-3)
    for fa, fb in (("v1", "v1"), ("v2", "v3_sh3"), ("v1", "v3_sh3"), ("v3_sh3", "v3_sh0"), ("v3_sh0", "v2")):
        check_views(spz, files[fa], files[fb], views, spz.RUB, bg=(0.5, 0.25, 0.0), deg=2)


def test_an_empty_file_compares_as_its_render(cuda, spz, tmp_path):
    _, (stream, hdr) = scene(cuda, 1500, 1, 3, False)
    src, empty = tmp_path / "in.spz", tmp_path / "empty.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    spz.filter_spz(str(src), str(empty), mask=np.zeros(1500, bool))
    views = orbit(spz, src, 2, 50, 40, spz.RUB)
    bg = (0.25, 0.5, 0.75)
    img = spz.render_spz(str(empty), **dict(views[0], coord=spz.RUB, background=bg))
    assert np.array_equal(img[..., :3], np.broadcast_to(np.float32(bg), (40, 50, 3))) and not img[..., 3].any()
    check_views(spz, empty, src, views, spz.RUB, bg=bg)
    for m in spz.compare_spz(str(empty), str(empty), views, coord=spz.RUB, background=bg):
        assert m["ssim"] == 1.0 and m["psnr"] == math.inf


def test_bad_view_is_named_and_mixed_coords_are_refused(cuda, spz):
    import torch
    from spz_amd import abi
    L = abi.load_library()
    raw = golden_streams()["v3_sh1"]
    rc, h = abi.peek_header(raw)
    st = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(cuda)
    good = abi.render_params(np.eye(3, 4, dtype=np.float32), 50, 50, 32, 24, 64, 48, coord=abi.RUB)
    other = abi.RenderParams.from_buffer_copy(good)
    other.coord = abi.LUF
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.width = 0
    for views, bad_at in (([good, good, other], 2), ([good, worse], 1)):
        arr = (abi.RenderParams * len(views))(*views)
        out = (abi.ImageMetrics * len(views))()
        bad = C.c_int32(-5)
        torch.cuda.synchronize()
        rc = L.spz_amd_compare_host(st.data_ptr(), st.numel(), C.byref(h), st.data_ptr(), st.numel(), C.byref(h), arr,
                                    len(views), 0, out, None, None, None, C.byref(bad))
        assert rc == abi.ERR_INVALID_ARG and bad.value == bad_at
    # the same file through the ABI with entries out: A and B totals per view, equal for one file
    arr = (abi.RenderParams * 2)(good, good)
    out = (abi.ImageMetrics * 2)()
    ent = (C.c_uint64 * 4)()
    ms = (C.c_float * 2)()
    rc = L.spz_amd_compare_host(st.data_ptr(), st.numel(), C.byref(h), st.data_ptr(), st.numel(), C.byref(h), arr, 2, 0,
                                out, None, ent, ms, None)
    assert rc == abi.OK and ent[0] == ent[1] == ent[2] == ent[3]
    assert out[0].ssim == 1.0 and out[1].mse == 0.0


def read_pfm_grey(path):
    data = open(path, "rb").read()
    head, rest = data.split(b"\n", 1)
    assert head == b"Pf"
    dims, rest = rest.split(b"\n", 1)
    w, h = (int(x) for x in dims.split())
    scale, rest = rest.split(b"\n", 1)
    assert float(scale) < 0
    return np.frombuffer(rest, "<f4").reshape(h, w)[::-1]


def test_cli_matches_compare_spz(cuda, spz, tmp_path):
    _, (stream, hdr) = scene(cuda, 2500, 2, 44, False)
    src, out = tmp_path / "in.spz", tmp_path / "dec.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    spz.decimate_spz(str(src), str(out), target_points=600)
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_compare")
    views = spz.orbit_views(3, width=45, height=33, fov_y=55.0, scene=str(src), coord=spz.RDF, distance=2.0)
    want = spz.compare_spz(str(src), str(out), views, coord=spz.RDF, background=(0.1, 0.2, 0.3), max_sh_degree=1,
                           return_maps=True)
    prefix = str(tmp_path / "map")
    args = [tool, str(src), str(out), "--orbit", "3", "--size", "45", "33", "--fov-y", "55", "--distance", "2",
            "--coord", "RDF", "--background", "0.1", "0.2", "0.3", "--max-sh-degree", "1"]
    r = subprocess.run(args + ["--ssim-maps", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4
    for j, line in enumerate(lines[:3]):
        tok = line.split()
        assert tok[:2] == ["view", str(j)]
        got = dict(zip(tok[2::2], (float(x) for x in tok[3::2])))
        for k in KEYS:
            assert got[k] == want[j][k], (j, k)
        assert np.array_equal(read_pfm_grey(f"{prefix}_{j}.pfm").view(np.uint32), want[j]["ssim_map"].view(np.uint32))
    tok = lines[3].split()
    psnr = [m["psnr"] for m in want]
    ssim = [m["ssim"] for m in want]
    mean_p, mean_s = 0.0, 0.0
    for p, s in zip(psnr, ssim):
        mean_p += p
        mean_s += s
    assert tok[0] == "mean" and float(tok[2]) == mean_p / 3 and float(tok[4]) == mean_s / 3
    assert float(tok[7]) == min(psnr) and int(tok[9]) == int(np.argmin(psnr))
    assert float(tok[12]) == min(ssim) and int(tok[14]) == int(np.argmin(ssim))
    # thresholds: missed -> 2, met -> 0
    worst = min(psnr)
    r = subprocess.run(args + ["--min-psnr", repr(worst + 0.5)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr
    r = subprocess.run(args + ["--min-psnr", repr(worst - 0.5), "--min-ssim", repr(min(ssim) - 1e-3)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(args + ["--min-ssim", "1.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr
    # --views: the same values
    vf = tmp_path / "views.txt"
    rows = []
    for v in views:
        vals = [v["width"], v["height"], v["fx"], v["fy"], v["cx"], v["cy"]] + list(v["world_to_camera"].reshape(-1))
        rows.append(" ".join(repr(float(x)) if not isinstance(x, int) else str(x) for x in vals))
    vf.write_text("\n".join(rows) + "\n")
    r = subprocess.run([tool, str(src), str(out), "--views", str(vf), "--coord", "RDF", "--background", "0.1", "0.2",
                        "0.3", "--max-sh-degree", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "\n".join(lines) + "\n"
