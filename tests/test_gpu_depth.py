"""spz_amd_render_depth_* / spz_amd.device.render_depth + render_depth_packed / spz.render_depth_spz / spz_render
--depth --ids --pick (include/spz_amd.h "render depth"; DESIGN §8 "Render") on the GPU, against the float64 restatement
of tests/depth_ref.py.

The rules of a comparison with the reference (check_maps):
  accumulated depth  within 1e-4 max(1, |D|) on at least 99.9 % of the pixels and within 5 % of the scene's depth range
                     on every pixel (the image test's two-level rule, scaled by depth);
  median             exactly the reference's Gaussian (the same index, and the bits of that record's f32 depth) on every
                     pixel whose gap (the smallest |T' - 0.5| over the pairs it used) is at least 1e-4; the pixels with a
                     smaller gap are left out, and they must be at most 0.5 % of the image.
The camera stands closer than test_gpu_render.py's (dist 1.2, not 2.2).  With that file's scene recipe (scales * 0.5 -
1.5, alphas * 0.5) that alone leaves a median on only 15.0 % and 3.8 % of the pixels of the two scenes of
test_maps_match_the_reference, so scene_cloud also makes the Gaussians twice as large and shifts the opacities up.
Measured with the float64 reference on those two scenes (the streams of the CPU oracle, which equal the device's): a
median on 52.8 % and 34.5 % of the pixels, 0.088 % and 0.076 % of the pixels left out."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import depth_ref as DR
import render_ref as RR
from conftest import ROOT
from test_filter_host import golden_streams

pytestmark = pytest.mark.gpu

W, H = 250, 190
NONE = -1


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def view_of(positions, width=W, height=H, up=(0.0, 1.0, 0.0), dist=1.2, q=5):
    """A camera on the box between the q-th and (100 - q)-th percentiles of the positions: looking at its centre from -z,
    close enough for the middle of the image to be opaque."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = np.percentile(p, q, axis=0), np.percentile(p, 100 - q, axis=0)
    c = 0.5 * (lo + hi)
    ext = float(max(hi - lo)) or 1.0
    eye = c + np.array([0.3 * ext, 0.2 * ext, -dist * ext])
    m = RR.look_at(eye, c, up)
    f = 0.9 * height
    return m, f, f, 0.5 * width + 3.25, 0.5 * height - 2.5


def params_and_cam(m, fx, fy, cx, cy, width=W, height=H, near=0.2, background=(0.1, 0.2, 0.3), max_sh_degree=3,
                   coord=0):
    from spz_amd import abi
    p = abi.render_params(m, fx, fy, cx, cy, width, height, near, background, max_sh_degree, coord)
    return p, RR.camera(m, fx, fy, cx, cy, width, height, near, background, max_sh_degree)


def to_np(cloud_t):
    return {k: v.cpu().numpy() for k, v in cloud_t.items()}


def scene_cloud(n, deg, seed, clustered=False):
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    c = (make_cloud_clustered(n, deg, seed, clusters=64, sigma=0.8) if clustered else make_cloud_numpy(n, deg, seed))
    # test_gpu_render.py's recipe is scales * 0.5 - 1.5 and alphas * 0.5: scenes so thin that even from dist 1.2 only
    # 15 % and 4 % of the pixels have a median.  Twice the size and opacities shifted up make them opaque enough.
    c["scales"] = (c["scales"] * 0.5 - 0.8).astype(np.float32)
    c["alphas"] = (c["alphas"] * 0.5 + 1.5).astype(np.float32)
    return c


def encode_scene(cuda, n, deg, seed, aa, clustered=False):
    from spz_amd import abi, device as D
    stream = D.encode(D.to_device(scene_cloud(n, deg, seed, clustered), cuda), n, deg, aa, abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0
    return stream, h


def u32(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def check_maps(depth, index, want, rec_depth, min_median=0.0):
    """The module docstring's rules.  depth (h, w, 2) and index (h, w) from the device; want: depth_ref's maps; rec_depth:
    the device's f32 record depths in input order."""
    depth, index = np.asarray(depth), np.asarray(index)
    vis = np.isfinite(rec_depth)
    span = float(rec_depth[vis].max() - rec_depth[vis].min()) if vis.any() else 0.0
    acc = depth[..., 0].astype(np.float64)
    err = np.abs(acc - want["accumulated"])
    close = float((err <= 1e-4 * np.maximum(1.0, np.abs(want["accumulated"]))).mean())
    left_out = want["gap"] < 1e-4
    has = want["index"] >= 0
    print(f"accumulated: {close:.5f} within 1e-4 max(1, |D|), worst {err.max():.3g} (depth range {span:.4g}); "
          f"median on {has.mean():.4f} of the pixels, {left_out.mean():.5f} left out")
    assert close >= 0.999, f"only {close:.5f} of the pixels within 1e-4 max(1, |D|) (worst {err.max()})"
    assert err.max() <= 0.05 * span, f"a pixel's accumulated depth is off by {err.max()} (depth range {span})"
    assert has.mean() >= min_median, f"the reference has a median on only {has.mean():.3f} of the pixels"
    assert left_out.mean() <= 0.005, f"{left_out.mean():.4f} of the pixels are within 1e-4 of the median threshold"
    ok = ~left_out
    assert np.array_equal(index[ok], want["index"][ok]), \
        f"{(index[ok] != want['index'][ok]).sum()} median indices differ from the reference"
    med = depth[..., 1]
    sel = ok & has
    assert np.array_equal(u32(med[sel]), u32(rec_depth[want["index"][sel]])), "a median depth is not its record's depth"
    assert np.all(np.isposinf(med[ok & ~has]))


# (n, degree, clustered, antialiased, coord, up): RUB with y up, RDF with y down
CASES = {"sh0_uniform_rub": (6000, 0, False, False, 4, (0.0, 1.0, 0.0)),
         "sh1_clustered_rdf_aa": (7000, 1, True, True, 6, (0.0, -1.0, 0.0))}
_scenes = {}


def scene(cuda, name):
    """The case's stream, header, decoded floats, params, reference maps and device records: made once per module."""
    if name not in _scenes:
        from spz_amd import device as D
        n, deg, clustered, aa, coord, up = CASES[name]
        stream, h = encode_scene(cuda, n, deg, 11 + deg, aa, clustered)
        floats_t = D.decode(stream, h, coord)
        floats = to_np(floats_t)
        m, fx, fy, cx, cy = view_of(floats["positions"], up=up)
        p, cam = params_and_cam(m, fx, fy, cx, cy, coord=coord)
        want = DR.render_depth(floats, deg, cam, aa)
        rec = D.preprocess_packed(stream, h, p)
        _scenes[name] = dict(stream=stream, h=h, floats_t=floats_t, n=n, deg=deg, aa=aa, p=p, want=want,
                             rec_depth=rec["depth"].cpu().numpy())
    return _scenes[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_maps_match_the_reference(cuda, name):
    from spz_amd import device as D
    s = scene(cuda, name)
    depth, index = D.render_depth_packed(s["stream"], s["h"], s["p"])
    check_maps(depth.cpu().numpy(), index.cpu().numpy(), s["want"], s["rec_depth"], min_median=0.30)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_are_consistent_and_repeat(cuda, name):
    import torch
    from spz_amd import device as D
    s = scene(cuda, name)
    depth, index, image, total, status = D.render_depth_packed(s["stream"], s["h"], s["p"], return_image=True,
                                                               return_info=True)
    assert int(status.cpu()[0]) == 0 and int(total.cpu()[0]) > 0
    d, i = depth.cpu().numpy(), index.cpu().numpy()
    assert i.dtype == np.int32 and d.shape == (H, W, 2) and i.shape == (H, W)
    has = i != NONE
    assert has.any() and (~has).any()
    assert i[has].min() >= 0 and i[has].max() < s["n"]
    assert np.array_equal(u32(d[..., 1][has]), u32(s["rec_depth"][i[has]])), "a median is not its record's depth"
    assert np.all(np.isposinf(d[..., 1][~has]))
    assert np.array_equal(u32(image), u32(D.render_packed(s["stream"], s["h"], s["p"]))), "the image differs"
    # where nothing was blended the depth sum is 0
    assert not d[..., 0][image.cpu().numpy()[..., 3] == 0].any()
    # the decoded floats, a second run and a side stream give the same bits
    side = torch.cuda.Stream(cuda)
    runs = [D.render_depth(s["floats_t"], s["n"], s["deg"], s["p"], antialiased=s["aa"], return_image=True),
            D.render_depth_packed(s["stream"], s["h"], s["p"], return_image=True),
            D.render_depth_packed(s["stream"], s["h"], s["p"], return_image=True, stream=side),
            D.render_depth_packed(s["stream"], s["h"], s["p"], return_image=True, stream=side,
                                  max_entries=int(total.cpu()[0]))]
    side.synchronize()
    for k, (d2, i2, img2) in enumerate(runs):
        assert np.array_equal(u32(d2), u32(depth)), k
        assert np.array_equal(i2.cpu().numpy(), i), k
        assert np.array_equal(u32(img2), u32(image)), k


def small_scene(cuda, n=300, seed=5):
    from spz_amd import device as D
    stream, h = encode_scene(cuda, n, 1, seed, False)
    floats = to_np(D.decode(stream, h, 4))
    floats["alphas"] = np.minimum(floats["alphas"], -0.7).astype(np.float32)  # opacity < 0.34: 3 sigma bounds a >= 1/255
    return floats


def run_floats(cuda, floats, n, deg, p, **kw):
    from spz_amd import device as D
    depth, index = D.render_depth(D.to_device(floats, cuda), n, deg, p, **kw)
    rec = D.preprocess(D.to_device(floats, cuda), n, deg, p, antialiased=kw.get("antialiased", False))
    return depth.cpu().numpy(), index.cpu().numpy(), rec["depth"].cpu().numpy()


def test_tiled_equals_bruteforce_on_device_scene(cuda):
    floats = small_scene(cuda)
    m, fx, fy, cx, cy = view_of(floats["positions"], width=67, height=45)
    p, cam = params_and_cam(m, fx, fy, cx, cy, width=67, height=45)
    depth, index, rec_depth = run_floats(cuda, floats, 300, 1, p)
    want = DR.render_depth_bruteforce(floats, 1, cam)
    assert (want["index"] >= 0).any()
    check_maps(depth, index, want, rec_depth)


@pytest.mark.parametrize("side", [16, 17])
def test_one_tile_and_one_pixel_more(cuda, side):
    floats = small_scene(cuda, seed=6)
    m, fx, fy, cx, cy = view_of(floats["positions"], width=side, height=side)
    p, cam = params_and_cam(m, fx, fy, cx, cy, width=side, height=side)
    depth, index, rec_depth = run_floats(cuda, floats, 300, 1, p)
    want = DR.render_depth(floats, 1, cam)
    assert (want["alpha"] > 0).any()
    check_maps(depth, index, want, rec_depth)


def test_empty_scene_and_behind_the_camera(cuda):
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_numpy
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    p, _ = params_and_cam(m, 100.0, 100.0, 40.0, 30.0, width=77, height=61)
    empty = {k: torch.empty(0, dtype=torch.float32, device=cuda) for k in ("positions", "scales", "rotations", "alphas",
                                                                            "colors", "sh")}
    c = make_cloud_numpy(500, 2, 3)
    c["positions"] = (c["positions"].reshape(-1, 3) * [1, 1, 0.1] - [0, 0, 8]).astype(np.float32).reshape(-1)
    for cloud, n, deg in ((empty, 0, 0), (D.to_device(c, cuda), 500, 2)):
        depth, index = D.render_depth(cloud, n, deg, p)
        d = depth.cpu().numpy()
        assert not d[..., 0].any() and np.all(np.isposinf(d[..., 1]))
        assert (index.cpu().numpy() == NONE).all()


def test_one_opaque_gaussian_filling_the_view(cuda):
    from spz_amd import device as D
    c = {"positions": np.float32([0, 0, 0]), "scales": np.float32([4, 4, 4]), "rotations": np.float32([0, 0, 0, 1]),
         "alphas": np.float32([3.0]), "colors": np.float32([0.5, -0.2, 1.0]), "sh": np.zeros(0, np.float32)}
    m = RR.look_at([0, 0, -10], [0, 0, 0], [0, 1, 0])
    p, _ = params_and_cam(m, 60.0, 60.0, 33.0, 20.0, width=66, height=40)
    depth, index, image = D.render_depth(D.to_device(c, cuda), 1, 0, p, return_image=True)
    d, i, alpha = depth.cpu().numpy(), index.cpu().numpy(), image.cpu().numpy()[..., 3]
    z = D.preprocess(D.to_device(c, cuda), 1, 0, p)["depth"].cpu().numpy()[0]
    assert abs(float(z) - 10.0) < 1e-5
    assert (alpha > 0.9).all()  # sigmoid(3) = 0.95 everywhere: one pair takes T under 0.5
    assert (i == 0).all() and np.array_equal(u32(d[..., 1]), np.full((40, 66), u32(np.float32([z]))[0]))
    exp = D.expected_depth(depth, image[..., 3]).cpu().numpy()
    assert np.abs(exp / np.float64(z) - 1.0).max() <= 1e-5


def stacked_cloud():
    rng = np.random.default_rng(17)
    n = 600
    pos = np.zeros((n, 3), np.float32)
    pos[:300, :2] = rng.uniform(-0.35, 0.35, (300, 2))
    pos[300:, :2] = rng.uniform(-0.1, 0.1, (300, 2))
    pos[:, 2] = 0.002 * np.arange(n)  # distinct depths, in input order
    opacity = np.concatenate([np.full(300, 0.05), rng.uniform(0.2, 0.3, 300)])
    return {"positions": pos.reshape(-1),
            "scales": np.repeat(np.float32([-4.5] * 300 + [-1.0] * 300), 3),
            "rotations": np.tile(np.float32([0, 0, 0, 1]), n),
            "alphas": np.log(opacity / (1.0 - opacity)).astype(np.float32),
            "colors": rng.uniform(-1, 1, n * 3).astype(np.float32), "sh": np.zeros(0, np.float32)}


def test_median_in_the_second_batch_of_a_tile(cuda):
    """600 Gaussians on one 16x16 tile, so the tile's list takes three LDS batches: the nearest 300 are a few pixels wide
    and faint, the 300 behind them cover the tile at opacity 0.2 to 0.3, so most pixels take their median past entry 256."""
    c, n = stacked_cloud(), 600
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    p, cam = params_and_cam(m, 100.0, 100.0, 8.0, 8.0, width=16, height=16)
    depth, index, rec_depth = run_floats(cuda, c, n, 0, p)
    want = DR.render_depth(c, 0, cam)
    assert np.isfinite(rec_depth).sum() > 512, "the tile must take more than two batches"
    assert (want["index"] >= 300).mean() > 0.5, "the medians must lie in the second batch"
    check_maps(depth, index, want, rec_depth)


def test_small_max_entries_sets_the_status_and_leaves_the_outputs(cuda):
    import torch
    from spz_amd import device as D
    s = scene(cuda, "sh0_uniform_rub")
    full = D.render_depth_packed(s["stream"], s["h"], s["p"], return_image=True, return_info=True)
    n_ent = int(full[3].cpu()[0])
    out = {"depth": torch.full((H, W, 2), -7.0, dtype=torch.float32, device=cuda),
           "index": torch.full((H, W), 12345, dtype=torch.int32, device=cuda),
           "image": torch.full((H, W, 4), -7.0, dtype=torch.float32, device=cuda)}
    depth, index, image, total, status = D.render_depth_packed(s["stream"], s["h"], s["p"], max_entries=n_ent - 1,
                                                               out=out, return_info=True)
    assert int(status.cpu()[0]) == 1 and int(total.cpu()[0]) == n_ent
    assert (depth.cpu().numpy() == -7.0).all() and (image.cpu().numpy() == -7.0).all()
    assert (index.cpu().numpy() == 12345).all()
    exact = D.render_depth_packed(s["stream"], s["h"], s["p"], max_entries=n_ent, out=out)
    assert exact[0] is out["depth"]
    for a, b in zip(exact, full[:3]):
        assert np.array_equal(u32(a), u32(b))
    with pytest.raises(ValueError):
        D.render_depth_packed(s["stream"], s["h"], s["p"], max_entries=-1)


def test_without_the_index_and_the_image(cuda):
    from spz_amd import device as D
    s = scene(cuda, "sh1_clustered_rdf_aa")
    depth, index = D.render_depth_packed(s["stream"], s["h"], s["p"])
    alone = D.render_depth_packed(s["stream"], s["h"], s["p"], return_index=False)
    assert alone.shape == (H, W, 2) and np.array_equal(u32(alone), u32(depth))


# the share of the pixels on which the float64 reference has a median from this view (measured: 11.6 %, 1.1 %, 100 %;
# it leaves out 0.019 %, 0 % and 0 %): the floor that keeps the exact median comparison from being empty
GOLDEN_MEDIAN_FLOOR = {"v1": 0.10, "v2": 0.01, "v3_sh3": 0.99}


@pytest.mark.parametrize("name", ["v1", "v2", "v3_sh3"])
def test_golden_streams_match_the_reference(cuda, name):
    import torch
    from spz_amd import abi, device as D
    raw = golden_streams()[name]
    rc, h = abi.peek_header(raw)
    assert rc == 0
    stream = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(cuda)
    floats = to_np(D.decode(stream, h, abi.RUB))
    # the goldens' positions span many orders of magnitude: frame the middle half
    m, fx, fy, cx, cy = view_of(floats["positions"], width=203, height=131, q=25, dist=0.8)
    p, cam = params_and_cam(m, fx, fy, cx, cy, width=203, height=131, background=(0.5, 0.5, 0.5))
    depth, index = D.render_depth_packed(stream, h, p)
    want = DR.render_depth(floats, h.sh_degree, cam, h.antialiased)
    assert (want["alpha"] > 0).any(), "the view shows nothing"
    check_maps(depth.cpu().numpy(), index.cpu().numpy(), want, D.preprocess_packed(stream, h, p)["depth"].cpu().numpy(),
               min_median=GOLDEN_MEDIAN_FLOOR[name])


def test_python_layer_and_the_cli(cuda, spz, tmp_path):
    """spz.render_depth_spz equals the device form; expected = accumulated / alpha in f32; spz_render's --depth, --ids and
    --pick carry the same bits; and without them the tool writes what it wrote before."""
    from spz_amd import abi, device as D
    stream, h = encode_scene(cuda, 2000, 3, 21, False, clustered=True)
    src = tmp_path / "in.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    eye, target = [4.0, 3.0, -16.0], [0.0, 0.0, 0.0]
    m = spz.look_at(eye, target, [0.0, 1.0, 0.0])
    kw = dict(world_to_camera=m, width=W, height=H, fx=180.0, fy=180.0, cx=W / 2, cy=H / 2, background=(0.0, 0.5, 1.0))
    got = spz.render_depth_spz(str(src), **kw)
    assert sorted(got) == ["accumulated", "alpha", "expected", "index", "median"]
    p = abi.render_params(m, 180.0, 180.0, W / 2, H / 2, W, H, 0.2, (0.0, 0.5, 1.0), 3, 0)
    depth, index, image = (t.cpu().numpy() for t in D.render_depth_packed(stream, h, p, return_image=True))
    assert np.array_equal(u32(got["accumulated"]), u32(depth[..., 0]))
    assert np.array_equal(u32(got["median"]), u32(depth[..., 1]))
    assert np.array_equal(u32(got["alpha"]), u32(image[..., 3]))
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"], index)
    assert (index != NONE).any() and (index == NONE).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = np.where(got["alpha"] > 0, got["accumulated"] / got["alpha"], np.float32(np.inf)).astype(np.float32)
    assert np.array_equal(u32(got["expected"]), u32(exp))
    assert np.array_equal(u32(spz.render_depth_spz(gz(stream.cpu().numpy().tobytes()), **kw)["expected"]), u32(exp))
    # the cloud form, on the decoded floats
    g = spz.GaussianCloud()
    g.sh_degree = 3
    for k, v in to_np(D.decode(stream, h, 0)).items():
        setattr(g, k, v)
    cl = spz.render_depth_cloud(g, **kw)
    for k in got:
        assert np.array_equal(u32(cl[k]), u32(got[k])), k
    # the CLI: same camera (look_at from --eye / --target / --up, the intrinsics given)
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_render")
    cam_args = ["--size", str(W), str(H), "--intrinsics", "180", "180", str(W / 2), str(H / 2), "--eye",
                *map(str, eye), "--target", *map(str, target), "--up", "0", "1", "0", "--background", "0", "0.5", "1"]
    vy, ux = (a[0] for a in np.nonzero(index != NONE))
    ny, nx = (a[0] for a in np.nonzero(index == NONE))
    out, ids = tmp_path / "out.pfm", tmp_path / "ids.bin"
    head = b"Pf\n%d %d\n-1.0\n" % (W, H)
    for kind in ("expected", "median"):
        dpt = tmp_path / f"{kind}.pfm"
        r = subprocess.run([tool, str(src), str(out), *cam_args, "--depth", str(dpt), "--depth-kind", kind, "--ids",
                            str(ids), "--pick", str(ux), str(vy), "--pick", str(nx), str(ny)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        body = dpt.read_bytes()
        assert body.startswith(head)
        pfm = np.frombuffer(body[len(head):], dtype="<f4").reshape(H, W)[::-1]
        assert np.array_equal(u32(pfm), u32(got[kind]))
        assert np.array_equal(np.frombuffer(ids.read_bytes(), dtype="<u4").reshape(H, W), index.view(np.uint32))
        lines = r.stdout.split("\n")
        assert lines[1] == "none" and lines[0].split()[0] == str(index[vy, ux])
        assert np.float32(lines[0].split()[1]) == depth[vy, ux, 1]
    # the colour image of a run with the new options, and of a run without them, is render_spz's
    colour = np.ascontiguousarray(spz.render_spz(str(src), **kw)[..., :3])
    assert np.array_equal(u32(colour), u32(np.ascontiguousarray(image[..., :3])))
    chead = b"PF\n%d %d\n-1.0\n" % (W, H)
    with_options = out.read_bytes()
    r = subprocess.run([tool, str(src), str(out), *cam_args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    body = out.read_bytes()
    assert body == with_options and body.startswith(chead)
    assert np.array_equal(u32(np.frombuffer(body[len(chead):], dtype="<f4").reshape(H, W, 3)[::-1]), u32(colour))


def test_unproject_depth_returns_the_gaussians_centre(cuda, spz, tmp_path):
    """One opaque Gaussian: the median depth at the pixel under its centre, back-projected, is its centre to within that
    pixel's footprint at its depth (z / fx across, z / fy down)."""
    from spz_amd import device as D
    centre = np.float32([0.4, -0.3, 1.0])
    c = {"positions": centre, "scales": np.float32([-1.5] * 3), "rotations": np.float32([0, 0, 0, 1]),
         "alphas": np.float32([6.0]), "colors": np.float32([0.5, 0.5, 0.5]), "sh": np.zeros(0, np.float32)}
    g = spz.GaussianCloud()
    for k, v in c.items():
        setattr(g, k, v)
    m = RR.look_at([1.0, 2.0, -6.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    fx, fy, cx, cy = 120.0, 110.0, 40.5, 30.25
    maps = spz.render_depth_cloud(g, world_to_camera=m, width=80, height=60, fx=fx, fy=fy, cx=cx, cy=cy)
    mean = D.preprocess(D.to_device(c, cuda), 1, 0, params_and_cam(m, fx, fy, cx, cy, 80, 60)[0])["mean"].cpu().numpy()[0]
    u, v = int(round(float(mean[0]))), int(round(float(mean[1])))
    assert maps["index"][v, u] == 0
    one = np.full((60, 80), np.inf, np.float32)
    one[v, u] = maps["median"][v, u]
    pts = spz.unproject_depth(one, m, fx, fy, cx, cy)
    assert pts.shape == (1, 3)
    z = float(one[v, u])
    in_cam = m[:, :3].astype(np.float64) @ (pts[0] - centre.astype(np.float64))
    assert abs(in_cam[0]) <= z / fx and abs(in_cam[1]) <= z / fy and abs(in_cam[2]) <= 1e-5 * z
    every = spz.unproject_depth(maps["median"], m, fx, fy, cx, cy)
    assert every.shape == (int(np.isfinite(maps["median"]).sum()), 3)
