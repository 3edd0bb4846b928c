"""spz.render_spz / spz_render / spz_amd_render_* / spz_amd.device.render + render_packed (DESIGN §8 "Render") on the
GPU, against the float64 restatement of tests/render_ref.py: the records within 1e-5 relative (or 1e-6 absolute), the
images within 1e-4 on at least 99.9 % of the channels and within 0.05 everywhere; a stream and its decoded floats, two
runs, a file and its sorted copy, and the CLI's PFM bit for bit."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import render_ref as RR
from conftest import ROOT
from test_filter_host import golden_streams

pytestmark = pytest.mark.gpu

W, H = 250, 190


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def view_of(positions, width=W, height=H, up=(0.0, 1.0, 0.0), dist=2.2, q=5):
    """A camera on the box between the q-th and (100 - q)-th percentiles of the positions: looking at its centre from -z,
    far enough to see it."""
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


def check_records(got, want):
    vis = want["visible"]
    g_vis = np.isfinite(got["depth"].cpu().numpy())
    r3 = want["r3"]
    near_int = np.abs(r3 - np.round(r3)) < 1e-4
    ok = ~near_int
    assert np.array_equal(g_vis[ok], vis[ok]), "visibility differs"
    sel = vis & ok & g_vis
    assert sel.sum() > 0
    for k in ("mean", "conic", "opacity", "rgb", "depth"):
        a = got[k].cpu().numpy()[sel].astype(np.float64)
        b = want[k][sel].astype(np.float64)
        bad = np.abs(a - b) > np.maximum(1e-5 * np.abs(b), 1e-6)
        assert not bad.any(), f"{k}: {bad.sum()} values off, worst {np.max(np.abs(a - b))}"
    assert np.array_equal(got["rect"].cpu().numpy()[sel], want["rect"][sel]), "tile rectangles differ"


def check_image(got, want):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    frac = float((err <= 1e-4).mean())
    assert frac >= 0.999, f"only {frac:.5f} of the channels within 1e-4 (worst {err.max()})"
    assert err.max() <= 0.05, f"a channel is off by {err.max()}"


def encode_scene(cuda, n, deg, seed, aa, coord, clustered=False):
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    c = (make_cloud_clustered(n, deg, seed, clusters=64, sigma=0.8) if clustered else make_cloud_numpy(n, deg, seed))
    c["scales"] = (c["scales"] * 0.5 - 1.5).astype(np.float32)       # 2D sizes of a few to a few tens of pixels
    c["alphas"] = (c["alphas"] * 0.5).astype(np.float32)
    stream = D.encode(D.to_device(c, cuda), n, deg, aa, abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0
    return stream, h


CASES = [(0, False, 4, 3), (1, True, 4, 3), (2, False, 6, 3), (3, True, 6, 3), (3, False, 4, 1), (2, True, 6, 0)]


@pytest.mark.parametrize("deg,aa,coord,max_sh", CASES)
def test_packed_v3_matches_the_reference(cuda, deg, aa, coord, max_sh):
    from spz_amd import device as D
    n = 6000 + 1000 * deg
    stream, h = encode_scene(cuda, n, deg, 11 + deg, aa, coord, clustered=deg % 2 == 1)
    floats = to_np(D.decode(stream, h, coord))
    up = (0.0, 1.0, 0.0) if coord in (4, 7, 8, 3) else (0.0, -1.0, 0.0)
    m, fx, fy, cx, cy = view_of(floats["positions"], up=up)
    p, cam = params_and_cam(m, fx, fy, cx, cy, max_sh_degree=max_sh, coord=coord)
    rec = D.preprocess_packed(stream, h, p)
    want_rec = RR.preprocess(floats, deg, cam, aa)
    check_records(rec, want_rec)
    assert int(rec["total"].cpu()[0]) == RR.entry_count(want_rec)
    img = D.render_packed(stream, h, p)
    check_image(img.cpu().numpy(), RR.render(floats, deg, cam, aa, rec=want_rec))
    # the decoded floats render to the same bits
    img_f = D.render(D.decode(stream, h, coord), n, deg, p, antialiased=aa)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), img_f.cpu().numpy().view(np.uint32))
    # and a second run repeats them
    img2 = D.render_packed(stream, h, p)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), img2.cpu().numpy().view(np.uint32))


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
    m, fx, fy, cx, cy = view_of(floats["positions"], width=203, height=131, q=25)
    p, cam = params_and_cam(m, fx, fy, cx, cy, width=203, height=131, background=(0.5, 0.5, 0.5))
    img = D.render_packed(stream, h, p).cpu().numpy()
    want = RR.render(floats, h.sh_degree, cam, h.antialiased)
    check_image(img, want)
    assert (img[..., 3] > 0).any(), "the view shows nothing"


def test_tiled_equals_bruteforce_on_device_scene(cuda):
    from spz_amd import device as D
    stream, h = encode_scene(cuda, 300, 1, 5, False, 4)
    floats = to_np(D.decode(stream, h, 4))
    floats["alphas"] = np.minimum(floats["alphas"], -0.7).astype(np.float32)  # opacity < 0.34: 3 sigma bounds a >= 1/255
    m, fx, fy, cx, cy = view_of(floats["positions"], width=70, height=45)
    p, cam = params_and_cam(m, fx, fy, cx, cy, width=70, height=45)
    img = D.render(D.to_device(floats, cuda), 300, 1, p).cpu().numpy()
    check_image(img, RR.render_bruteforce(floats, 1, cam))


def test_file_equals_its_sorted_copy_and_the_cli(cuda, spz, tmp_path):
    from spz_amd import device as D
    stream, h = encode_scene(cuda, 2000, 3, 21, False, 4, clustered=True)
    raw = stream.cpu().numpy().tobytes()
    src, srt = tmp_path / "in.spz", tmp_path / "sorted.spz"
    src.write_bytes(gz(raw))
    spz.sort_spz(str(src), str(srt))
    floats = to_np(D.decode(stream, h, 4))
    eye, target = [4.0, 3.0, -30.0], [0.0, 0.0, 0.0]
    m = spz.look_at(eye, target, [0.0, 1.0, 0.0])
    kw = dict(world_to_camera=m, width=W, height=H, fx=180.0, fy=180.0, cx=W / 2, cy=H / 2, background=(0.0, 0.5, 1.0))
    a = spz.render_spz(str(src), **kw)
    rec = RR.preprocess(floats, 3, RR.camera(m, 180.0, 180.0, W / 2, H / 2, W, H))
    d = rec["depth"][rec["visible"]]
    assert np.unique(d).size == d.size, "the scene must have distinct depths"
    b = spz.render_spz(str(srt), **kw)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the sorted file renders differently"
    c = spz.render_spz(gz(raw), **kw)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    # the CLI's PFM: same camera (look_at from --eye / --target / --up, the intrinsics given)
    out = tmp_path / "out.pfm"
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_render")
    r = subprocess.run([tool, str(src), str(out), "--size", str(W), str(H), "--intrinsics", "180", "180", str(W / 2),
                        str(H / 2), "--eye", *map(str, eye), "--target", *map(str, target), "--up", "0", "1", "0",
                        "--background", "0", "0.5", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    body = out.read_bytes()
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert body.startswith(head)
    pfm = np.frombuffer(body[len(head):], dtype="<f4").reshape(H, W, 3)[::-1]
    assert np.array_equal(pfm.view(np.uint32), np.ascontiguousarray(a[..., :3]).view(np.uint32))
    ppm = tmp_path / "out.ppm"
    r = subprocess.run([tool, str(src), str(ppm), "--size", str(W), str(H), "--fov-y", "50", "--eye", *map(str, eye),
                        "--target", *map(str, target)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert ppm.read_bytes().startswith(b"P6\n%d %d\n255\n" % (W, H))


def test_empty_scene_and_behind_the_camera(cuda):
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_numpy
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    p, cam = params_and_cam(m, 100.0, 100.0, 40.0, 30.0, width=77, height=61, background=(0.25, 0.5, 0.75))
    empty = {k: torch.empty(0, dtype=torch.float32, device=cuda) for k in ("positions", "scales", "rotations", "alphas",
                                                                            "colors", "sh")}
    img = D.render(empty, 0, 0, p).cpu().numpy()
    assert np.array_equal(img[..., :3], np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (61, 77, 3)))
    assert not img[..., 3].any()
    c = make_cloud_numpy(500, 2, 3)
    c["positions"] = (c["positions"].reshape(-1, 3) * [1, 1, 0.1] - [0, 0, 8]).astype(np.float32).reshape(-1)
    img = D.render(D.to_device(c, cuda), 500, 2, p).cpu().numpy()
    assert np.array_equal(img[..., :3], np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (61, 77, 3)))
    assert not img[..., 3].any()


def test_one_gaussian_filling_the_view(cuda):
    from spz_amd import device as D
    c = {"positions": np.float32([0, 0, 0]), "scales": np.float32([4, 4, 4]), "rotations": np.float32([0, 0, 0, 1]),
         "alphas": np.float32([3.0]), "colors": np.float32([0.5, -0.2, 1.0]), "sh": np.zeros(0, np.float32)}
    m = RR.look_at([0, 0, -10], [0, 0, 0], [0, 1, 0])
    p, cam = params_and_cam(m, 60.0, 60.0, 33.0, 20.0, width=66, height=40)
    img = D.render(D.to_device(c, cuda), 1, 0, p).cpu().numpy()
    want = RR.render(c, 0, cam)
    check_image(img, want)
    assert (img[..., 3] > 0.9).all()


def test_small_max_entries_sets_the_status_and_leaves_the_image(cuda, spz, tmp_path):
    import torch
    from spz_amd import device as D
    stream, h = encode_scene(cuda, 3000, 0, 8, False, 4)
    floats = to_np(D.decode(stream, h, 4))
    m, fx, fy, cx, cy = view_of(floats["positions"])
    p, _ = params_and_cam(m, fx, fy, cx, cy)
    full, total, status = D.render_packed(stream, h, p, return_info=True)
    n_ent = int(total.cpu()[0])
    assert n_ent > 100 and int(status.cpu()[0]) == 0
    out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=cuda)
    img, total2, status2 = D.render_packed(stream, h, p, max_entries=n_ent - 1, out=out, return_info=True)
    assert int(status2.cpu()[0]) == 1 and int(total2.cpu()[0]) == n_ent
    assert (img.cpu().numpy() == -7.0).all()
    exact = D.render_packed(stream, h, p, max_entries=n_ent)
    assert np.array_equal(exact.cpu().numpy().view(np.uint32), full.cpu().numpy().view(np.uint32))
    # the host form sizes its own workspace
    src = tmp_path / "s.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    a = spz.render_spz(str(src), world_to_camera=m, width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy,
                       background=(0.1, 0.2, 0.3))
    assert np.array_equal(a.view(np.uint32), full.cpu().numpy().view(np.uint32))


def test_bad_arguments_are_refused_before_any_launch(cuda, spz, tmp_path):
    from spz_amd import abi, device as D
    stream, h = encode_scene(cuda, 100, 0, 2, False, 4)
    m = RR.look_at([0, 0, -30], [0, 0, 0], [0, 1, 0])
    bad = m.copy()
    bad[0, 0] *= 1.01
    for kw in (dict(world_to_camera=bad), dict(fx=-1.0), dict(width=0), dict(height=16385), dict(near=0.0),
               dict(max_sh_degree=4)):
        args = dict(world_to_camera=m, fx=100.0, fy=100.0, cx=50.0, cy=50.0, width=100, height=100)
        args.update(kw)
        with pytest.raises(ValueError):
            abi.render_params(args["world_to_camera"], args["fx"], args["fy"], args["cx"], args["cy"], args["width"],
                              args["height"], args.get("near", 0.2), (0, 0, 0), args.get("max_sh_degree", 3))
        src = tmp_path / "b.spz"
        src.write_bytes(gz(stream.cpu().numpy().tobytes()))
        with pytest.raises(ValueError):
            spz.render_spz(str(src), **{"near": 0.2, "max_sh_degree": 3, **args})
    p = abi.render_params(m, 100.0, 100.0, 50.0, 50.0, 100, 100)
    with pytest.raises(ValueError):
        D.render_packed(stream, h, p, max_entries=-1)


def test_side_stream_renders_the_same_bits(cuda):
    """Every surface with stream= on a side stream: the image, the status, the total and the records equal the
    current stream's, both with the total read back (max_entries None) and with a given max_entries."""
    import torch
    from spz_amd import device as D
    stream, h = encode_scene(cuda, 12000, 3, 31, True, 4, clustered=True)
    floats_t = D.decode(stream, h, 4)
    m, fx, fy, cx, cy = view_of(floats_t["positions"].cpu().numpy())
    p, _ = params_and_cam(m, fx, fy, cx, cy)
    want, total, _ = D.render_packed(stream, h, p, return_info=True)
    want = want.cpu().numpy()
    n_ent = int(total.cpu()[0])
    want_rec = {k: v.cpu().numpy() for k, v in D.preprocess_packed(stream, h, p).items()}
    side = torch.cuda.Stream(cuda)
    for _ in range(3):
        got = [D.render_packed(stream, h, p, stream=side, return_info=True),
               D.render_packed(stream, h, p, max_entries=n_ent, stream=side, return_info=True),
               D.render(floats_t, 12000, 3, p, antialiased=True, stream=side, return_info=True)]
        rec = D.preprocess_packed(stream, h, p, stream=side)
        side.synchronize()
        for img, tot, status in got:
            assert int(tot.cpu()[0]) == n_ent and int(status.cpu()[0]) == 0
            assert np.array_equal(img.cpu().numpy().view(np.uint32), want.view(np.uint32))
        for k, v in rec.items():
            assert np.array_equal(v.cpu().numpy(), want_rec[k]), k


def test_render_cloud_from_host_memory(cuda, spz):
    """spz.render_cloud (spz::renderCloud -> spz_amd_render_cloud_host) equals the device form on the same floats."""
    from spz_amd import device as D
    stream, h = encode_scene(cuda, 7000, 2, 41, False, 4)
    floats = to_np(D.decode(stream, h, 4))
    m, fx, fy, cx, cy = view_of(floats["positions"])
    p, _ = params_and_cam(m, fx, fy, cx, cy, max_sh_degree=1)
    want = D.render(D.to_device(floats, cuda), 7000, 2, p).cpu().numpy()
    g = spz.GaussianCloud()
    g.sh_degree = 2
    for k, v in floats.items():
        setattr(g, k, v)
    for aa in (False, True):
        g.antialiased = aa
        got = spz.render_cloud(g, world_to_camera=m, width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy,
                               background=(0.1, 0.2, 0.3), max_sh_degree=1)
        ref = want if not aa else D.render(D.to_device(floats, cuda), 7000, 2, p, antialiased=True).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    empty = spz.GaussianCloud()
    img = spz.render_cloud(empty, world_to_camera=m, width=31, height=17, fx=fx, fy=fy, cx=cx, cy=cy,
                           background=(0.1, 0.2, 0.3))
    assert np.array_equal(img[..., :3], np.broadcast_to(np.float32([0.1, 0.2, 0.3]), (17, 31, 3)))
    assert not img[..., 3].any()
