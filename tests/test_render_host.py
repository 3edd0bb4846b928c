"""The render contract without a GPU (DESIGN §8 "Render"): tests/render_ref.py on analytic scenes and against a
brute-force per-pixel blend, spz.look_at, the C ABI's parameter check and workspace size, and spz_render's usage
errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_ref as RR
from conftest import ROOT


def one(pos, log_scale, alpha, colour, rot=(0.0, 0.0, 0.0, 1.0)):
    return {"positions": np.float32(pos), "scales": np.float32([log_scale] * 3), "rotations": np.float32(rot),
            "alphas": np.float32([alpha]), "colors": np.float32(colour), "sh": np.zeros(0, np.float32)}


def cat(*clouds):
    return {k: np.concatenate([c[k] for c in clouds]) for k in clouds[0]}


def cam_at_origin(w=64, h=48, bg=(0.2, 0.4, 0.6)):
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    # cx, cy such that the optical axis falls on pixel (32, 24): m = fx x / z + cx - 0.5
    return RR.camera(m, 50.0, 50.0, 32.5, 24.5, w, h, background=bg)


def colour_of(rgb):
    return ((np.float32(rgb) - 0.5) / RR.C0).astype(np.float32)


def test_single_isotropic_gaussian_centre_pixel():
    cam = cam_at_origin()
    alpha = np.log(0.6 / 0.4)  # opacity 0.6
    c = one([0, 0, 5], -1.0, alpha, colour_of([0.9, 0.1, 0.3]))
    rec = RR.preprocess(c, 0, cam)
    assert rec["visible"][0]
    assert np.allclose(rec["mean"][0], [32.0, 24.0])
    assert np.allclose(rec["rgb"][0], [0.9, 0.1, 0.3], atol=1e-6)
    img = RR.render(c, 0, cam)
    o = float(rec["opacity"][0])
    want = o * np.float64(rec["rgb"][0]) + (1 - o) * cam["background"]
    assert np.allclose(img[24, 32, :3], want, atol=1e-12)
    assert np.isclose(img[24, 32, 3], o)
    # symmetric about the centre, fading outwards
    assert np.allclose(img[24, 30], img[24, 34]) and img[24, 40, 3] < img[24, 34, 3] < img[24, 32, 3]


def test_front_gaussian_occludes_the_back_one():
    cam = cam_at_origin()
    front = one([0, 0, 4], -0.5, 8.0, colour_of([1.0, 0.0, 0.0]))
    back = one([0, 0, 8], 0.0, 8.0, colour_of([0.0, 0.0, 1.0]))
    for order in ((front, back), (back, front)):
        img = RR.render(cat(*order), 0, cam)
        px = img[24, 32]
        assert px[0] > 0.98 and px[2] < 0.02, px  # alpha is capped at 0.99: a trace of what lies behind


def test_empty_scene_and_everything_behind_the_camera():
    cam = cam_at_origin(w=37, h=21)
    empty = {k: np.zeros(0, np.float32) for k in ("positions", "scales", "rotations", "alphas", "colors", "sh")}
    for c in (empty, cat(one([0, 0, -3], 0.0, 5.0, [1, 1, 1]), one([0, 0, 0.1], 0.0, 5.0, [1, 1, 1]))):
        img = RR.render(c, 0, cam)
        assert np.array_equal(img[..., :3], np.broadcast_to(cam["background"], (21, 37, 3)))
        assert not img[..., 3].any()
        assert RR.entry_count(RR.preprocess(c, 0, cam)) == 0


def test_tiled_equals_bruteforce():
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(400, 2, 9)
    c["scales"] = (c["scales"] * 0.5 - 1.5).astype(np.float32)
    c["alphas"] = np.minimum(c["alphas"], -0.7).astype(np.float32)  # opacity < 0.34: beyond 3 sigma a < 1/255
    m = RR.look_at([2.0, 3.0, -35.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])
    for aa in (False, True):
        cam = RR.camera(m, 70.0, 66.0, 41.0, 27.0, 83, 50, background=(0.3, 0.3, 0.3), max_sh_degree=2)
        t, b = RR.render(c, 2, cam, aa), RR.render_bruteforce(c, 2, cam, aa)
        assert t[..., 3].max() > 0.05 and (t[..., 3] > 0).mean() > 0.05
        assert np.allclose(t, b, rtol=0, atol=1e-12)


def deep_scene():
    """The first gradient scene of test_gpu_render_grad (300 Gaussians and 4 clamp hits at 40 x 36, degree 3 used to
    degree 2): lists of up to about 290 entries, a few hundred pixels that stop, alphas that clamp."""
    import render_grad_ref as GR
    from test_gpu_render import view_of
    c = GR.scene(1, 3, clamp_hits=4)
    m, fx, fy, cx, cy = view_of(c["positions"], width=40, height=36)
    return c, RR.camera(m, fx, fy, cx, cy, 40, 36, 0.2, (0.1, 0.2, 0.3), 2)


@pytest.mark.parametrize("aa", [False, True])
def test_vectorised_blend_equals_the_loop_bit_for_bit(aa):
    """render_ref.walk makes _blend's products and sums in _blend's order: render() through _blend_vec and
    render_tiles() give the bits of render() through _blend, and walk's decisions are render_grad_ref._walk's."""
    import render_grad_ref as GR
    c, cam = deep_scene()
    rec = RR.preprocess(c, 3, cam, aa)
    want = RR.render(c, 3, cam, aa, rec=rec)
    tw, th = RR.tiles(cam)
    lists = RR.tile_lists(rec, cam)
    assert max(len(s) for s in lists.values()) >= 100 and sum(len(s) for s in lists.values()) == RR.entry_count(rec)
    some = [0, 4, tw * th - 1, tw + 2]
    got = RR.render_tiles(rec, cam, some)
    loop = RR.render_tiles(rec, cam, some, blend=RR._blend)
    assert sorted(got) == sorted(some)
    for t in some:
        vv, uu = RR.tile_pixels(cam, t)
        assert np.array_equal(got[t], want[vv, uu]) and np.array_equal(loop[t], want[vv, uu]), t
    everything = RR.render_tiles(rec, cam, range(tw * th))
    img = np.zeros_like(want)
    for t, px in everything.items():
        vv, uu = RR.tile_pixels(cam, t)
        img[vv, uu] = px
    assert np.array_equal(img, want)
    # the decisions: used pairs, marginal pairs per pixel, stopped pixels, clamped alphas
    dec = GR.decisions(c, 3, cam, aa)
    vec = GR.decisions(c, 3, cam, aa, vectorised=True)
    assert dec["stopped"] >= 190 and (aa or dec["clamped"] >= 1) and dec["used"] >= 18000
    for k in ("entries", "used", "stopped", "clamped", "marginal"):
        assert dec[k] == vec[k], k
    assert np.array_equal(dec["marginal_mask"], vec["marginal_mask"])
    for a, b in zip(dec["tiles"], vec["tiles"]):
        assert np.array_equal(a["sel"], b["sel"]) and np.array_equal(a["take"], b["take"])
        assert np.array_equal(a["marginal"], b["marginal"])


def test_marginal_mask_sums_to_the_marginal_count():
    """decisions() keeps the marginal pairs per pixel: they sum to its count, and the mask marks their pixels.  The
    scene is made to have some: Gaussians whose peak alpha is 1/255 to within 1e-5 relative, each on a pixel centre."""
    import render_grad_ref as GR
    cam = cam_at_origin()
    alpha = float(np.log((1.0 / 255.0) / (1.0 - 1.0 / 255.0)))  # opacity 1/255
    px = [(10, 7), (40, 30), (41, 30)]
    c = cat(one([0, 0, 6], 0.0, 2.0, colour_of([0.2, 0.6, 0.4])),
            *[one([(u - 32) * 5 / 50.0, (v - 24) * 5 / 50.0, 5], -1.0, alpha, colour_of([0.9, 0.1, 0.3])) for u, v in px])
    for vectorised in (False, True):
        dec = GR.decisions(c, 0, cam, vectorised=vectorised)
        per_pixel = np.zeros((cam["height"], cam["width"]), dtype=np.int64)
        for t in dec["tiles"]:
            per_pixel[t["v"], t["u"]] = t["marginal"]
        assert dec["marginal"] == per_pixel.sum() >= len(px)
        assert np.array_equal(dec["marginal_mask"], per_pixel > 0)
        for u, v in px:
            assert dec["marginal_mask"][v, u], (u, v)
        assert dec["marginal_mask"].sum() < 20


def test_look_at_projects_target_to_the_principal_point():
    import spz_amd.spz as spz
    eye, target, up = np.array([1.0, 2.0, -3.0]), np.array([0.5, -1.0, 4.0]), np.array([0.0, 0.0, 1.0])
    m = spz.look_at(eye, target, up).astype(np.float64)
    assert m.shape == (3, 4)
    assert np.allclose(m[:, :3] @ m[:, :3].T, np.eye(3), atol=1e-6) and np.linalg.det(m[:, :3]) > 0
    fx = fy = 100.0
    cx, cy = 64.0, 48.0

    def proj(p):
        x, y, z = m[:, :3] @ p + m[:, 3]
        return fx * x / z + cx, fy * y / z + cy, z

    u, v, z = proj(target)
    assert z > 0 and np.isclose(u, cx, atol=1e-4) and np.isclose(v, cy, atol=1e-4)
    u, v, _ = proj(target + 0.5 * up)
    assert v < cy - 1.0
    assert np.allclose(m, RR.look_at(eye, target, up), atol=1e-6)
    for bad in ((eye, eye, up), (eye, target, [0, 0, 0]), (eye, target, target - eye)):
        with pytest.raises(ValueError):
            spz.look_at(*bad)


def good_params():
    from spz_amd import abi
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    return abi.render_params(m, 100.0, 100.0, 50.0, 40.0, 100, 80)


def test_params_check_and_workspace_without_a_gpu():
    from spz_amd import abi
    L = abi.load_library()
    p = good_params()
    assert L.spz_amd_render_check_params(C.byref(p)) == 0
    assert L.spz_amd_render_check_params(None) == abi.ERR_INVALID_ARG

    def bad(**kw):
        q = good_params()
        for k, v in kw.items():
            if k == "R":  # (index, factor)
                q.world_to_camera[v[0]] = q.world_to_camera[v[0]] * v[1]
            else:
                setattr(q, k, v)
        return L.spz_amd_render_check_params(C.byref(q))

    for kw in (dict(R=(0, 1.001)), dict(R=(5, 0.01)), dict(R=(3, float("nan"))), dict(R=(11, float("inf"))),
               dict(fx=0.0), dict(fy=-2.0), dict(cx=float("inf")), dict(width=0), dict(height=16385), dict(near_plane=0.0),
               dict(near_plane=float("nan")), dict(max_sh_degree=4), dict(max_sh_degree=-1), dict(coord=9)):
        assert bad(**kw) == abi.ERR_INVALID_ARG, kw
    mirror = good_params()
    for k in range(4):
        mirror.world_to_camera[k] = -mirror.world_to_camera[k]
    assert L.spz_amd_render_check_params(C.byref(mirror)) == abi.ERR_INVALID_ARG  # det R = -1
    assert bad(R=(0, 1.00005)) == 0  # within 1e-4
    with pytest.raises(ValueError):
        abi.render_params(np.eye(3), 1, 1, 0, 0, 10, 10)
    # the prepare part is a prefix; the entries part grows with max_entries
    w0, w1, w2 = (int(L.spz_amd_render_workspace_bytes(1000, m)) for m in (0, 1, 10 ** 6))
    assert w0 >= 1000 * 48 and w0 < w1 < w2
    assert w2 - w1 >= (10 ** 6 - 1) * 16
    assert int(L.spz_amd_render_workspace_bytes(0, 0)) > 0


def test_cli_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_render")
    src = str(tmp_path / "missing.spz")
    base = ["--size", "64", "48", "--fov-y", "60", "--eye", "0", "0", "-5", "--target", "0", "0", "0"]
    cases = [
        [],
        [src],
        [src, str(tmp_path / "o.png")] + base,
        [src, str(tmp_path / "o.ppm")] + base[:3] + base[5:],           # no camera model
        [src, str(tmp_path / "o.ppm")] + base + ["--intrinsics", "1", "1", "0", "0"],  # both models
        [src, str(tmp_path / "o.ppm"), "--size", "0", "48"] + base[3:],
        [src, str(tmp_path / "o.ppm"), "--size", "64", "16385"] + base[3:],
        [src, str(tmp_path / "o.ppm")] + base + ["--sh-degree", "4"],
        [src, str(tmp_path / "o.ppm")] + base + ["--near", "0"],
        [src, str(tmp_path / "o.ppm")] + base + ["--coord", "XYZ"],
        [src, str(tmp_path / "o.ppm")] + base + ["--up", "0", "0", "1"],  # parallel to the view direction
        [src, str(tmp_path / "o.ppm")] + base[:8],                       # no --target
        [src, str(tmp_path / "o.ppm")] + base + ["--sh-degree", ""],
        [src, str(tmp_path / "o.ppm")] + base + ["--sh-degree", "1", "--sh-degree", "2"],   # repeated options
        [src, str(tmp_path / "o.ppm")] + base + ["--near", "1", "--near", "2"],
        [src, str(tmp_path / "o.ppm")] + base + ["--background", "0", "0", "0", "--background", "1", "1", "1"],
        [src, str(tmp_path / "o.ppm")] + base + ["--coord", "RUB", "--coord", "RDF"],
        [src, str(tmp_path / "o.ppm")] + base + ["--eye", "0", "0", "-6"],
    ]
    for args in cases:
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "Usage: spz_render" in r.stderr, args
