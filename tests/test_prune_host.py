"""Significance pruning without a GPU (DESIGN §8 "Prune"): tests/prune_ref.py on analytic scenes, the argument checks
of spz.prune_spz and of the C ABI, the views-file parser, spz.load_3dgs_cameras, spz.orbit_views and spz_prune's usage
errors."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import prune_ref as PR
import render_ref as RR
from conftest import ROOT


def one(pos, log_scale, alpha, colour=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0)):
    return {"positions": np.float32(pos), "scales": np.float32([log_scale] * 3), "rotations": np.float32(rot),
            "alphas": np.float32([alpha]), "colors": np.float32(colour), "sh": np.zeros(0, np.float32)}


def cat(*clouds):
    return {k: np.concatenate([c[k] for c in clouds]) for k in clouds[0]}


def cam_at_origin(w=70, h=45):
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    return RR.camera(m, 50.0, 50.0, 35.5, 22.5, w, h)


def test_three_opaque_screens_the_third_scores_zero():
    cam = cam_at_origin()
    screens = cat(*(one([0, 0, z], 4.0, 12.0) for z in (4.0, 6.0, 8.0)))
    wsum, wmax, alpha = PR.view_scores(screens, 0, cam)
    assert wsum[0] > 0 and wsum[1] > 0
    assert wsum[2] == 0.0 and wmax[2] == 0.0
    assert np.isclose(wmax[0], 0.99) and np.isclose(wmax[1], 0.99 * 0.01)
    assert np.isclose(wsum.sum(), alpha, rtol=1e-12)


def test_outside_the_frustum_and_behind_the_near_plane_score_zero():
    cam = cam_at_origin()
    c = cat(one([0, 0, 5], -1.0, 2.0), one([100, 0, 5], -1.0, 2.0), one([0, 0, 0.1], -1.0, 2.0),
            one([0, 0, -3], 0.0, 2.0))
    wsum, wmax = PR.scores(c, 0, [cam, cam_at_origin(33, 17)])
    assert wsum[0] > 0 and wmax[0] > 0
    assert not wsum[1:].any() and not wmax[1:].any()


def test_lone_splat_sum_is_its_pixels():
    cam = cam_at_origin()
    c = one([0.3, -0.2, 5], -0.8, 0.5, rot=(0.2, 0.1, 0.3, 0.9))
    rec = RR.preprocess(c, 0, cam)
    wsum, wmax, alpha = PR.view_scores(c, 0, cam, rec=rec)
    x0, y0, x1, y1 = (int(v) for v in rec["rect"][0])
    vv, uu = np.mgrid[y0 * 16:min(cam["height"], y1 * 16), x0 * 16:min(cam["width"], x1 * 16)].astype(np.float64)
    dx, dy = uu - float(rec["mean"][0, 0]), vv - float(rec["mean"][0, 1])
    A, B, Cc = rec["conic"][0].astype(np.float64)
    power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
    a = np.minimum(0.99, float(rec["opacity"][0]) * np.exp(np.minimum(power, 0.0)))
    used = (power <= 0) & (a >= 1 / 255)
    assert np.isclose(wsum[0], a[used].sum(), rtol=1e-12)
    assert np.isclose(wmax[0], a[used].max(), rtol=1e-12)
    assert np.isclose(alpha, wsum[0], rtol=1e-12)


def test_sum_telescopes_to_the_alpha_sum():
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(200, 0, 3)
    c["positions"] = (c["positions"].reshape(-1, 3) * 0.3 + [0, 0, 6]).astype(np.float32).reshape(-1)
    c["scales"] = (c["scales"] * 0.5 - 2.0).astype(np.float32)
    cam = cam_at_origin()
    wsum, wmax, alpha = PR.view_scores(c, 0, cam)
    assert alpha > 1.0
    assert np.isclose(wsum.sum(), alpha, rtol=1e-12)
    assert (wmax <= 0.99).all()


def test_keep_mask_ranks_by_score_then_index():
    s = np.array([3, 0, 5, 3, 0, 1], dtype=np.uint64)
    assert PR.keep_mask(s, "keep", 3).tolist() == [True, False, True, True, False, False]
    assert PR.keep_mask(s, "keep", 5).tolist() == [True, True, True, True, False, True]
    assert PR.keep_mask(s, "keep_fraction", 0.5).tolist() == [True, False, True, True, False, False]
    assert PR.keep_mask(s.astype(np.float32), "min_score", 3).tolist() == [True, False, True, True, False, False]


# ---- arguments -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


def a_view(**kw):
    v = {"world_to_camera": RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), "fx": 50.0, "fy": 50.0, "cx": 32.0,
         "cy": 24.0, "width": 64, "height": 48}
    v.update(kw)
    return v


@pytest.mark.parametrize("kw,msg", [
    ({}, "exactly one"),
    ({"keep": 3, "keep_fraction": 0.5}, "exactly one"),
    ({"keep": 3, "min_score": 1.0}, "exactly one"),
    ({"keep": -1}, "keep"),
    ({"keep": 2.5}, "keep"),
    ({"keep": True}, "keep"),
    ({"keep_fraction": 1.5}, "keep_fraction"),
    ({"keep_fraction": -0.1}, "keep_fraction"),
    ({"keep_fraction": float("nan")}, "keep_fraction"),
    ({"min_score": float("inf")}, "min_score"),
    ({"keep": 1, "score": "mean"}, "score"),
])
def test_prune_spz_rules_are_checked_first(spz, tmp_path, kw, msg):
    with pytest.raises(ValueError, match=msg):
        spz.prune_spz(str(tmp_path / "missing.spz"), str(tmp_path / "out.spz"), [a_view()], **kw)
    assert not (tmp_path / "out.spz").exists()


def test_prune_spz_views_are_checked_first(spz, tmp_path):
    out = str(tmp_path / "out.spz")
    with pytest.raises(ValueError, match="1..1024"):
        spz.prune_spz("missing.spz", out, [], keep=1)
    with pytest.raises(ValueError, match="1..1024"):
        spz.prune_spz("missing.spz", out, [a_view()] * 1025, keep=1)
    bad = np.eye(3, 4, dtype=np.float32) * 2
    with pytest.raises(ValueError, match="view 3: bad camera"):
        spz.prune_spz("missing.spz", out, [a_view()] * 3 + [a_view(world_to_camera=bad)], keep=1)
    with pytest.raises(ValueError, match="view 1: bad camera"):
        spz.prune_spz("missing.spz", out, [a_view(), a_view(width=0)], keep=1)
    with pytest.raises(ValueError, match="view 2: has no fx"):
        v = a_view()
        del v["fx"]
        spz.prune_spz("missing.spz", out, [a_view(), a_view(), v], keep=1)
    with pytest.raises(ValueError, match="view 1: its coord differs"):
        spz.prune_spz("missing.spz", out, [a_view(coord=spz.RDF), a_view(coord=spz.RUB)], keep=1, coord=spz.RDF)
    with pytest.raises(ValueError, match="views must be a sequence"):
        spz.prune_spz("missing.spz", out, a_view(), keep=1)
    assert not os.path.exists(out)


def test_c_abi_checks_the_views_before_any_device_work():
    from spz_amd import abi
    L = abi.load_library()
    h = abi.Header()
    h.num_points, h.sh_degree, h.version, h.fractional_bits = 10, 0, 3, 12
    buf = (C.c_uint8 * 4096)()
    good = abi.render_params(RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), 50, 50, 32, 24, 64, 48, coord=abi.RUB)

    def call(views, rule=abi.PRUNE_KEEP_COUNT, value=1.0, kind=abi.PRUNE_SCORE_SUM, stream=buf, hdr=h):
        arr = (abi.RenderParams * max(1, len(views)))(*views)
        ctx, nbytes, bad = C.c_void_p(), C.c_uint64(), C.c_int32(7)
        rc = L.spz_amd_prune_open(stream, 4096, C.byref(hdr), arr, len(views), kind, rule, value, 0, C.byref(ctx),
                                  C.byref(nbytes), None, None, None, None, None, C.byref(bad))
        assert not ctx.value
        return rc, bad.value

    assert call([]) == (abi.ERR_INVALID_ARG, -1)
    assert call([good] * 1025) == (abi.ERR_INVALID_ARG, -1)
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.fx = -1.0
    assert call([good, good, worse]) == (abi.ERR_INVALID_ARG, 2)
    assert call([worse, good, good]) == (abi.ERR_INVALID_ARG, 0)
    other = abi.RenderParams.from_buffer_copy(good)
    other.coord = abi.RDF
    assert call([good, other]) == (abi.ERR_INVALID_ARG, 1)
    assert call([good, other], stream=None) == (abi.ERR_INVALID_ARG, -1)    # no stream: before the views
    assert call([good, other], kind=2) == (abi.ERR_INVALID_ARG, 1)          # the views: before the score kind,
    big = abi.Header.from_buffer_copy(h)
    big.num_points = 0x80000000
    assert call([good, other], hdr=big) == (abi.ERR_INVALID_ARG, 1)         # and before the input;
    assert call([good], hdr=big)[0] == abi.ERR_TOO_MANY_POINTS              # the point count before the short stream
    big.sh_degree = 4
    assert call([good], hdr=big)[0] == abi.ERR_SH_DEGREE
    big.version = 4
    assert call([good], hdr=big)[0] == abi.ERR_VERSION
    assert call([good], kind=2)[0] == abi.ERR_INVALID_ARG
    assert call([good], rule=3)[0] == abi.ERR_INVALID_ARG
    assert call([good], value=11.0)[0] == abi.ERR_INVALID_ARG       # K above n
    assert call([good], value=2.5)[0] == abi.ERR_INVALID_ARG        # K not an integer
    assert call([good], rule=abi.PRUNE_KEEP_FRACTION, value=1.01)[0] == abi.ERR_INVALID_ARG
    assert call([good], rule=abi.PRUNE_MIN_SCORE, value=float("nan"))[0] == abi.ERR_INVALID_ARG


def test_keep_count_of_a_fraction():
    from spz_amd import abi
    L = abi.load_library()

    def k(n, f):
        out = C.c_uint64()
        assert L.spz_amd_prune_keep_count(n, abi.PRUNE_KEEP_FRACTION, f, C.byref(out)) == abi.OK
        return out.value

    assert k(10, 0.0) == 0 and k(10, 1.0) == 10 and k(10, 0.31) == 4 and k(10, 0.3) == 3 and k(0, 0.5) == 0
    assert k(3, 1e-9) == 1
    out = C.c_uint64()
    assert L.spz_amd_prune_keep_count(5, abi.PRUNE_KEEP_COUNT, 5.0, C.byref(out)) == abi.OK and out.value == 5
    assert L.spz_amd_prune_keep_count(5, abi.PRUNE_KEEP_COUNT, 6.0, C.byref(out)) == abi.ERR_INVALID_ARG
    assert L.spz_amd_prune_keep_count(5, abi.PRUNE_KEEP_COUNT, -1.0, C.byref(out)) == abi.ERR_INVALID_ARG


# ---- camera sets ---------------------------------------------------------------------------------------------------

def test_views_file_parser(spz, tmp_path):
    p = tmp_path / "views.txt"
    m = RR.look_at([1, 2, -5], [0, 0, 0], [0, 1, 0])
    line = " ".join(["64", "48", "50", "51", "32", "24.5"] + [repr(float(v)) for v in m.reshape(-1)])
    p.write_text(f"# two views\n{line}\n\n   {line}  # the same again\n")
    v = spz.load_views_file(str(p))
    assert len(v) == 2
    assert v[0]["width"] == 64 and v[0]["height"] == 48 and v[0]["fy"] == 51.0 and v[0]["cy"] == 24.5
    assert np.array_equal(v[1]["world_to_camera"], m)
    for body, msg in [("64 48 50\n", "line 1: expected 18"), (f"# x\n{line} 7\n", "line 2: expected 18"),
                      (line.replace("24.5", "abc") + "\n", "'abc'"), (line.replace("64", "64.5", 1) + "\n", "integers"),
                      (line.replace("24.5", "nan") + "\n", "'nan'"), ("# nothing\n\n", "holds no view")]:
        p.write_text(body)
        with pytest.raises(ValueError, match=msg):
            spz.load_views_file(str(p))
    with pytest.raises(ValueError, match="unable to open"):
        spz.load_views_file(str(tmp_path / "none.txt"))


def test_load_3dgs_cameras(spz, tmp_path):
    rng = np.random.default_rng(5)
    cams = []
    for k in range(4):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        cams.append({"id": k, "img_name": f"{k:05d}", "width": 80 + k, "height": 60, "position": rng.normal(size=3).tolist(),
                     "rotation": q.tolist(), "fy": 70.0, "fx": 71.0})
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps(cams))
    views = spz.load_3dgs_cameras(str(path))
    assert len(views) == 4
    for c, v in zip(cams, views):
        m = np.asarray(v["world_to_camera"], dtype=np.float64)
        R, t = m[:, :3], m[:, 3]
        centre, axis = np.asarray(c["position"]), np.asarray(c["rotation"])[:, 2]
        assert np.allclose(R @ centre + t, 0, atol=1e-5)                    # the camera centre maps to the origin
        assert np.allclose(R @ axis, [0, 0, 1], atol=1e-5)                   # the viewing axis maps to +z
        assert v["cx"] == c["width"] / 2 and v["cy"] == 30.0 and v["fx"] == 71.0 and v["fy"] == 70.0
        from spz_amd import abi
        abi.render_params(m, v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"], coord=abi.RDF)
    path.write_text(json.dumps([{"width": 4}]))
    with pytest.raises(ValueError, match="camera 0 lacks"):
        spz.load_3dgs_cameras(str(path))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 1024])
def test_orbit_views_look_at_the_centre(spz, n):
    from spz_amd import abi
    centre, radius = np.array([1.0, -2.0, 3.0]), 2.0
    views = spz.orbit_views(n, width=96, height=64, fov_y=50.0, center=centre.tolist(), radius=radius, distance=3.0)
    assert len(views) == n
    eyes = []
    for v in views:
        m = np.asarray(v["world_to_camera"], dtype=np.float64)
        abi.render_params(m, v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"])
        R, t = m[:, :3], m[:, 3]
        c = R @ centre + t
        assert np.allclose(c[:2], 0, atol=1e-4) and np.isclose(c[2], 6.0, rtol=1e-5)
        eyes.append(-R.T @ t)
        assert np.isclose(v["fy"], 32.0 / np.tan(np.radians(25.0)), rtol=1e-6) and v["cx"] == 48.0
    eyes = np.array(eyes)
    assert np.allclose(np.linalg.norm(eyes - centre, axis=1), 6.0, rtol=1e-5)
    if n > 1:
        d = np.linalg.norm(eyes[:, None] - eyes[None], axis=2) + np.eye(n) * 1e9
        assert d.min() > 1e-3, "two views coincide"
    if n == 1024:  # the Fibonacci sphere reaches within 2.6 degrees of both poles of +-y
        ys = (eyes[:, 1] - centre[1]) / 6.0
        assert ys.max() > 0.999 and ys.min() < -0.999


def test_orbit_views_arguments(spz):
    kw = dict(width=64, height=48, fov_y=50.0, center=[0, 0, 0], radius=1.0)
    for bad in [dict(n=0), dict(n=1025), dict(fov_y=0.0), dict(fov_y=180.0), dict(radius=0.0), dict(distance=-1.0),
                dict(width=0), dict(center=[0, float("nan"), 0])]:
        args = dict(kw, **bad)
        n = args.pop("n", 3)
        with pytest.raises(ValueError):
            spz.orbit_views(n, **args)
    with pytest.raises(ValueError, match="center and radius"):
        spz.orbit_views(3, width=64, height=48, fov_y=50.0)


def test_cli_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_prune")
    views = tmp_path / "v.txt"
    views.write_text("64 48 50 50 32 24 1 0 0 0 0 1 0 0 0 0 1 5\n")
    bad_views = tmp_path / "bad.txt"
    bad_views.write_text("64 48 50 50 32 24 1 0 0\n")
    base = ["in.spz", "out.spz"]
    for args in [[], ["in.spz"], base, base + ["--views", str(views)], base + ["--keep", "3"],
                 base + ["--views", str(views), "--keep", "3", "--keep-fraction", "0.5"],
                 base + ["--views", str(views), "--keep", "-3"],
                 base + ["--views", str(views), "--keep-fraction", "1.5"],
                 base + ["--views", str(views), "--min-score", "inf"],
                 base + ["--views", str(views), "--keep", "3", "--score", "mean"],
                 base + ["--views", str(views), "--keep", "3", "--coord", "XYZ"],
                 base + ["--views", str(views), "--orbit", "4", "--keep", "3"],
                 base + ["--orbit", "4", "--size", "64", "48", "--keep", "3"],
                 base + ["--orbit", "0", "--size", "64", "48", "--fov-y", "50", "--keep", "3"],
                 base + ["--orbit", "1025", "--size", "64", "48", "--fov-y", "50", "--keep", "3"],
                 base + ["--orbit", "4", "--size", "64", "48", "--fov-y", "50", "--center", "0", "0", "0", "--keep", "3"],
                 base + ["--orbit", "4", "--size", "64", "48", "--fov-y", "50", "--radius", "-1", "--keep", "3"],
                 base + ["--views", str(bad_views), "--keep", "3"],
                 base + ["--views", str(tmp_path / "none.txt"), "--keep", "3"]]:
        r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "Usage: spz_prune" in r.stderr, (args, r.stderr)
