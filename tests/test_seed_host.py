"""The host side of seed (include/spz_amd.h "seed"; DESIGN §8 "Seed"), no GPU: the option check, the lattice count, the
refusals of spz.seed_spz, spz::seedSpz (through spz_seed) and spz_seed before any device work, and one property of the
reference alone that pins the default scale and opacity as consistent with the default cover test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_ref as DR
import render_ref as RR
import seed_ref as SR
from seed_ref import write_pfm, write_views
from conftest import ROOT

TOOL = os.path.join(ROOT, "spz_amd", "bin", "spz_seed")
USAGE = "Usage: spz_seed <out.spz>"
W, H, F = 8, 6, 10.0


# ---- the C ABI's host-only entries -----------------------------------------------------------------------------------
def test_seed_check_accepts_the_defaults_and_refuses_each_bad_option():
    from spz_amd import abi
    L = abi.load_library()
    o = abi.SeedOptions()
    assert L.spz_amd_seed_default_options(C.byref(o)) == abi.OK
    assert (o.stride, o.scale_factor, o.alpha, o.cover_alpha, o.cover, o.sh_degree) == (1, 1.0, 0.0, 0.5, 1, 0)
    assert o.cover_tolerance == np.float32(0.05)
    assert L.spz_amd_seed_check(C.byref(o)) == abi.OK
    assert L.spz_amd_seed_check(None) == abi.ERR_INVALID_ARG
    nan, inf = float("nan"), float("inf")
    bad = [("stride", 0), ("stride", 65), ("scale_factor", 0.0), ("scale_factor", -1.0), ("scale_factor", nan),
           ("scale_factor", inf), ("alpha", nan), ("alpha", inf), ("cover_alpha", -0.01), ("cover_alpha", 1.01),
           ("cover_alpha", nan), ("cover_tolerance", -0.01), ("cover_tolerance", nan), ("cover_tolerance", inf),
           ("cover", 2), ("cover", -1), ("sh_degree", -1), ("sh_degree", 4)]
    for k, v in bad:
        x = abi.SeedOptions.from_buffer_copy(o)
        setattr(x, k, v)
        assert L.spz_amd_seed_check(C.byref(x)) == abi.ERR_INVALID_ARG, (k, v)
    good = [("stride", 64), ("scale_factor", 1e-3), ("alpha", -7.5), ("cover_alpha", 0.0), ("cover_alpha", 1.0),
            ("cover_tolerance", 0.0), ("cover", 0), ("sh_degree", 3)]
    for k, v in good:
        x = abi.SeedOptions.from_buffer_copy(o)
        setattr(x, k, v)
        assert L.spz_amd_seed_check(C.byref(x)) == abi.OK, (k, v)


def test_seed_options_helper():
    from spz_amd import abi
    o = abi.seed_options(stride=3, opacity=0.5, cover=False, sh_degree=2)
    assert (o.stride, o.alpha, o.cover, o.sh_degree) == (3, 0.0, 0, 2)
    assert abi.seed_options(opacity=0.1).alpha == np.float32(np.log(0.1 / 0.9))
    for kw in (dict(opacity=0.0), dict(opacity=1.0), dict(opacity=float("nan")), dict(stride=0), dict(stride=True),
               dict(scale_factor=0.0), dict(cover_alpha=2.0), dict(cover_tolerance=-1.0), dict(sh_degree=4),
               dict(colour=1)):
        with pytest.raises(ValueError, match="seed"):
            abi.seed_options(**kw)


def test_seed_samples_equals_the_reference_lattice():
    from spz_amd import abi
    L = abi.load_library()
    for width in (1, 2, 3, 7, 8, 63, 64, 65, 255, 257):
        for height in (1, 5, 48):
            for stride in (1, 2, 3, 4, 5, 8, 63, 64):      # width < stride, width % stride != 0, width < stride / 2
                want = SR.samples(width, height, stride)
                assert abi.seed_samples(width, height, stride) == want, (width, height, stride)
                u, v, (lw, lh) = SR.lattice(width, height, stride)
                assert len(u) == want == lw * lh and (want == 0 or (u.max() < width and v.max() < height))
                assert L.spz_amd_seed_workspace_bytes(width, height, stride) >= want
    assert abi.seed_samples(1, 1, 4) == 0 and abi.seed_samples(3, 3, 4) == 1
    for width, height, stride in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 4, 0), (4, 4, 65)):
        assert abi.seed_samples(width, height, stride) == 0
        assert L.spz_amd_seed_workspace_bytes(width, height, stride) == 0


# ---- refusals before any device work ---------------------------------------------------------------------------------
def view_dict(width=W, height=H):
    return {"world_to_camera": RR.look_at([0, 0, -3], [0, 0, 0], [0, 1, 0]), "fx": F, "fy": F, "cx": 0.5 * width,
            "cy": 0.5 * height, "width": width, "height": height}


def maps(width=W, height=H):
    return np.full((height, width, 3), 0.5, np.float32), np.full((height, width), 2.0, np.float32)


PY_ROWS = [
    ("wrong image size", lambda s: s.seed_spz([view_dict()], [maps(W + 1, H)[0]], [maps()[1]]), ValueError,
     r"images\[0\] must be the view's height x width"),
    ("wrong depth size", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps(W, H + 1)[1]]), ValueError,
     r"depths\[0\] must be a float32 array of the view's height x width"),
    ("missing depth", lambda s: s.seed_spz([view_dict()] * 2, [maps()[0]] * 2, [maps()[1], None]), ValueError,
     "seed_spz: refused"),
    ("no depths", lambda s: s.seed_spz([view_dict()], [maps()[0]], None), ValueError, "depths must be a sequence"),
    ("fewer images", lambda s: s.seed_spz([view_dict()] * 2, [maps()[0]], [maps()[1]] * 2), ValueError,
     "2 views, 1 images"),
    ("fewer depths", lambda s: s.seed_spz([view_dict()] * 2, [maps()[0]] * 2, [maps()[1]]), ValueError,
     "2 views, 1 depths"),
    ("fewer masks", lambda s: s.seed_spz([view_dict()] * 2, [maps()[0]] * 2, [maps()[1]] * 2, masks=[None]), ValueError,
     "2 views, 1 weights"),
    ("opacity 0", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], opacity=0.0), ValueError,
     r"opacity must be in \(0, 1\)"),
    ("opacity 1", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], opacity=1.0), ValueError,
     r"opacity must be in \(0, 1\)"),
    ("opacity nan", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], opacity=float("nan")), ValueError,
     r"opacity must be in \(0, 1\)"),
    ("stride", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], stride=65), ValueError, "stride must be"),
    ("sh_degree", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], sh_degree=4), ValueError, "sh_degree"),
    ("cover", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], cover=1), ValueError, "cover must be a bool"),
    ("max_points", lambda s: s.seed_spz([view_dict()], [maps()[0]], [maps()[1]], max_points=10**7 + 1), ValueError,
     "max_points"),
    ("no views", lambda s: s.seed_spz([], [], []), ValueError, "give 1..1024 views"),
]


@pytest.mark.parametrize("name,call,kind,message", PY_ROWS, ids=[r[0] for r in PY_ROWS])
def test_seed_spz_answers_a_bad_argument(name, call, kind, message, capfd):
    import spz_amd.spz as spz
    with pytest.raises(kind, match=message):
        call(spz)
    if name == "missing depth":  # the C++ layer's own line names the view
        assert "[SPZ ERROR] seedSpz: image 1 has no depth" in capfd.readouterr().out


def run(args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=60)


def test_spz_seed_refuses_bad_arguments(tmp_path):
    out, views = tmp_path / "out.spz", tmp_path / "views.txt"
    write_views(views, [view_dict(), view_dict()])
    rgb, z = maps()
    im, zm, big, zbig = (tmp_path / n for n in ("a.pfm", "z.pfm", "big.pfm", "zbig.pfm"))
    write_pfm(im, rgb, b"PF")
    write_pfm(zm, z, b"Pf")
    write_pfm(big, maps(W + 2, H)[0], b"PF")
    write_pfm(zbig, maps(W + 2, H)[1], b"Pf")
    base = [out, "--views", views]
    # the tool's own reader: what is missing or malformed is the usage line
    for args in ([], [out], base, base + ["--images", im, im], base + ["--depths", zm, zm],
                 base + ["--images", im, im, "--depths", zm, zm, "--stride", "0"],
                 base + ["--images", im, im, "--depths", zm, zm, "--stride", "65"],
                 base + ["--images", im, im, "--depths", zm, zm, "--sh-degree", "4"],
                 base + ["--images", im, im, "--depths", zm, zm, "--cover-alpha", "1.5"],
                 base + ["--images", im, im, "--depths", zm, zm, "--cover-tolerance", "-1"],
                 base + ["--images", im, im, "--depths", zm, zm, "--scale-factor", "0"],
                 base + ["--images", im, im, "--depths", zm, zm, "--opacity"],
                 base + ["--images", im, im, "--depths", zm, zm, "--orbit", "3"],
                 base + ["--images", im, im, "--depths", zm, zm, "--bogus"]):
        r = run(args)
        assert r.returncode == 1 and USAGE in r.stderr, args
    # images against depths and masks is the tool's to count
    r = run(base + ["--images", im, im, "--depths", zm])
    assert r.returncode == 1 and "[SPZ ERROR] spz_seed: 2 images but 1 depths" in r.stderr and USAGE in r.stderr
    r = run(base + ["--images", im, im, "--depths", zm, zm, "--masks", im])
    assert r.returncode == 1 and "2 images but 2 depths and 1 masks" in r.stderr
    # a depth map that is not its image's size names both files
    r = run(base + ["--images", im, im, "--depths", zm, zbig])
    assert r.returncode == 1 and f"{im} is {W} x {H} but {zbig} is {W + 2} x {H}" in r.stderr and USAGE not in r.stderr
    # spz::seedSpz's refusals, by its own line, before any device work
    r = run(base + ["--images", im, "--depths", zm])
    assert r.returncode == 1 and "[SPZ ERROR] seedSpz: 2 views but 1 images" in r.stdout
    r = run(base + ["--images", im, big, "--depths", zm, zbig])
    assert r.returncode == 1 and f"[SPZ ERROR] seedSpz: view 1 is {W} x {H} but its image is {W + 2} x {H}" in r.stdout
    for opacity in ("0", "1", "1.5", "nan"):
        r = run(base + ["--images", im, im, "--depths", zm, zm, "--opacity", opacity])
        assert r.returncode == 1 and "[SPZ ERROR] seedSpz: opacity must be in (0, 1)" in r.stdout, opacity
    r = run(base + ["--images", im, im, "--depths", zm, zm, "--onto", tmp_path / "missing.spz"])
    assert r.returncode == 1 and "[SPZ ERROR]" in r.stdout + r.stderr and USAGE not in r.stderr
    assert not out.exists()
    r = run([out, "--views", tmp_path / "missing.txt", "--images", im, "--depths", zm])
    assert r.returncode == 1 and "missing.txt" in r.stderr


def test_spz_seed_is_listed():
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "|spz_seed|" in r.stderr


# ---- the defaults are consistent: a view seeded twice appends nothing in its interior ---------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_reference_seeding_a_view_twice_appends_nothing_inside(stride):
    """A fronto-parallel textured plane at z = 2 seen by one 32 x 24 view.  The first pass lifts every lattice sample; the
    second renders them (render_ref / depth_ref) and must find every interior sample covered: alpha >= cover_alpha = 0.5
    and the expected depth within 5 % of the measurement, with the default scale factor 1 and opacity 0.5."""
    width, height, f, z = 32, 24, 28.0, 2.0
    vw = SR.view(RR.look_at([0, 0, -z], [0, 0, 0], [0, 1, 0]), f, f, 0.5 * width, 0.5 * height, width, height)
    rng = np.random.default_rng(5)
    vv, uu = np.mgrid[0:height, 0:width]
    image = np.stack([0.5 + 0.4 * np.sin(0.7 * uu), 0.5 + 0.4 * np.cos(0.5 * vv), rng.uniform(0.1, 0.9, (height, width))],
                     axis=-1).astype(np.float32)
    depth = np.full((height, width), z, np.float32)
    opts = SR.options(stride=stride)
    assert opts["alpha"] == 0.0 and opts["cover_alpha"] == 0.5 and opts["scale_factor"] == 1.0
    cam = RR.camera(vw["world_to_camera"], vw["fx"], vw["fy"], vw["cx"], vw["cy"], width, height, near=vw["near"],
                    max_sh_degree=0)

    def render_depth(cloud, n, _view):
        head = {k: cloud[k][: n * (cloud[k].size // capacity)] for k in SR.FIELDS}
        m = DR.render_depth(head, 0, cam)
        ci = np.zeros((height, width, 4), np.float32)
        ci[..., 3] = m["alpha"]
        cd = np.zeros((height, width, 2), np.float32)
        cd[..., 0] = m["accumulated"]
        return ci, cd

    capacity = 2 * SR.samples(width, height, stride)
    cloud, n, counts = SR.seed_loop([vw, vw], [image, image], [depth, depth], None, opts, capacity, render_depth)
    total = SR.samples(width, height, stride)
    assert counts[0] == (total, total, 0) and n == total + counts[1][1]
    assert counts[1][0] == total
    # which samples the second pass appended: none more than 3 sigma from the image's edge (sigma in pixels: the scale
    # is one lattice step, and the rasteriser adds 0.3 to the variance)
    ci, cd = render_depth(cloud, total, vw)
    flags, _ = SR.select(vw, image, depth, None, ci, cd, opts)
    u, v, _ = SR.lattice(width, height, stride)
    margin = 3.0 * np.sqrt(stride * stride + 0.3)
    inside = (u > margin) & (u < width - 1 - margin) & (v > margin) & (v < height - 1 - margin)
    assert inside.sum() > 0.2 * total
    again = (flags & SR.SELECTED) != 0
    assert not (again & inside).any(), f"{int((again & inside).sum())} interior samples seeded twice"
    # and the positions the first pass wrote are cameras.unproject_depth's, on the plane z = 0 of the world
    from spz_amd import cameras
    P = cloud["positions"][: 3 * total].reshape(-1, 3)
    want = cameras.unproject_depth(depth, vw["world_to_camera"], vw["fx"], vw["fy"], vw["cx"], vw["cy"])
    assert np.abs(P[:, 2]).max() < 1e-6
    assert np.allclose(P, want[v * width + u], rtol=0, atol=1e-6)
    assert np.allclose(np.exp(cloud["scales"][: 3 * total]), stride * z / f, rtol=1e-6)
