"""The view backward and the pose fit without a GPU (include/spz_amd.h "render view backward" and "locate"; DESIGN §8
"Locate"): tests/view_grad_ref.py's gradients against central differences, the library's host-only update functions
against the numpy restatement, and the new entry points' signatures, argument checks and loud failure without a
device."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_grad_ref as GR
import render_ref as RR
import view_grad_ref as VR
from test_gpu_render import view_of

W, H = 40, 36
BG = (0.1, 0.2, 0.3)


def small_scene(aa):
    """The 12-Gaussian scene of test_render_grad_host.test_gradients_equal_central_differences."""
    c = GR.scene(3, 3, n=12)
    c["scales"] = (c["scales"] + 0.8).astype(np.float32)
    c["alphas"] = (c["alphas"] + 2.5).astype(np.float32)
    m, fx, fy, cx, cy = view_of(c["positions"], width=W, height=H)
    cam = RR.camera(m, fx, fy, cx, cy, W, H, 0.2, BG, 3)
    dec = GR.decisions(c, 3, cam, aa)
    assert dec["marginal"] == 0 and dec["visible"].all() and dec["used"] >= 1500 and dec["stopped"] >= 10
    G = np.random.default_rng(5).standard_normal((H, W, 4)).astype(np.float32)
    return c, cam, dec, G


def loss_at(cloud, cam, dec, aa, Gt, pose):
    c = dict(cam)
    c["R"], c["t"] = torch.as_tensor(pose[:, :3].copy()), torch.as_tensor(pose[:, 3].copy())
    with torch.no_grad():
        return float((GR.forward(cloud, 3, c, dec, aa, round_records=False)[0] * Gt).sum())


@pytest.mark.parametrize("aa", [False, True])
def test_view_gradient_equals_central_differences(aa):
    """Float64, records not rounded, L = sum(image * G), the 12 entries of [R | t] moved one at a time with the
    decisions held.  h = 1e-5 and the bound of 1e-6 of the largest entry are those of
    test_render_grad_host.test_gradients_equal_central_differences, whose docstring derives them.  The twist gradient
    is checked the same way against L(Exp(w) R, Exp(w) t + v)."""
    c, cam, dec, G = small_scene(aa)
    g = VR.view_gradient(c, 3, cam, dec, G, aa, round_records=False)["view"]
    Gt = torch.as_tensor(G).to(torch.float64)
    cloud = GR.as_tensors(c, torch.float64, requires_grad=False)
    pose = np.concatenate([cam["R"], cam["t"][:, None]], axis=1)
    h = 1e-5
    num = np.zeros((3, 4))
    for r in range(3):
        for k in range(4):
            up, down = pose.copy(), pose.copy()
            up[r, k] += h
            down[r, k] -= h
            num[r, k] = (loss_at(cloud, cam, dec, aa, Gt, up) - loss_at(cloud, cam, dec, aa, Gt, down)) / (2 * h)
    scale = np.abs(g).max()
    err = np.abs(num - g).max()
    print(f"view: largest gradient {scale:.3e}, central differences off by {err:.3e}")
    assert scale > 1e-3 and err <= 1e-6 * scale, (err, scale)
    # the rotation's part is not a multiple of the translation's: all three paths of R carry weight
    assert np.abs(g[:, :3]).max() > 1e-3

    tw = VR.twist_gradient(pose, g)
    num = np.zeros(6)
    for k in range(6):
        def moved(s):
            d = np.zeros(6)
            d[k] = s
            E = VR.so3_exp(d[:3])
            return np.concatenate([E @ pose[:, :3], (E @ pose[:, 3] + d[3:])[:, None]], axis=1)
        num[k] = (loss_at(cloud, cam, dec, aa, Gt, moved(h)) - loss_at(cloud, cam, dec, aa, Gt, moved(-h))) / (2 * h)
    scale = np.abs(tw).max()
    err = np.abs(num - tw).max()
    print(f"twist: largest gradient {scale:.3e}, central differences off by {err:.3e}")
    assert scale > 1e-3 and err <= 1e-6 * scale, (err, scale)


def test_the_chain_from_the_record_gradients_sums_to_the_view_gradient():
    """view_grad_ref.chain (what the device kernel is checked against) on the reference's own record gradients."""
    c, cam, dec, G = small_scene(False)
    g = VR.view_gradient(c, 3, cam, dec, G, False)
    per = VR.chain(c, 3, cam, dec, g["records"], False)
    assert per.shape == (12, 3, 4)
    assert np.abs(per.sum(axis=0) - g["view"]).max() <= 1e-12 * np.abs(per).sum(axis=0).max()


@pytest.mark.parametrize("aa", [False, True])
def test_the_forward_mode_chain_is_the_chain(aa):
    """chain(forward_mode=True), which scenes of tens of thousands of Gaussians use, gives chain()'s derivatives: the
    same float64 operations differentiated the other way round, so only the rounding of a few dozen operations per
    value apart (1e-12 of each Gaussian's largest contribution)."""
    c, cam, dec, G = small_scene(aa)
    rg = np.random.default_rng(9).standard_normal((12, 9))
    back = VR.chain(c, 3, cam, dec, rg, aa)
    fwd = VR.chain(c, 3, cam, dec, rg, aa, forward_mode=True)
    scale = np.abs(back).max(axis=(1, 2), keepdims=True)
    assert scale.min() > 0 and np.all(np.abs(fwd - back) <= 1e-12 * scale)


def dbl(a):
    return (C.c_double * len(a))(*[float(x) for x in a])


def test_host_update_functions_equal_the_restatement():
    """spz_amd_locate_twist_gradient, _pose_step and _level_params against view_grad_ref's numpy: the same f64
    operations, so to a few ulps; the small-angle branch of Exp is taken with tiny step sizes."""
    from spz_amd import abi
    L = abi.load_library()
    rng = np.random.default_rng(11)
    pose0 = VR.perturbed(RR.look_at([1, 2, -5], [0, 0, 0], [0, 1, 0]), 0.0, 0.0).astype(np.float64)
    for lr in (2e-3, 1e-7, 0.3):
        opts = {"iterations": 7, "lr_rotation": lr, "lr_translation": 3 * lr, "lr_final_factor": 0.25}
        o = abi.locate_options(**opts)
        pose, m, v = pose0.copy(), np.zeros(6), np.zeros(6)
        cp, cm, cv = dbl(pose0.reshape(-1)), dbl(np.zeros(6)), dbl(np.zeros(6))
        for i in range(7):
            G = rng.standard_normal((3, 4))
            if i == 3:
                G[:] = 0.0  # the moments still move the pose
            want_g = VR.twist_gradient(pose, G)
            got_g = dbl(np.zeros(6))
            assert L.spz_amd_locate_twist_gradient(cp, dbl(G.reshape(-1)), got_g) == abi.OK
            assert np.abs(np.array(got_g) - want_g).max() <= 1e-14 * max(1.0, np.abs(want_g).max())
            pose, m, v = VR.pose_step(opts, i, want_g, m, v, pose)
            assert L.spz_amd_locate_pose_step(C.byref(o), i, got_g, cm, cv, cp) == abi.OK
            assert np.abs(np.array(cp).reshape(3, 4) - pose).max() <= 1e-13
            assert np.abs(np.array(cm) - m).max() <= 1e-15 and np.abs(np.array(cv) - v).max() <= 1e-15
        R = np.array(cp).reshape(3, 4)[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6  # pose0 is a float32 matrix; Exp keeps what it is given
    # a zero gradient moves nothing, with eps = 0 too
    o = abi.locate_options(iterations=1, eps=0.0)
    cp, cm, cv = dbl(pose0.reshape(-1)), dbl(np.zeros(6)), dbl(np.zeros(6))
    assert L.spz_amd_locate_pose_step(C.byref(o), 0, dbl(np.zeros(6)), cm, cv, cp) == abi.OK
    assert np.array_equal(np.array(cp).reshape(3, 4), pose0)
    assert L.spz_amd_locate_pose_step(C.byref(o), 1, dbl(np.zeros(6)), cm, cv, cp) == abi.ERR_INVALID_ARG
    # levels
    p = good_params()
    cam = RR.camera(np.array(list(p.world_to_camera)).reshape(3, 4), p.fx, p.fy, p.cx, p.cy, p.width, p.height)
    for k in range(3):
        q = abi.locate_level_params(p, k)
        want = VR.level_camera(cam, k)
        assert (q.width, q.height, q.fx, q.fy, q.cx, q.cy) == (want["width"], want["height"], want["fx"], want["fy"],
                                                               want["cx"], want["cy"])
        assert list(q.world_to_camera) == list(p.world_to_camera)
    with pytest.raises(ValueError):
        abi.locate_level_params(p, 3)  # 100 is not divisible by 8
    assert VR.level_schedule(10, 3) == [(2, 0, 3), (1, 3, 6), (0, 6, 10)]
    a = rng.standard_normal((6, 8, 3)).astype(np.float32)
    assert np.array_equal(VR.box_mean(a)[1, 2], ((a[2, 4] + a[2, 5]) + (a[3, 4] + a[3, 5])) * np.float32(0.25))


def good_params():
    from spz_amd import abi
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    return abi.render_params(m, 100.0, 100.0, 50.0, 40.0, 100, 80)


def test_signatures_resolve_and_defaults():
    from spz_amd import abi
    L = abi.load_library()
    for name, restype, nargs in (("spz_amd_render_records_backward_device", C.c_int, 8),
                                 ("spz_amd_render_view_backward_workspace_bytes", C.c_uint64, 1),
                                 ("spz_amd_render_view_backward_device", C.c_int, 12),
                                 ("spz_amd_locate_default_options", C.c_int, 1),
                                 ("spz_amd_locate_check", C.c_int, 1),
                                 ("spz_amd_locate_level_params", C.c_int, 3),
                                 ("spz_amd_locate_twist_gradient", C.c_int, 3),
                                 ("spz_amd_locate_pose_step", C.c_int, 6),
                                 ("spz_amd_image_halve_device", C.c_int, 6),
                                 ("spz_amd_locate_host", C.c_int, 14),
                                 ("spz_amd_locate_cloud_host", C.c_int, 15)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is restype and len(f.argtypes) == nargs, name
    small, big = (int(L.spz_amd_render_view_backward_workspace_bytes(n)) for n in (0, 10 ** 7))
    assert small > 0 and big - small >= (10 ** 7 // 256) * 12 * 8
    o = abi.locate_options()
    assert (o.iterations, o.levels, o.lambda_dssim, o.lr_rotation, o.lr_translation, o.lr_final_factor, o.beta1, o.beta2,
            o.eps) == (300, 1, 0.2, 2e-3, 2e-3, 0.1, 0.9, 0.999, 1e-15)
    assert {k: getattr(o, k) for k in abi.LOCATE_FIELDS} == VR.DEFAULTS
    for bad in (dict(iterations=-1), dict(levels=0), dict(levels=9), dict(lambda_dssim=1.5), dict(lambda_dssim=-0.1),
                dict(lr_rotation=-1.0), dict(lr_translation=float("nan")), dict(lr_final_factor=0.0),
                dict(lr_final_factor=1.5), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(iterations=1.5),
                dict(speed=3)):
        with pytest.raises(ValueError):
            abi.locate_options(**bad)
    assert L.spz_amd_locate_check(None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_locate_default_options(None) == abi.ERR_INVALID_ARG


def test_bad_arguments_are_refused_and_no_device_is_an_error():
    """Every refusal comes before the first HIP call, so it is the same with and without a device; the pointers that
    are not NULL are never dereferenced.  With every argument in order and no device the answer is ERR_NO_DEVICE."""
    from spz_amd import abi
    L = abi.load_library()
    p = good_params()
    some = C.c_void_p(4096)
    cl = abi.CloudPtrs(*([4096] * 6))
    no_sh = abi.CloudPtrs(*([4096] * 5), None)
    have_gpu = torch.cuda.is_available()

    def records(n=10, params=p, m=100, grad=some, rec=some, status=some, rws=some):
        return L.spz_amd_render_records_backward_device(n, C.byref(params) if params is not None else None, m, grad, rec,
                                                        status, rws, None)

    for kw in (dict(params=None), dict(grad=None), dict(rec=None), dict(status=None), dict(rws=None), dict(m=2 ** 31)):
        assert records(**kw) == abi.ERR_INVALID_ARG, kw
    assert records(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS

    def view(cloud=cl, n=10, deg=1, aa=0, params=p, m=100, rec=some, out=some, status=some, rws=some, ws=some):
        return L.spz_amd_render_view_backward_device(C.byref(cloud) if cloud is not None else None, n, deg, aa,
                                                     C.byref(params) if params is not None else None, m, rec, out,
                                                     status, rws, ws, None)

    for kw in (dict(cloud=None), dict(params=None), dict(rec=None), dict(out=None), dict(status=None), dict(rws=None),
               dict(ws=None), dict(deg=4), dict(deg=-1), dict(cloud=no_sh), dict(m=2 ** 31), dict(out=C.c_void_p(4100))):
        assert view(**kw) == abi.ERR_INVALID_ARG, kw
    assert view(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    for kw in (dict(fx=0.0), dict(width=0), dict(near_plane=0.0), dict(max_sh_degree=4), dict(coord=9)):
        q = good_params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert view(params=q) == abi.ERR_INVALID_ARG, kw
        assert records(params=q) == abi.ERR_INVALID_ARG, kw

    assert L.spz_amd_image_halve_device(some, 3, 41, 36, some, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_halve_device(some, 2, 40, 36, some, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_halve_device(None, 3, 40, 36, some, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_image_halve_device(some, 3, 40, 36, None, None) == abi.ERR_INVALID_ARG

    hdr = abi.Header(3, 10, 1, 12, 0, 0)
    size = abi.stream_layout(10, 1, 3).total_bytes
    pose = (C.c_float * 12)()
    hist = (C.c_double * 300)()

    def locate(stream=some, size=size, hdr=hdr, params=p, target=some, ch=3, out=pose, history=hist, **fields):
        o = abi.LocateOptions()
        assert L.spz_amd_locate_default_options(C.byref(o)) == abi.OK
        for k, v in fields.items():
            setattr(o, k, v)
        return L.spz_amd_locate_host(stream, size, C.byref(hdr) if hdr is not None else None,
                                     C.byref(params) if params is not None else None, target, ch, C.byref(o), 0, out,
                                     history, None, None, None, None)

    for kw in (dict(stream=None), dict(hdr=None), dict(params=None), dict(target=None), dict(out=None), dict(history=None),
               dict(ch=2), dict(ch=5), dict(iterations=-1), dict(levels=0), dict(levels=9), dict(lambda_dssim=2.0),
               dict(lr_rotation=-1.0), dict(lr_final_factor=0.0), dict(beta1=1.0),
               dict(levels=4)):  # 100 x 80 is not divisible by 8
        assert locate(**kw) == abi.ERR_INVALID_ARG, kw
    assert locate(size=size - 1) == abi.ERR_SHORT_STREAM
    assert locate(hdr=abi.Header(4, 10, 1, 12, 0, 0)) == abi.ERR_VERSION

    def locate_cloud(cloud=cl, n=10, deg=1, **fields):
        o = abi.locate_options(**fields)
        return L.spz_amd_locate_cloud_host(C.byref(cloud) if cloud is not None else None, n, deg, 0, C.byref(p), some, 4,
                                           C.byref(o), 0, pose, hist, None, None, None, None)

    for kw in (dict(cloud=None), dict(cloud=no_sh), dict(deg=4)):
        assert locate_cloud(**kw) == abi.ERR_INVALID_ARG, kw
    assert locate_cloud(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    if not have_gpu:
        assert records() == abi.ERR_NO_DEVICE
        assert view() == abi.ERR_NO_DEVICE
        assert view(deg=0, cloud=no_sh) == abi.ERR_NO_DEVICE
        assert L.spz_amd_image_halve_device(some, 4, 40, 36, some, None) == abi.ERR_NO_DEVICE
        assert locate() == abi.ERR_NO_DEVICE
        assert locate(levels=3, iterations=0, history=None) == abi.ERR_NO_DEVICE  # 100 x 80 is divisible by 4
        assert locate_cloud() == abi.ERR_NO_DEVICE


def test_python_forms_refuse_host_tensors_and_bad_arguments():
    from spz_amd import device as D
    c = GR.scene(1, 1, n=8)
    cloud = {k: torch.as_tensor(v) for k, v in c.items()}
    p = good_params()
    g = torch.zeros((p.height, p.width, 4))
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.render_view_backward(cloud, 8, 1, p, g)
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.locate(cloud, 8, 1, p, g)
    with pytest.raises(ValueError):
        D.render_view_backward(cloud, 8, 4, p, g)
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.image_halve(g)
    with pytest.raises(ValueError, match=r"shape \(3, 4\)"):
        D.render_autograd(cloud, 8, 1, p, world_to_camera=torch.zeros(4, 4))


def write_pfm(path, rgb, little=True, comment=False):
    """A colour PFM as spz_render writes it (little-endian, scale -1.0, rows bottom to top), or big-endian."""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n" + (b"# a comment\n" if comment else b"") + f"{w} {h}\n".encode()
                + (b"-1.0\n" if little else b"1.0\n"))
        f.write(rgb[::-1].astype("<f4" if little else ">f4").tobytes())


def write_ppm(path, rgb):
    """A binary PPM as spz_render writes it: clamp to [0, 1], round(255 v), rows top to bottom."""
    h, w, _ = rgb.shape
    v = np.where(np.isnan(rgb), np.float32(0.0), np.clip(rgb, 0.0, 1.0)).astype(np.float32)
    with open(path, "wb") as f:
        f.write(f"P6\n{w} {h}\n255\n".encode())
        f.write(np.floor(np.float32(255.0) * v + np.float32(0.5)).astype(np.uint8).tobytes())


def test_image_reader_round_trips_what_spz_render_writes(tmp_path):
    """spz.load_image (spz::loadImageFile) on files in spz_render's two spellings (test_gpu_locate reads the files the
    tool itself wrote): the PFM carries the floats' bits, either byte order; the PPM gives k / 255."""
    import spz_amd.spz as spz
    rng = np.random.default_rng(3)
    img = (rng.standard_normal((5, 7, 3)) * 0.6 + 0.5).astype(np.float32)
    img[0, 0] = (-0.0, 1e-30, 3.5)
    for little in (True, False):
        path = str(tmp_path / f"a{int(little)}.pfm")
        write_pfm(path, img, little, comment=not little)
        got = spz.load_image(path)
        assert got.shape == (5, 7, 3) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), img.view(np.uint32))
    path = str(tmp_path / "a.ppm")
    write_ppm(path, img)
    got = spz.load_image(path)
    want = np.floor(np.float32(255.0) * np.clip(img, 0.0, 1.0) + np.float32(0.5)) / np.float32(255.0)
    assert np.array_equal(got, want.astype(np.float32))
    for name, data in (("short.pfm", b"PF\n7 5\n-1.0\n" + b"\0" * 10), ("grey.pfm", b"Pf\n7 5\n-1.0\n" + b"\0" * 140),
                       ("deep.ppm", b"P6\n7 5\n65535\n" + b"\0" * 210), ("wide.ppm", b"P6\n0 5\n255\n"),
                       ("text.ppm", b"P3\n1 1\n255\n0 0 0\n")):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ValueError, match=name):
            spz.load_image(str(p))
    with pytest.raises(ValueError, match="unable to open"):
        spz.load_image(str(tmp_path / "missing.pfm"))


def test_locate_spz_and_the_tool_refuse_bad_arguments(tmp_path, capfd):
    """Every refusal of spz.locate_spz is a ValueError before any device work; spz::locateSpz prints one [SPZ ERROR]
    line; spz_locate prints its usage line or names what does not fit."""
    import os
    import subprocess
    import spz_amd.spz as spz
    from conftest import ROOT
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    view = {"world_to_camera": m, "fx": 30.0, "fy": 30.0, "cx": 20.0, "cy": 18.0, "width": 40, "height": 36}
    image = np.zeros((36, 40, 3), np.float32)
    missing = str(tmp_path / "missing.spz")
    for kw in (dict(iterations=-1), dict(levels=0), dict(levels=9), dict(levels=4), dict(lambda_dssim=1.5),
               dict(lr_rotation=-1.0), dict(lr_translation=float("inf")), dict(lr_final_factor=0.0), dict(beta1=1.0),
               dict(eps=-1.0), dict(near=0.0), dict(max_sh_degree=4), dict(background=(0.0, 1.0))):
        with pytest.raises(ValueError):
            spz.locate_spz(missing, view, image, **kw)
    for bad in (np.zeros((36, 40, 2), np.float32), np.zeros((36, 41, 3), np.float32), np.zeros((36, 40, 3), np.float64),
                [[0.0]]):
        with pytest.raises(ValueError, match="image"):
            spz.locate_spz(missing, view, bad)
    with pytest.raises(ValueError, match="view 0"):
        spz.locate_spz(missing, dict(view, fx=0.0), image)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        spz.locate_spz(missing, view, image)  # the arguments are in order; the file is not there
    said = capfd.readouterr()
    assert "[SPZ ERROR]" in said.out + said.err
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_locate")
    views_file = tmp_path / "views.txt"
    views_file.write_text("40 36 30 30 20 18 " + " ".join(repr(float(x)) for x in np.asarray(m).reshape(-1)) + "\n")
    pfm = str(tmp_path / "a.pfm")
    write_pfm(pfm, image)
    for args in ([], [missing], [missing, "--views", str(views_file)], [missing, "--images", pfm],
                 [missing, "--views", str(views_file), "--images", pfm, "--levels", "9"],
                 [missing, "--views", str(views_file), "--images", pfm, "--lambda", "2"],
                 [missing, "--views", str(views_file), "--images", pfm, "--iterations", "-3"],
                 [missing, "--views", str(views_file), "--images", pfm, "--speed", "3"]):
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr.startswith("Usage: spz_locate"), args
    r = subprocess.run([tool, missing, "--views", str(views_file), "--images", pfm, pfm], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "1 views but 2 images" in r.stderr
    small = str(tmp_path / "small.pfm")
    write_pfm(small, image[:, :38])
    r = subprocess.run([tool, missing, "--views", str(views_file), "--images", small], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "40 x 36" in r.stderr and "38 x 36" in r.stderr
    r = subprocess.run([tool, missing, "--views", str(views_file), "--images", pfm], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "[SPZ ERROR]" in r.stdout + r.stderr
    assert subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True,
                          text=True).stderr.strip().endswith("spz_locate} <args...>")
