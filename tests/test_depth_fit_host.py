"""The depth render backward and the depth loss without a GPU (include/spz_amd.h "render depth backward" and "depth
loss"; DESIGN §8 "Depth fit"): tests/depth_grad_ref.py's D against tests/depth_ref.py, its gradients and the depth
loss's against central differences; the new entry points' signatures, argument checks and loud failure without a
device; depth_default_options and depth_check; spz.load_depth; what spz.refine_spz_to_images answers to a bad depth
argument (one thing wrong per row, the whole message); and spz_fit's usage errors for the depth flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
import depth_ref as DR
from conftest import ROOT
import render_grad_ref as GR
import render_ref as RR
from test_render_grad_host import H, W, camera_of, good_params


def test_reference_depth_equals_depth_ref():
    """At float64, with the records rounded to float32 as depth_ref reads them, the torch forward's D is depth_ref's
    accumulated depth and its image render_ref's."""
    c = GR.scene(6, 0)
    cam = camera_of(c)
    dec = GR.decisions(c, 0, cam)
    assert dec["visible"].all() and dec["marginal"] == 0
    with torch.no_grad():
        img, D, _ = DG.forward(GR.as_tensors(c, torch.float64, requires_grad=False), 0, cam, dec)
    maps = DR.render_depth(c, 0, cam)
    assert np.abs(maps["accumulated"]).max() > 1.0
    assert np.abs(D.numpy() - maps["accumulated"]).max() <= 1e-12 * np.abs(maps["accumulated"]).max()
    assert np.abs(img.numpy()[..., 3] - maps["alpha"]).max() <= 1e-12
    assert np.abs(img.numpy() - RR.render(c, 0, cam)).max() <= 1e-12


@pytest.mark.parametrize("aa", [False, True])
def test_gradients_equal_central_differences(aa):
    """test_render_grad_host's scene and reasoning (12 Gaussians, no marginal pairs, float64, records not rounded) for
    L = sum(image * G) + sum(D * G_D): h = 1e-5, bound 1e-6 of the array's largest gradient; over 6 position
    components, 2 alphas and 2 log scales."""
    c = GR.scene(3, 3, n=12)
    c["scales"] = (c["scales"] + 0.8).astype(np.float32)
    c["alphas"] = (c["alphas"] + 2.5).astype(np.float32)
    cam = camera_of(c)
    dec = GR.decisions(c, 3, cam, aa)
    assert dec["marginal"] == 0 and dec["visible"].all() and dec["used"] >= 1500 and dec["stopped"] >= 10
    rng = np.random.default_rng(5)
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    GD = rng.standard_normal((H, W)).astype(np.float32)
    g = DG.gradients(c, 3, cam, dec, G, GD, aa, round_records=False)
    Gt, GDt = torch.as_tensor(G).to(torch.float64), torch.as_tensor(GD).to(torch.float64)
    cloud = GR.as_tensors(c, torch.float64, requires_grad=False)

    def loss():
        with torch.no_grad():
            img, D, _ = DG.forward(cloud, 3, cam, dec, aa, round_records=False)
            return float((img * Gt).sum() + (D * GDt).sum())

    h = 1e-5
    for k, elements in (("positions", (0, 1, 2, 15, 16, 17)), ("alphas", (1, 7)), ("scales", (4, 20))):
        t = cloud[k]
        scale = np.abs(g[k]).max()
        assert scale > 1e-3, k
        for e in elements:
            x = float(t[e])
            t[e] = x + h
            up = loss()
            t[e] = x - h
            down = loss()
            t[e] = x
            err = abs((up - down) / (2 * h) - g[k][e])
            print(f"{k}[{e}]: gradient {g[k][e]:.3e} of at most {scale:.3e}, central difference off by {err:.3e}")
            assert err <= 1e-6 * scale, (k, e, err, scale)
    # the depth term is in it: without G_D the position gradients differ
    g0 = GR.gradients(c, 3, cam, dec, G, aa, round_records=False)
    assert np.abs(g0["positions"] - g["positions"]).max() > 1e-3 * np.abs(g["positions"]).max()


@pytest.mark.parametrize("kind", ["l1", "inverse"])
def test_depth_loss_gradients_equal_central_differences(kind):
    """scale L is piecewise smooth in (D, alpha) with the validity held constant; no |e| of this input is within 1e-3
    of its kink.  h = 1e-6 on values of order 1: bound 1e-6 of the largest gradient."""
    rng = np.random.default_rng(11)
    shape = (5, 7)
    alpha = rng.uniform(0.55, 1.0, shape)
    t = rng.uniform(2.0, 6.0, shape)
    D = alpha * t * rng.choice([0.8, 1.25], shape)
    w = rng.uniform(0.1, 1.0, shape)
    t[0, 0] = np.inf
    alpha[1, 1] = 0.3
    ref = DG.depth_loss(D, alpha, t, w, kind, 0.5, 0.37)
    assert ref["valid"].sum() == 33 and np.abs(ref["e"][ref["valid"]]).min() > 1e-3
    h = 1e-6
    for name, arr, got in (("D", D, ref["g_depth"]), ("alpha", alpha, ref["g_alpha"])):
        num = np.zeros(shape)
        for i in np.ndindex(shape):
            x = arr[i]
            arr[i] = x + h
            up = DG.depth_loss(D, alpha, t, w, kind, 0.5)["L"]
            arr[i] = x - h
            down = DG.depth_loss(D, alpha, t, w, kind, 0.5)["L"]
            arr[i] = x
            num[i] = 0.37 * (up - down) / (2 * h)
        err, scale = np.abs(num - got).max(), np.abs(got).max()
        print(f"{kind} {name}: largest gradient {scale:.3e}, central differences off by {err:.3e}")
        assert scale > 1e-3 and err <= 1e-6 * scale
        assert got[0, 0] == 0.0 and got[1, 1] == 0.0


def test_signatures_resolve():
    from spz_amd import abi
    L = abi.load_library()
    for name, restype, nargs in (("spz_amd_render_depth_backward_workspace_bytes", C.c_uint64, 1),
                                 ("spz_amd_render_depth_backward_device", C.c_int, 15),
                                 ("spz_amd_depth_loss_workspace_bytes", C.c_uint64, 2),
                                 ("spz_amd_depth_loss_device", C.c_int, 14)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is restype and len(f.argtypes) == nargs, name
    small, big = (int(L.spz_amd_render_depth_backward_workspace_bytes(n)) for n in (0, 10 ** 6))
    assert small > 0 and big - small >= 10 ** 6 * 10 * 4
    assert L.spz_amd_depth_loss_workspace_bytes(0, 5) == 0 and L.spz_amd_depth_loss_workspace_bytes(5, 16385) == 0
    assert L.spz_amd_depth_loss_workspace_bytes(45, 70) >= 13 * 16


def test_depth_backward_refuses_bad_arguments_and_no_device_is_an_error():
    """Every refusal comes before the first HIP call; the pointers that are not NULL are never dereferenced."""
    from spz_amd import abi
    L = abi.load_library()
    p = good_params()
    some = C.c_void_p(4096)
    cl = abi.CloudPtrs(*([4096] * 6))
    no_sh = abi.CloudPtrs(*([4096] * 5), None)

    def call(cloud=cl, n=10, deg=1, aa=0, params=p, m=100, grad=None, gdepth=some, grads=cl, rec=None, dz=None,
             status=some, rws=some, bws=some):
        return L.spz_amd_render_depth_backward_device(C.byref(cloud) if cloud is not None else None, n, deg, aa,
                                                      C.byref(params) if params is not None else None, m, grad, gdepth,
                                                      C.byref(grads) if grads is not None else None, rec, dz, status,
                                                      rws, bws, None)

    for kw in (dict(cloud=None), dict(params=None), dict(gdepth=None), dict(grads=None), dict(status=None),
               dict(rws=None), dict(bws=None), dict(deg=4), dict(deg=-1), dict(cloud=no_sh), dict(grads=no_sh),
               dict(m=2 ** 31)):
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    assert call(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert call(n=0, cloud=abi.CloudPtrs(), grads=abi.CloudPtrs(), gdepth=None) == abi.ERR_INVALID_ARG
    for kw in (dict(fx=0.0), dict(width=0), dict(height=16385), dict(near_plane=0.0), dict(max_sh_degree=4)):
        q = good_params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert call(params=q) == abi.ERR_INVALID_ARG, kw
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE  # the image gradient may be NULL
        assert call(deg=0, cloud=no_sh, grads=no_sh, grad=some, rec=some, dz=some) == abi.ERR_NO_DEVICE


def test_depth_loss_refuses_bad_arguments_and_no_device_is_an_error():
    from spz_amd import abi
    L = abi.load_library()
    some, odd = C.c_void_p(4096), C.c_void_p(4098)

    def call(depth=some, image=some, target=some, weight=None, w=40, h=36, kind=0, min_alpha=0.5, scale=1.0, loss=some,
             gdepth=some, gimage=None, ws=some):
        return L.spz_amd_depth_loss_device(depth, image, target, weight, w, h, kind, min_alpha, scale, loss, gdepth,
                                           gimage, ws, None)

    for kw in (dict(depth=None), dict(image=None), dict(target=None), dict(loss=None), dict(gdepth=None), dict(ws=None),
               dict(depth=odd), dict(image=odd), dict(target=odd), dict(weight=odd), dict(gdepth=odd), dict(gimage=odd),
               dict(loss=C.c_void_p(4100)), dict(w=0), dict(h=0), dict(w=16385), dict(kind=2), dict(kind=-1),
               dict(min_alpha=0.0), dict(min_alpha=1.5), dict(min_alpha=float("nan")), dict(scale=-1.0),
               dict(scale=float("inf")), dict(scale=float("nan"))):
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE
        assert call(weight=some, gimage=some, kind=1, min_alpha=1.0, scale=0.0) == abi.ERR_NO_DEVICE


def test_python_forms_refuse_host_tensors_and_bad_arguments():
    from spz_amd import device as D
    c = GR.scene(1, 1, n=8)
    cloud = {k: torch.as_tensor(v) for k, v in c.items()}
    p = good_params()
    g, gd = torch.zeros((p.height, p.width, 4)), torch.zeros((p.height, p.width))
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.render_depth_backward(cloud, 8, 1, p, g, gd)
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.render_depth_autograd({k: v.clone().requires_grad_(True) for k, v in cloud.items()}, 8, 1, p)
    with pytest.raises(ValueError):
        D.render_depth_backward(cloud, 8, 4, p, g, gd)
    with pytest.raises(ValueError, match="image must be a contiguous float32 CUDA tensor"):
        D.depth_loss(torch.zeros((4, 5, 2)), torch.zeros((4, 5, 4)), torch.zeros((4, 5)))


# ---- refine images with depth --------------------------------------------------------------------------------------

def test_depth_options_defaults_and_check():
    from spz_amd import abi
    L = abi.load_library()
    o = abi.DepthOptions(7.0, 7.0, 7)
    assert C.sizeof(abi.DepthOptions) == 16
    assert L.spz_amd_depth_default_options(C.byref(o)) == abi.OK
    assert (o.weight, o.min_alpha, o.kind) == (1.0, 0.5, abi.DEPTH_L1)
    assert L.spz_amd_depth_default_options(None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_depth_check(C.byref(o)) == abi.OK and L.spz_amd_depth_check(None) == abi.ERR_INVALID_ARG
    inf, nan = float("inf"), float("nan")
    for weight, min_alpha, kind, want in ((0.0, 1.0, 1, abi.OK), (5.0, 1e-3, 0, abi.OK), (-1e-9, 0.5, 0, abi.ERR_INVALID_ARG),
                                          (nan, 0.5, 0, abi.ERR_INVALID_ARG), (inf, 0.5, 0, abi.ERR_INVALID_ARG),
                                          (1.0, 0.0, 0, abi.ERR_INVALID_ARG), (1.0, 1.0001, 0, abi.ERR_INVALID_ARG),
                                          (1.0, nan, 0, abi.ERR_INVALID_ARG), (1.0, 0.5, 2, abi.ERR_INVALID_ARG),
                                          (1.0, 0.5, -1, abi.ERR_INVALID_ARG)):
        assert L.spz_amd_depth_check(C.byref(abi.DepthOptions(weight, min_alpha, kind))) == want, (weight, min_alpha, kind)
    z = abi.depth_options(0.25, "inverse", 0.75)
    assert (z.weight, z.min_alpha, z.kind) == (0.25, 0.75, abi.DEPTH_INVERSE_L1)
    for kw in (dict(weight=-1.0), dict(weight=nan), dict(min_alpha=0.0), dict(kind="l2")):
        with pytest.raises(ValueError, match="depth_"):
            abi.depth_options(**kw)


def test_refine_images_depth_checks_its_arguments_before_any_hip_call():
    """tests/test_photo_host.py's table for the two depth entries: pointers that are never followed, and every refusal
    leaves ctx NULL and the byte count 0."""
    from spz_amd import abi
    L = abi.load_library()
    n = 4
    stream = np.zeros(abi.stream_layout(n, 0, 3).total_bytes, np.uint8)
    stream[:16] = np.frombuffer(abi.write_header(3, n, 0), np.uint8)
    hdr = abi.Header(3, n, 0, 12, 0, 0)
    eye = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]], np.float64)
    views = (abi.RenderParams * 2)(*[abi.render_params(eye, 30.0, 30.0, 8.0, 6.0, 16, 12, 0.2, (0.0, 0.0, 0.0), 3, abi.RDF)] * 2)
    p = 0x1000
    good = (C.c_void_p * 2)(p, p)

    def call(entry, targets=good, channels=3, weights=None, depths=good, depth=abi.depth_options(),
             opts=abi.refine_options(2), photo=abi.photo_options(), densify=None, nviews=2, rounds_capacity=0):
        ctx, nbytes, bad = C.c_void_p(7), C.c_uint64(7), C.c_int32(7)
        hist, dhist, derr = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 4)()
        rc = getattr(L, entry)(stream.ctypes.data, stream.size, C.byref(hdr), views, nviews, targets, channels, weights,
                               depths, C.byref(depth) if depth is not None else None, C.byref(opts),
                               C.byref(photo) if photo is not None else None,
                               C.byref(densify) if densify is not None else None, 0, C.byref(ctx), C.byref(nbytes),
                               hist, None, None, None, None, C.byref(bad), None, None, rounds_capacity, None, None, None,
                               dhist, derr)
        assert ctx.value is None and nbytes.value == 0
        return rc, bad.value

    invalid = abi.ERR_INVALID_ARG
    for entry in ("spz_amd_refine_images_depth_open", "spz_amd_refine_images_depth_host_open"):
        assert call(entry, targets=None) == (invalid, -1), entry
        assert call(entry, targets=(C.c_void_p * 2)(p, None)) == (invalid, 1), entry
        assert call(entry, channels=2) == (invalid, -1), entry
        assert call(entry, photo=None) == (invalid, -1), entry
        assert call(entry, depth=None) == (invalid, -1), entry
        assert call(entry, depth=abi.DepthOptions(-1.0, 0.5, 0)) == (invalid, -1), entry
        assert call(entry, depth=abi.DepthOptions(1.0, 0.0, 0)) == (invalid, -1), entry
        assert call(entry, depth=abi.DepthOptions(1.0, 0.5, 2)) == (invalid, -1), entry
        assert call(entry, nviews=0) == (invalid, -1), entry
        assert call(entry, rounds_capacity=-1) == (invalid, -1), entry
    entry = "spz_amd_refine_images_depth_open"
    assert call(entry, depths=(C.c_void_p * 2)(None, p + 2)) == (invalid, 1)   # a map that cannot be read as floats
    assert call(entry, weights=(C.c_void_p * 2)(None, p + 1)) == (invalid, 1)
    if not torch.cuda.is_available():
        assert call(entry)[0] == abi.ERR_NO_DEVICE   # the arguments are in order
        assert call(entry, depths=None)[0] == abi.ERR_NO_DEVICE
        assert call(entry, depths=(C.c_void_p * 2)(None, p))[0] == abi.ERR_NO_DEVICE


def write_pfm(path, pixels, magic, little=True):
    """A PFM with rows bottom to top: magic b"Pf" (pixels (h, w)) or b"PF" ((h, w, 3)), in either byte order."""
    h, w = pixels.shape[:2]
    with open(path, "wb") as f:
        f.write(magic + b"\n" + f"{w} {h}\n".encode() + (b"-1.0\n" if little else b"1.0\n"))
        f.write(pixels[::-1].astype("<f4" if little else ">f4").tobytes())


def test_load_depth(tmp_path):
    import spz_amd.spz as spz
    z = np.array([[1.5, np.inf], [-0.0, 3.25], [np.nan, 7.0]], np.float32)
    for little in (True, False):
        path = str(tmp_path / f"z{int(little)}.pfm")
        write_pfm(path, z, b"Pf", little)
        got = spz.load_depth(path)
        assert got.dtype == np.float32 and got.shape == (3, 2)
        assert np.array_equal(got.view(np.uint32), z.view(np.uint32)), "bit for bit, +inf and -0.0 included"
        with pytest.raises(ValueError, match="neither a binary PPM"):
            spz.load_image(path)   # a picture is never one channel
    rgb = np.stack([z, z + 1.0, z + 2.0], axis=2)
    path = str(tmp_path / "rgb.pfm")
    write_pfm(path, rgb, b"PF")
    assert np.array_equal(spz.load_depth(path).view(np.uint32), z.view(np.uint32)), "the first channel of a colour PFM"
    short, ppm, bad = (str(tmp_path / n) for n in ("short.pfm", "a.ppm", "bad.pfm"))
    with open(str(tmp_path / "z1.pfm"), "rb") as f:
        whole = f.read()
    with open(short, "wb") as f:
        f.write(whole[:-1])
    with open(ppm, "wb") as f:
        f.write(b"P6\n2 3\n255\n" + bytes(18))
    with open(bad, "wb") as f:
        f.write(b"Pf\n0 3\n-1.0\n")
    for path, why in ((short, "short file"), (ppm, "neither a one-channel PFM (Pf) nor a colour PFM (PF)"),
                      (bad, "bad width"), (str(tmp_path / "missing.pfm"), "unable to open")):
        with pytest.raises(ValueError) as e:
            spz.load_depth(path)
        assert str(e.value) == f"loadDepthFile: {path}: {why}"


IN, OUT = "/nonexistent/in.spz", "/nonexistent/out.spz"
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
VIEW = dict(world_to_camera=EYE, fx=1.0, fy=1.0, cx=1.0, cy=1.0, width=2, height=3)
VIEWS = [VIEW, VIEW]
IMG = np.zeros((3, 2, 3), np.float32)
IMGS = [IMG, IMG]
Z = np.ones((3, 2), np.float32)
NAMES = dict(np=np, IN=IN, OUT=OUT, VIEWS=VIEWS, IMGS=IMGS, Z=Z, nan=float("nan"), inf=float("inf"))

ROWS = [
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=Z)", ValueError,
     "depths must be None or a sequence of numpy arrays or None, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths='ab')", ValueError,
     "depths must be None or a sequence of numpy arrays or None, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z])", ValueError,
     "depths must have one entry per view: 2 views, 1 depths"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[None, np.ones((2, 3), np.float32)])", ValueError,
     "depths[1] must be a float32 array of the view's height x width"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[np.ones((3, 2)), None])", ValueError,
     "depths[0] must be a float32 array of the view's height x width"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, [[1.0]]])", ValueError,
     "depths[1] must be a float32 array of the view's height x width"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_weight=-1.0)", ValueError,
     "depth_weight must be finite and >= 0"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_weight=inf)", ValueError,
     "depth_weight must be finite and >= 0"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_kind='l2')", ValueError,
     "depth_kind must be 'l1' or 'inverse'"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_kind=1)", ValueError,
     "depth_kind must be 'l1' or 'inverse'"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_min_alpha=0.0)", ValueError,
     "depth_min_alpha must be in (0, 1]"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, Z], depth_min_alpha=nan)", ValueError,
     "depth_min_alpha must be in (0, 1]"),
    # the checks of the images come first
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMGS[0]], depths=[Z])", ValueError,
     "images must have one array per view: 2 views, 1 images"),
]


@pytest.mark.parametrize("call,kind,message", ROWS, ids=[r[0] for r in ROWS])
def test_refine_spz_to_images_answers_a_bad_depth_argument(call, kind, message):
    import spz_amd.spz as spz
    with pytest.raises(kind) as e:
        eval("spz." + call, {"spz": spz}, NAMES)
    assert str(e.value) == message


def test_refine_spz_to_images_with_good_depth_arguments_reaches_the_file(capfd):
    import spz_amd.spz as spz
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        spz.refine_spz_to_images(IN, OUT, VIEWS, IMGS, depths=[Z, None], depth_weight=0.5, depth_kind="inverse",
                                 depth_min_alpha=1.0, iterations=3)
    said = capfd.readouterr()
    assert "[SPZ ERROR]" in said.out + said.err


def test_spz_fit_depth_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_fit")
    usage = "Usage: spz_fit <in.spz> <out.spz>"
    missing, out = str(tmp_path / "missing.spz"), str(tmp_path / "out.spz")
    views_file = tmp_path / "views.txt"
    line = "2 3 1 1 1 1 " + " ".join(repr(float(x)) for x in EYE.reshape(-1)) + "\n"
    views_file.write_text(line + line)
    pfm, z, small = (str(tmp_path / n) for n in ("a.pfm", "z.pfm", "small.pfm"))
    write_pfm(pfm, IMG, b"PF")
    write_pfm(z, Z, b"Pf")
    write_pfm(small, Z[:2], b"Pf")
    base = [missing, out, "--views", str(views_file), "--images", pfm, pfm]
    for args in (base + ["--depth-weight", "0.5"],                      # the three options without --depths
                 base + ["--depth-kind", "inverse"],
                 base + ["--depth-min-alpha", "0.7"],
                 base + ["--depths", z],                                # 2 views, 1 map
                 base + ["--depths", z, z, "none"],
                 base + ["--depths", z, z, "--depth-weight", "-1"],
                 base + ["--depths", z, z, "--depth-kind", "l2"],
                 base + ["--depths", z, z, "--depth-min-alpha", "0"],
                 base + ["--depths", z, z, "--depth-min-alpha", "1.5"]):
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and usage in r.stderr, (args, r.stderr)
    r = subprocess.run([tool] + base + ["--depths", "none", small], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "view 1 is 2 x 3 but" in r.stderr and "small.pfm is 2 x 2" in r.stderr
    r = subprocess.run([tool] + base + ["--depths", "none", pfm + ".missing"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "loadDepthFile" in r.stderr and "unable to open" in r.stderr
    # the arguments are in order; the input file is not there
    r = subprocess.run([tool] + base + ["--depths", z, "none", "--depth-weight", "0.5", "--depth-kind", "inverse",
                                        "--depth-min-alpha", "0.7", "--iters", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[SPZ ERROR]" in r.stdout + r.stderr and usage not in r.stderr
    listed = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True).stderr
    assert listed.strip().endswith("spz_locate} <args...>")
