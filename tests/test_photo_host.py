"""Host-only checks of DESIGN §8 "Fit" (include/spz_amd.h "photo loss" and "refine images"): every new ABI entry
refuses a bad argument before any HIP call, so these pass without a device; photo_default_options and photo_check;
tests/photo_ref.py against loss_ref.py where they must agree; what spz.refine_spz_to_images answers to a bad argument,
as a table in the shape of tests/test_python_arguments.py (one thing wrong per row, the exception's type and its whole
message); and spz_fit's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as LR
import photo_ref as PR
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from spz_amd import abi
    return abi.load_library()


def test_photo_options_defaults_and_check(lib):
    from spz_amd import abi
    o = abi.PhotoOptions(7, 7, 7.0)
    assert lib.spz_amd_photo_default_options(C.byref(o)) == abi.OK
    assert (o.fit_exposure, o.reserved, o.lr_exposure) == (0, 0, 0.01)
    assert lib.spz_amd_photo_default_options(None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_photo_check(C.byref(o)) == abi.OK
    assert lib.spz_amd_photo_check(None) == abi.ERR_INVALID_ARG
    for fit, lr, want in ((1, 0.0, abi.OK), (1, 5.0, abi.OK), (2, 0.01, abi.ERR_INVALID_ARG), (-1, 0.01, abi.ERR_INVALID_ARG),
                          (0, -1e-9, abi.ERR_INVALID_ARG), (0, float("nan"), abi.ERR_INVALID_ARG),
                          (1, float("inf"), abi.ERR_INVALID_ARG)):
        assert lib.spz_amd_photo_check(C.byref(abi.PhotoOptions(fit, 0, lr))) == want, (fit, lr)
    assert abi.photo_options(True, 0.02).fit_exposure == 1 and abi.photo_options(True, 0.02).lr_exposure == 0.02
    assert abi.photo_options().lr_exposure == 0.01
    for lr in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="lr_exposure"):
            abi.photo_options(True, lr)
    with pytest.raises(ValueError):
        abi.exposure_values(np.zeros(11))
    with pytest.raises(ValueError):
        abi.exposure_values(np.full((3, 4), np.inf))
    assert list(abi.exposure_values(PR.IDENTITY)) == list(abi.EXPOSURE_IDENTITY)


def test_photo_loss_and_image_exposure_check_their_arguments_before_any_hip_call(lib):
    """Pointers that are never followed: every call below returns on an argument check."""
    from spz_amd import abi
    assert lib.spz_amd_photo_loss_workspace_bytes(0, 4) == 0 and lib.spz_amd_photo_loss_workspace_bytes(4, 16385) == 0
    w, h = 70, 45
    tiles = 3 * 3
    assert lib.spz_amd_photo_loss_workspace_bytes(w, h) >= 72 * w * h + 32 * tiles + 96 * tiles
    assert lib.spz_amd_photo_loss_workspace_bytes(w, h) > lib.spz_amd_image_loss_workspace_bytes(w, h)
    p = 0x1000   # aligned, not NULL, not memory
    ex, bad_ex = abi.exposure_values(PR.IDENTITY), abi.exposure_values(PR.IDENTITY)
    bad_ex[11] = float("nan")

    def loss(**k):
        return lib.spz_amd_photo_loss_device(k.get("a", p), k.get("ca", 4), k.get("b", p), k.get("cb", 3), k.get("w", None),
                                             k.get("ex", None), k.get("width", 8), k.get("height", 8), k.get("lam", 0.2),
                                             k.get("loss", p), k.get("grad", p), k.get("eg", None), k.get("ws", p), None)

    for k in ({"a": None}, {"b": None}, {"loss": None}, {"grad": None}, {"ws": None}, {"ca": 2}, {"cb": 5}, {"width": 0},
              {"height": 16385}, {"lam": -0.1}, {"lam": 1.1}, {"lam": float("nan")}, {"a": p + 2}, {"b": p + 1}, {"w": p + 3},
              {"loss": p + 4}, {"grad": p + 2}, {"ex": ex}, {"ex": ex, "eg": p + 4}, {"ex": bad_ex, "eg": p}):
        assert loss(**k) == abi.ERR_INVALID_ARG, k

    def apply(**k):
        return lib.spz_amd_image_exposure_device(k.get("src", p), k.get("ch", 4), k.get("ex", ex), k.get("width", 8),
                                                 k.get("height", 8), k.get("dst", p), None)

    for k in ({"src": None}, {"dst": None}, {"ex": None}, {"ex": bad_ex}, {"ch": 2}, {"width": 0}, {"height": -1},
              {"src": p + 1}, {"dst": p + 2}):
        assert apply(**k) == abi.ERR_INVALID_ARG, k
    if not torch.cuda.is_available():
        assert loss() == abi.ERR_NO_DEVICE and apply() == abi.ERR_NO_DEVICE   # the arguments are in order


def test_refine_images_checks_its_arguments_before_any_hip_call(lib):
    from spz_amd import abi
    n = 4
    stream = np.zeros(abi.stream_layout(n, 0, 3).total_bytes, np.uint8)
    stream[:16] = np.frombuffer(abi.write_header(3, n, 0), np.uint8)
    hdr = abi.Header(3, n, 0, 12, 0, 0)
    eye = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]], np.float64)
    views = (abi.RenderParams * 2)(*[abi.render_params(eye, 30.0, 30.0, 8.0, 6.0, 16, 12, 0.2, (0.0, 0.0, 0.0), 3, abi.RDF)] * 2)
    p = 0x1000
    good = (C.c_void_p * 2)(p, p)

    def call(entry, targets=good, channels=3, weights=None, opts=abi.refine_options(2), photo=abi.photo_options(),
             densify=None, nviews=2, rounds_capacity=0):
        ctx, nbytes, bad = C.c_void_p(7), C.c_uint64(7), C.c_int32(7)
        hist = (C.c_double * 2)()
        rc = getattr(lib, entry)(stream.ctypes.data, stream.size, C.byref(hdr), views, nviews, targets, channels, weights,
                                 C.byref(opts), C.byref(photo) if photo is not None else None,
                                 C.byref(densify) if densify is not None else None, 0, C.byref(ctx), C.byref(nbytes),
                                 hist, None, None, None, None, C.byref(bad), None, None, rounds_capacity, None, None, None)
        assert ctx.value is None and nbytes.value == 0
        return rc, bad.value

    invalid = abi.ERR_INVALID_ARG
    on = abi.densify_options({"interval": 1, "max_points": 0})
    for entry in ("spz_amd_refine_images_open", "spz_amd_refine_images_host_open"):
        assert call(entry, targets=None) == (invalid, -1), entry
        assert call(entry, targets=(C.c_void_p * 2)(p, None)) == (invalid, 1), entry
        assert call(entry, channels=2) == (invalid, -1), entry
        assert call(entry, photo=None) == (invalid, -1), entry
        assert call(entry, photo=abi.PhotoOptions(1, 0, -0.5)) == (invalid, -1), entry
        assert call(entry, photo=abi.PhotoOptions(1, 0, float("nan"))) == (invalid, -1), entry
        assert call(entry, nviews=0) == (invalid, -1), entry
        assert call(entry, rounds_capacity=-1) == (invalid, -1), entry
        opts = abi.refine_options(2)
        opts.lambda_dssim = 2.0
        assert call(entry, opts=opts) == (invalid, -1), entry
    # the device form also refuses what it could not read as floats; densify without a count to grow to
    entry = "spz_amd_refine_images_open"
    assert call(entry, targets=(C.c_void_p * 2)(p + 2, p)) == (invalid, 0)
    assert call(entry, weights=(C.c_void_p * 2)(None, p + 1)) == (invalid, 1)
    assert call(entry, densify=on) == (invalid, -1)
    if not torch.cuda.is_available():
        assert call(entry)[0] == abi.ERR_NO_DEVICE   # the arguments are in order


def test_photo_ref_without_weights_and_exposure_is_loss_ref():
    rng = np.random.default_rng(3)
    a = rng.uniform(-0.2, 1.2, (13, 17, 4)).astype(np.float32)
    b = rng.uniform(-0.2, 1.2, (13, 17, 3)).astype(np.float32)
    a[2, 3, 1], a[4, 4, 0], a[5, 5, 2], a[6, 6, 0] = np.nan, np.inf, 0.0, 1.0
    for lam in (0.2, 1.0, 0.0):
        got, want = PR.photo_loss(a, b, lam), LR.loss(a, b, lam)
        assert (got["L"], got["l1"], got["ssim"]) == (want["L"], want["l1"], want["ssim"])
        assert np.array_equal(got["grad"], want["grad"]) and got["exposure_grad"] is None
    # the identity exposure changes nothing where every a is finite, and closes every gate of a pixel where one is not
    # (0 inf = NaN), whose a' is then 0 in all three channels
    fin = np.where(np.isfinite(a), a, 0.5).astype(np.float32)
    got, want = PR.photo_loss(fin, b, 0.2, None, PR.IDENTITY), LR.loss(fin, b, 0.2)
    assert abs(got["L"] - want["L"]) <= 1e-15 and np.allclose(got["grad"], want["grad"], rtol=0, atol=1e-15)
    got = PR.photo_loss(a, b, 0.2, None, PR.IDENTITY)
    finite = np.isfinite(a[..., :3]).all(axis=-1)
    assert (~finite).sum() == 2 and not got["grad"][~finite].any() and np.isfinite(got["exposure_grad"]).all()
    # the exposure's gradient against central differences of L
    ex = PR.IDENTITY + 0.05 * rng.standard_normal((3, 4))
    wt = rng.uniform(0.0, 1.0, (13, 17)).astype(np.float32)
    a = rng.uniform(0.2, 0.8, (13, 17, 3)).astype(np.float32)   # away from the clamp's corners
    g = PR.photo_loss(a, b, 0.2, wt, ex)["exposure_grad"]
    for at in ((0, 0), (1, 2), (2, 3)):
        d = np.zeros((3, 4))
        d[at] = 1e-6
        num = (PR.photo_loss(a, b, 0.2, wt, ex + d)["L"] - PR.photo_loss(a, b, 0.2, wt, ex - d)["L"]) / 2e-6
        assert abs(num - g[at]) <= 1e-6 * max(1.0, abs(g[at])), (at, num, g[at])
    # all-zero weights
    z = PR.photo_loss(a, b, 0.2, np.zeros((13, 17), np.float32), ex)
    assert (z["L"], z["l1"], z["ssim"]) == (0.0, 0.0, 1.0) and not z["grad"].any() and not z["exposure_grad"].any()
    # the two small restatements
    out = PR.apply_exposure_f32(a, PR.IDENTITY)
    assert np.array_equal(out, a)
    e1, m1, v1 = PR.exposure_adam_step(np.ones(12), np.r_[np.full(11, 0.5), np.nan], np.zeros(12), np.zeros(12), 1, 0.01)
    assert np.allclose(e1[:11], 1.0 - 0.01) and e1[11] == 1.0 and m1[11] == 0.0 and v1[11] == 0.0


# ---- spz.refine_spz_to_images: one thing wrong per row -------------------------------------------------------------

IN, OUT = "/nonexistent/in.spz", "/nonexistent/out.spz"
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
VIEW = dict(world_to_camera=EYE, fx=1.0, fy=1.0, cx=1.0, cy=1.0, width=2, height=3)
VIEWS = [VIEW, VIEW]
IMG = np.zeros((3, 2, 3), np.float32)
IMGS = [IMG, IMG]
WT = np.ones((3, 2), np.float32)
NAMES = dict(np=np, IN=IN, OUT=OUT, VIEWS=VIEWS, IMG=IMG, IMGS=IMGS, WT=WT, nan=float("nan"))

ROWS = [
    ("refine_spz_to_images(IN, OUT, VIEWS, 7)", ValueError, "images must be a sequence of numpy arrays, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMG)", ValueError, "images must be a sequence of numpy arrays, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, 'ab')", ValueError, "images must be a sequence of numpy arrays, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMG])", ValueError, "images must have one array per view: 2 views, 1 images"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMG, np.zeros((2, 3, 3), np.float32)])", ValueError,
     "images[1] must be the view's height x width x 3 or 4"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMG, np.zeros((3, 2, 2), np.float32)])", ValueError,
     "images[1] must be the view's height x width x 3 or 4"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [np.zeros((3, 2, 3)), IMG])", ValueError, "images[0] must be float32"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMG, [[0.0]]])", ValueError, "images[1] must be a numpy array"),
    ("refine_spz_to_images(IN, OUT, VIEWS, [IMG, np.zeros((3, 2, 4), np.float32)])", ValueError,
     "images[1] has 4 channels but images[0] has 3"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, weights=WT)", ValueError,
     "weights must be None or a sequence of numpy arrays or None, one per view"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, weights=[WT])", ValueError,
     "weights must have one entry per view: 2 views, 1 weights"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, weights=[None, np.ones((2, 3), np.float32)])", ValueError,
     "weights[1] must be a float32 array of the view's height x width"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, weights=[np.ones((3, 2)), None])", ValueError,
     "weights[0] must be a float32 array of the view's height x width"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, lr_exposure=-1.0)", ValueError, "lr_exposure must be finite and >= 0"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, lr_exposure=nan)", ValueError, "lr_exposure must be finite and >= 0"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, fit_exposure=1)", ValueError, "fit_exposure must be a bool"),
    ("refine_spz_to_images(IN, OUT, VIEWS, IMGS, iterations=-1)", ValueError, "iterations must be >= 0"),
    ("refine_spz_to_images(IN, None, VIEWS, IMGS)", ValueError, "with a path in, give the output path"),
    ("refine_spz_to_images(b'', OUT, VIEWS, IMGS)", ValueError, "with bytes in, output must be None: the bytes are returned"),
]


@pytest.mark.parametrize("call,kind,message", ROWS, ids=[r[0] for r in ROWS])
def test_refine_spz_to_images_answers_a_bad_argument(call, kind, message):
    import spz_amd.spz as spz
    with pytest.raises(kind) as e:
        eval("spz." + call, {"spz": spz}, NAMES)
    assert str(e.value) == message


def test_refine_spz_to_images_with_good_arguments_reaches_the_file(capfd):
    import spz_amd.spz as spz
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        spz.refine_spz_to_images(IN, OUT, VIEWS, IMGS, weights=[WT, None], fit_exposure=True, lr_exposure=0.02, iterations=3)
    said = capfd.readouterr()
    assert "[SPZ ERROR]" in said.out + said.err


# ---- spz_fit -------------------------------------------------------------------------------------------------------

def write_pfm(path, rgb):
    """A colour PFM as spz_render writes it (little-endian, scale -1.0, rows bottom to top)."""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n" + f"{w} {h}\n".encode() + b"-1.0\n")
        f.write(rgb[::-1].astype("<f4").tobytes())


def test_spz_fit_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_fit")
    usage = "Usage: spz_fit <in.spz> <out.spz>"
    missing, out = str(tmp_path / "missing.spz"), str(tmp_path / "out.spz")
    views_file = tmp_path / "views.txt"
    line = "2 3 1 1 1 1 " + " ".join(repr(float(x)) for x in EYE.reshape(-1)) + "\n"
    views_file.write_text(line + line)
    pfm, small = str(tmp_path / "a.pfm"), str(tmp_path / "small.pfm")
    write_pfm(pfm, IMG)
    write_pfm(small, IMG[:2])
    base = [missing, out, "--views", str(views_file)]
    for args in ([], [missing], base,                                              # no --images
                 [missing, out, "--images", pfm, pfm],                             # no --views
                 base + ["--images", pfm],                                         # 2 views, 1 image
                 base + ["--images", pfm, pfm, pfm],
                 base + ["--images", pfm, pfm, "--masks", pfm],                    # 2 images, 1 mask
                 base + ["--images", pfm, pfm, "--lr-exposure", "0.02"],           # without --fit-exposure
                 base + ["--images", pfm, pfm, "--exposures-out", out],
                 base + ["--images", pfm, pfm, "--fit-exposure", "--lr-exposure", "-1"],
                 base + ["--images", pfm, pfm, "--iters", "-3"],
                 base + ["--images", pfm, pfm, "--max-points", "5"],               # densify's, without --densify-interval
                 base + ["--images", pfm, pfm, "--speed", "3"]):
        r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and usage in r.stderr, (args, r.stderr)
    r = subprocess.run([tool] + base + ["--images", pfm, small], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "view 1 is 2 x 3 but" in r.stderr and "is 2 x 2" in r.stderr
    r = subprocess.run([tool] + base + ["--images", pfm, pfm, "--masks", pfm, small], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "view 1 is 2 x 3 but" in r.stderr and "small.pfm is 2 x 2" in r.stderr
    # the arguments are in order; the file is not there
    r = subprocess.run([tool] + base + ["--images", pfm, pfm, "--masks", pfm, pfm, "--fit-exposure", "--iters", "2"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[SPZ ERROR]" in r.stdout + r.stderr and usage not in r.stderr
    listed = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True).stderr
    assert "|spz_fit|" in listed and listed.strip().endswith("spz_locate} <args...>")
