"""Refine without a GPU (DESIGN §8 "Refine"): tests/loss_ref.py against tests/metrics_ref.py and against central
differences, the float32 restatement of the Adam step against torch.optim.Adam, the argument checks of the new C entries
(every refusal comes before the first HIP call), spz.refine_spz's argument checks and spz_refine's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as LR
import metrics_ref as MR
import render_ref as RR
from conftest import ROOT


@pytest.mark.parametrize("h,w,ca,cb,seed", [(5, 7, 3, 4, 1), (13, 17, 4, 3, 2), (23, 12, 4, 4, 3)])
def test_loss_ref_restates_metrics_ref(h, w, ca, cb, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.2, 1.2, (h, w, ca)).astype(np.float32)
    b = rng.uniform(-0.2, 1.2, (h, w, cb)).astype(np.float32)
    a[0, 0, 0], a[1, 2, 1], b[2, 1, 2] = np.nan, np.inf, -np.inf
    want, _ = MR.metrics(a, b)
    for lam in (0.0, 0.2, 1.0):
        got = LR.loss(a, b, lam)
        assert abs(got["l1"] - want["l1"]) <= 1e-12 and abs(got["ssim"] - want["ssim"]) <= 1e-12
        assert abs(got["L"] - ((1.0 - lam) * want["l1"] + lam * (1.0 - want["ssim"]))) <= 1e-12
        assert got["grad"].shape == a.shape
        if ca == 4:
            assert not got["grad"][..., 3].any()
        assert got["grad"][0, 0, 0] == 0.0 and got["grad"][1, 2, 1] == 0.0  # NaN and +inf pass nothing


def test_loss_ref_gradient_equals_central_differences():
    """9 x 8 x 3, float64, values in [0.05, 0.95] with |a - b| >= 0.01, so no element is within h of a kink (the clamp's
    ends, |d| at 0).  With h = 1e-5 a central difference is off by about eps L / h ~ 1e-11 from rounding and by h^2
    L''' / 6 from truncation; the gradients are about 1 / (3 H W) ~ 5e-3: the bound is 1e-6 of the largest."""
    rng = np.random.default_rng(7)
    a = rng.uniform(0.05, 0.95, (9, 8, 3))
    b = np.clip(a + rng.choice([-1.0, 1.0], a.shape) * rng.uniform(0.01, 0.3, a.shape), 0.0, 1.0)
    for lam in (0.0, 0.2, 1.0):
        t = torch.as_tensor(a).clone().requires_grad_(True)
        LR.loss_terms(t, b.astype(np.float32), lam)[0].backward()
        g = t.grad.numpy()
        x = torch.as_tensor(a).clone()
        num = np.zeros(a.size)
        hstep = 1e-5
        flat = x.view(-1)
        with torch.no_grad():
            for e in range(a.size):
                v = float(flat[e])
                flat[e] = v + hstep
                up = float(LR.loss_terms(x, b.astype(np.float32), lam)[0])
                flat[e] = v - hstep
                down = float(LR.loss_terms(x, b.astype(np.float32), lam)[0])
                flat[e] = v
                num[e] = (up - down) / (2 * hstep)
        scale = np.abs(g).max()
        err = np.abs(num.reshape(a.shape) - g).max()
        print(f"lambda {lam}: largest gradient {scale:.3e}, central differences off by {err:.3e}")
        assert scale > 1e-3 and err <= 1e-6 * scale, (lam, err, scale)


def test_clamp_passes_gradient_at_both_ends_and_sign_of_zero_is_zero():
    a = np.full((6, 6, 3), 0.5, np.float32)
    b = np.full((6, 6, 3), 0.25, np.float32)
    a[0, 0, 0], a[0, 1, 0], a[0, 2, 0], a[0, 3, 0] = 0.0, 1.0, -0.01, 1.01
    a[3, 3, 1] = b[3, 3, 1]
    g = LR.loss(a, b, 0.0)["grad"]
    n = a.size
    assert g[0, 0, 0] == -1.0 / n and g[0, 1, 0] == 1.0 / n      # the ends pass
    assert g[0, 2, 0] == 0.0 and g[0, 3, 0] == 0.0                # outside: nothing
    assert g[3, 3, 1] == 0.0                                      # sign(0) = 0
    assert LR.loss(a, b, 1.0)["grad"][0, 0, 0] != 0.0


@pytest.mark.parametrize("t", [1, 2, 100])
def test_f32_adam_step_agrees_with_torch_adam(t):
    """One step from a state torch.optim.Adam reached in float64 after t - 1 steps; the restatement's few float32
    operations are off by a few 2^-24 relative to the step (about lr) and to p: 1e-6 (|p| + lr) per element."""
    rng = np.random.default_rng(10 + t)
    n, lr = 500, 2.5e-3
    p = torch.as_tensor(rng.standard_normal(n)).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-15)
    grads = rng.standard_normal((t, n)) * 10.0 ** rng.uniform(-4, 1, (t, n))
    grads[:, :5] = 0.0
    for k in range(t - 1):
        p.grad = torch.as_tensor(grads[k]).clone()
        opt.step()
    state = opt.state[p] if t > 1 else {"exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}
    p0 = p.detach().numpy().astype(np.float32)
    m0 = state["exp_avg"].numpy().astype(np.float32)
    v0 = state["exp_avg_sq"].numpy().astype(np.float32)
    g = grads[t - 1].astype(np.float32)
    with torch.no_grad():
        p.copy_(torch.as_tensor(p0.astype(np.float64)))
        if t > 1:
            state["exp_avg"].copy_(torch.as_tensor(m0.astype(np.float64)))
            state["exp_avg_sq"].copy_(torch.as_tensor(v0.astype(np.float64)))
    p.grad = torch.as_tensor(g.astype(np.float64))
    opt.step()
    p1, m1, v1, skipped = LR.adam_step(p0, g, m0, v0, t, lr)
    assert skipped == 0 and p1.dtype == np.float32
    want = p.detach().numpy()
    assert (np.abs(p1 - want) <= 1e-6 * (np.abs(want) + lr)).all()
    # the moments: three roundings each, relative to the terms of the sum (which may cancel in m)
    u = 2.0 ** -24
    assert (np.abs(m1 - opt.state[p]["exp_avg"].numpy()) <= 4 * u * (np.abs(m0) + np.abs(g))).all()
    assert (np.abs(v1 - opt.state[p]["exp_avg_sq"].numpy()) <= 4 * u * (np.abs(v0) + g.astype(np.float64) ** 2)).all()


def test_adam_restatement_leaves_non_finite_elements_alone():
    p = np.float32([1.0, np.inf, -np.inf, np.nan, 2.0, 3.0])
    g = np.float32([0.5, 0.5, 0.5, 0.5, np.nan, np.inf])
    m = np.float32([0.1] * 6)
    v = np.float32([0.2] * 6)
    p1, m1, v1, skipped = LR.adam_step(p, g, m, v, 3, 0.1)
    assert skipped == 5
    assert np.array_equal(p1[1:].view(np.uint32), p[1:].view(np.uint32))
    assert np.array_equal(m1[1:], m[1:]) and np.array_equal(v1[1:], v[1:])
    assert p1[0] != p[0] and m1[0] != m[0] and v1[0] != v[0]


# ---- the C entries -------------------------------------------------------------------------------------------------

def test_signatures_resolve():
    from spz_amd import abi
    L = abi.load_library()
    for name, restype, nargs in (("spz_amd_image_loss_workspace_bytes", C.c_uint64, 2),
                                 ("spz_amd_image_loss_device", C.c_int, 11), ("spz_amd_adam_scalars_of", C.c_int, 6),
                                 ("spz_amd_adam_step_device", C.c_int, 10), ("spz_amd_refine_check", C.c_int, 1),
                                 ("spz_amd_refine_default_options", C.c_int, 1), ("spz_amd_refine_open", C.c_int, 18),
                                 ("spz_amd_refine_fetch", C.c_int, 2), ("spz_amd_refine_device_data", C.c_void_p, 1),
                                 ("spz_amd_refine_close", None, 1)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is restype and len(f.argtypes) == nargs, name
    assert L.spz_amd_image_loss_workspace_bytes(0, 5) == 0 and L.spz_amd_image_loss_workspace_bytes(5, 16385) == 0
    assert L.spz_amd_image_loss_workspace_bytes(1920, 1080) >= 72 * 1920 * 1080
    assert C.sizeof(abi.AdamScalars) == 48 and C.sizeof(abi.RefineOptions) == 88


def test_image_loss_refuses_bad_arguments_and_no_device_is_an_error():
    from spz_amd import abi
    L = abi.load_library()
    some = C.c_void_p(4096)

    def call(a=some, ca=4, b=some, cb=3, w=40, h=30, lam=0.2, loss=some, grad=some, ws=some):
        return L.spz_amd_image_loss_device(a, ca, b, cb, w, h, lam, loss, grad, ws, None)

    for kw in (dict(w=0), dict(h=0), dict(w=16385), dict(h=-1), dict(ca=2), dict(ca=5), dict(cb=1), dict(lam=-0.01),
               dict(lam=1.01), dict(lam=float("nan")), dict(a=None), dict(b=None), dict(loss=None), dict(grad=None),
               dict(ws=None), dict(a=C.c_void_p(4098)), dict(loss=C.c_void_p(4100)), dict(grad=C.c_void_p(4097))):
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE
        assert call(lam=0.0, ca=3, cb=4) == abi.ERR_NO_DEVICE


def test_adam_scalars_are_the_f64_values_rounded():
    from spz_amd import abi
    lrs = [1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4]
    for t in (1, 2, 100, 30000):
        sc = abi.adam_scalars(t, lrs)
        want = LR.adam_scalars(t, 1.0)
        for k in ("beta1", "c1", "beta2", "c2", "eps", "r"):
            assert np.float32(getattr(sc, k)) == want[k], (t, k)
        for k, lr in enumerate(lrs):
            assert np.float32(sc.s[k]) == LR.adam_scalars(t, lr)["s"], (t, k)
    for kw in (dict(t=0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(eps=float("nan")),
               dict(lrs=[0, 0, float("inf"), 0, 0, 0]), dict(lrs=[-1.0, 0, 0, 0, 0, 0])):
        args = dict(t=1, lrs=lrs, beta1=0.9, beta2=0.999, eps=1e-15)
        args.update(kw)
        with pytest.raises(abi.SpzAmdError):
            abi.adam_scalars(**args)


def test_adam_step_refuses_bad_arguments_and_no_device_is_an_error():
    from spz_amd import abi
    L = abi.load_library()
    some = C.c_void_p(4096)
    cl = abi.CloudPtrs(*([4096] * 6))
    no_sh = abi.CloudPtrs(*([4096] * 5), None)
    only_colors = abi.CloudPtrs(None, None, None, None, 4096, None)
    odd = abi.CloudPtrs(*([4098] * 6))
    good = abi.adam_scalars(1, [1e-3] * 6)

    def call(p=cl, g=cl, m=cl, v=cl, n=10, deg=1, mask=63, sc=good, skipped=some):
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        return L.spz_amd_adam_step_device(ref(p), ref(g), ref(m), ref(v), n, deg, mask, sc, skipped, None)

    bad_r = abi.AdamScalars.from_buffer_copy(good)
    bad_r.r = 0.0
    bad_s = abi.AdamScalars.from_buffer_copy(good)
    bad_s.s[2] = float("nan")
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(skipped=None), dict(mask=0), dict(mask=64),
               dict(p=no_sh), dict(v=no_sh), dict(g=only_colors), dict(m=odd), dict(sc=bad_r), dict(sc=bad_s),
               dict(skipped=C.c_void_p(4098))):
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    assert call(deg=4) == abi.ERR_SH_DEGREE and call(deg=-1) == abi.ERR_SH_DEGREE
    assert call(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE
        # an array whose bit is clear may be NULL everywhere; sh may be NULL at degree 0
        assert call(p=only_colors, g=only_colors, m=only_colors, v=only_colors, mask=16) == abi.ERR_NO_DEVICE
        assert call(p=no_sh, g=no_sh, m=no_sh, v=no_sh, deg=0) == abi.ERR_NO_DEVICE
        assert call(p=no_sh, g=no_sh, m=no_sh, v=no_sh, deg=2, mask=31) == abi.ERR_NO_DEVICE


def good_view(coord=4):
    from spz_amd import abi
    return abi.render_params(RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), 50, 50, 32, 24, 64, 48, coord=coord)


def test_refine_open_refuses_bad_arguments_and_no_device_is_an_error():
    from spz_amd import abi
    L = abi.load_library()
    h = abi.Header()
    h.num_points, h.sh_degree, h.version, h.fractional_bits = 10, 1, 3, 12
    buf = (C.c_uint8 * 4096)()
    good = good_view()
    history = (C.c_double * 8)()

    def call(views, a=buf, b=buf, ha=h, hb=h, size_a=4096, size_b=4096, hist=history, **kw):
        o = abi.refine_options(kw.pop("iterations", 4), **kw) if "options" not in kw else kw["options"]
        arr = (abi.RenderParams * max(1, len(views)))(*views)
        ctx, nbytes, bad = C.c_void_p(), C.c_uint64(), C.c_int32(7)
        rc = L.spz_amd_refine_open(a, size_a, C.byref(ha) if ha is not None else None, b, size_b,
                                   C.byref(hb) if hb is not None else None, arr, len(views),
                                   C.byref(o) if o is not None else None, 0, C.byref(ctx), C.byref(nbytes), hist, None,
                                   None, None, None, C.byref(bad))
        assert not ctx.value and nbytes.value == 0
        return rc, bad.value

    assert call([]) == (abi.ERR_INVALID_ARG, -1)
    assert call([good] * 1025) == (abi.ERR_INVALID_ARG, -1)
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.fx = -1.0
    assert call([good, good, worse]) == (abi.ERR_INVALID_ARG, 2)
    assert call([worse, good, good]) == (abi.ERR_INVALID_ARG, 0)
    assert call([good, good_view(coord=6)]) == (abi.ERR_INVALID_ARG, 1)      # mixed coords
    # the options before the views, the views before the streams
    assert call([worse, good], options=None) == (abi.ERR_INVALID_ARG, -1)
    assert call([], options=None) == (abi.ERR_INVALID_ARG, -1)
    assert call([good, good, worse], a=None, b=None, ha=None, hb=None) == (abi.ERR_INVALID_ARG, 2)
    big = abi.Header.from_buffer_copy(h)
    big.num_points = 0x80000000
    assert call([good, good_view(coord=6)], ha=big) == (abi.ERR_INVALID_ARG, 1)
    assert call([good], ha=big)[0] == abi.ERR_SHORT_STREAM                   # here the stream's length comes first,
    assert call([good], hb=big)[0] == abi.ERR_SHORT_STREAM
    assert call([good], hb=big, size_b=2 ** 36)[0] == abi.ERR_TOO_MANY_POINTS  # then the point count (B never read)
    assert call([good], options=None) == (abi.ERR_INVALID_ARG, -1)
    assert call([good], a=None)[0] == abi.ERR_INVALID_ARG
    assert call([good], b=None)[0] == abi.ERR_INVALID_ARG
    assert call([good], ha=None)[0] == abi.ERR_INVALID_ARG
    assert call([good], hist=None)[0] == abi.ERR_INVALID_ARG                 # iterations > 0 need a history
    assert call([good], size_a=100)[0] == abi.ERR_SHORT_STREAM
    for field, value in (("iterations", -1), ("train_mask", 0), ("train_mask", 64), ("lambda_dssim", -0.1),
                         ("lambda_dssim", 1.5), ("lambda_dssim", float("nan")), ("beta1", 1.0), ("beta2", -0.5),
                         ("eps", -1.0)):
        o = abi.refine_options(4)
        setattr(o, field, value)
        assert L.spz_amd_refine_check(C.byref(o)) == abi.ERR_INVALID_ARG, (field, value)
        assert call([good], options=o) == (abi.ERR_INVALID_ARG, -1), (field, value)
    o = abi.refine_options(4)
    o.lr[3] = float("inf")
    assert call([good], options=o) == (abi.ERR_INVALID_ARG, -1)
    v1 = abi.Header.from_buffer_copy(h)
    v1.version = 1
    assert call([good], ha=v1)[0] == abi.ERR_UNSUPPORTED                     # the encoder writes versions 2 and 3
    f10 = abi.Header.from_buffer_copy(h)
    f10.fractional_bits = 10
    assert call([good], ha=f10)[0] == abi.ERR_UNSUPPORTED                    # and positions at 12 bits,
    if not torch.cuda.is_available():
        assert call([good], ha=f10, train=("colors",))[0] == abi.ERR_NO_DEVICE  # which matters when they are trained
        assert call([good, good])[0] == abi.ERR_NO_DEVICE
        assert call([good], iterations=0, hist=None)[0] == abi.ERR_NO_DEVICE


OPEN_ENTRIES = ("spz_amd_refine_open", "spz_amd_refine_densify_open", "spz_amd_refine_images_open",
                "spz_amd_refine_images_depth_open", "spz_amd_refine_images_host_open",
                "spz_amd_refine_images_depth_host_open")


def open_with_one_bad_argument(entry, kind):
    """One call of `entry` with everything in order but `kind`: (status, bad_view, ctx, bytes, num_points, num_rounds),
    every output filled with 7 before the call (the last two None for spz_amd_refine_open, which has neither).  The
    device forms are given addresses that are never followed; the host forms real images, which they may upload."""
    from spz_amd import abi
    L = abi.load_library()
    images, depth_entry, host = "images" in entry, "depth" in entry, "host" in entry
    hdr = abi.Header(1 if kind == "version 1" else 3, 4, 0, 12, 0, 0)
    stream = np.zeros(4096, np.uint8)
    eye = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5]], np.float64)
    good = abi.render_params(eye, 30.0, 30.0, 8.0, 6.0, 16, 12, 0.2, (0.0, 0.0, 0.0), 3, abi.RDF)
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.fx = -1.0
    views = (abi.RenderParams * 3)(good, worse if kind == "bad view" else good, good)
    keep = [np.zeros((12, 16, 3), np.float32), np.zeros((12, 16), np.float32)]   # what a host form would upload
    p, z = (keep[0].ctypes.data, keep[1].ctypes.data) if host else (0x1000, 0x1000)
    targets = (C.c_void_p * 3)(p, None if kind == "NULL target" else p, p)
    weights = (C.c_void_p * 3)(None, 0x1001, None) if kind == "odd weight" else None
    depths = (C.c_void_p * 3)(z, 0x1002 if kind == "odd depth" else z, None)
    opts, photo, depth = abi.refine_options(2), abi.photo_options(), abi.depth_options()
    ctx, nbytes, bad, n_out, n_rounds = C.c_void_p(7), C.c_uint64(7), C.c_int32(7), C.c_uint64(7), C.c_int32(7)
    rounds, hist, dhist, derr = (abi.DensifyRound * 2)(), (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 6)()
    args = [stream.ctypes.data, 50 if kind == "short stream" else stream.size, C.byref(hdr)]
    if not images:
        args += [stream.ctypes.data, stream.size, C.byref(abi.Header(3, 4, 0, 12, 0, 0))]
    args += [views, 0 if kind == "zero views" else 3]
    if images:
        args += [targets, 3, weights]
    if depth_entry:
        args += [depths, None if kind == "NULL depth options" else C.byref(depth)]
    args += [None if kind == "NULL options" else C.byref(opts)]
    if images:
        args += [None if kind == "NULL photo options" else C.byref(photo)]
    if entry != "spz_amd_refine_open":
        args += [None]                                                        # densify: off
    args += [0, C.byref(ctx), C.byref(nbytes), hist, None, None, None, None, C.byref(bad)]
    if entry != "spz_amd_refine_open":
        args += [C.byref(n_out), None if kind == "NULL rounds" else rounds, -1 if kind == "rounds_capacity -1" else 2,
                 C.byref(n_rounds), None]
    if images:
        args += [None]                                                        # exposures
    if depth_entry:
        args += [dhist, derr]
    rc = getattr(L, entry)(*args)
    counted = entry != "spz_amd_refine_open"
    return rc, bad.value, ctx.value, nbytes.value, n_out.value if counted else None, n_rounds.value if counted else None


@pytest.mark.parametrize("entry", OPEN_ENTRIES)
def test_every_open_entry_refuses_one_bad_argument_and_resets_every_output(entry):
    """The six open entries over one table: the status and bad_view of every single bad argument the entry accepts, and
    after each refusal ctx NULL, the byte count 0 and, where the entry reports them, num_points 0 and num_rounds 0.
    A weight or depth map at an odd address is refused by the device forms alone: the host forms copy from theirs.
    Before the entries shared one reset, num_points and num_rounds kept the caller's 7 on the refusals the entries made
    themselves: rounds_capacity -1 and NULL rounds in all five entries that have them, NULL depth options in the two
    depth entries, and every row of the two host forms (which also uploaded the images before they looked at the
    stream's version, so that without a device version 1 was answered with ERR_NO_DEVICE)."""
    from spz_amd import abi
    invalid = abi.ERR_INVALID_ARG
    table = [("NULL options", invalid, -1), ("zero views", invalid, -1), ("bad view", invalid, 1),
             ("short stream", abi.ERR_SHORT_STREAM, -1), ("version 1", abi.ERR_UNSUPPORTED, -1)]
    if entry != "spz_amd_refine_open":
        table += [("rounds_capacity -1", invalid, -1), ("NULL rounds", invalid, -1)]
    if "images" in entry:
        table += [("NULL photo options", invalid, -1), ("NULL target", invalid, 1)]
    if "depth" in entry:
        table += [("NULL depth options", invalid, -1)]
    if "images" in entry and "host" not in entry:
        table += [("odd weight", invalid, 1)]
    if entry == "spz_amd_refine_images_depth_open":
        table += [("odd depth", invalid, 1)]
    for kind, status, view in table:
        rc, bad, ctx, nbytes, num_points, num_rounds = open_with_one_bad_argument(entry, kind)
        assert (rc, bad) == (status, view), kind
        assert ctx is None and nbytes == 0, kind
        if entry != "spz_amd_refine_open":
            assert (num_points, num_rounds) == (0, 0), kind


def test_refine_defaults_are_the_published_arguments():
    from spz_amd import abi
    o = abi.refine_options(0)
    assert o.iterations == 0 and o.train_mask == 63 and o.lambda_dssim == 0.2
    assert list(o.lr) == [1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3, 2.5e-3 / 20]
    assert (o.beta1, o.beta2, o.eps) == (0.9, 0.999, 1e-15)
    assert abi.train_mask(("colors", "sh")) == 48 and abi.train_mask(abi.TRAIN_ARRAYS) == 63
    for bad in ((), ("colour",), 0, 64):
        with pytest.raises(ValueError):
            abi.train_mask(bad)
    with pytest.raises(ValueError):
        abi.refine_options(2.5)


# ---- the layers above ----------------------------------------------------------------------------------------------

def a_view(**kw):
    v = {"world_to_camera": RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), "fx": 50.0, "fy": 50.0, "cx": 32.0,
         "cy": 24.0, "width": 64, "height": 48}
    v.update(kw)
    return v


def test_refine_spz_checks_its_arguments_first(tmp_path):
    import spz_amd.spz as spz
    out = str(tmp_path / "out.spz")
    args = ("missing.spz", "missing_target.spz", out)
    for kw, msg in [(dict(iterations=-1), "iterations"), (dict(lambda_dssim=1.5), "lambda_dssim"),
                    (dict(lambda_dssim=float("nan")), "lambda_dssim"), (dict(beta1=1.0), "beta1"),
                    (dict(eps=-1.0), "eps"), (dict(train=[]), "at least one"), (dict(train=["colour"]), "unknown array"),
                    (dict(train="colors"), "sequence"), (dict(lrs={"colour": 1.0}), "unknown array"),
                    (dict(lrs={"colors": -1.0}), "lrs"), (dict(lrs=[1.0] * 6), "dict"),
                    (dict(max_sh_degree=4), "max_sh_degree"), (dict(near=0.0), "near")]:
        with pytest.raises(ValueError, match=msg):
            spz.refine_spz(*args, [a_view()], **kw)
    with pytest.raises(ValueError, match="1..1024"):
        spz.refine_spz(*args, [])
    with pytest.raises(ValueError, match="view 1: bad camera"):
        spz.refine_spz(*args, [a_view(), a_view(width=0)])
    with pytest.raises(ValueError, match="view 1: its coord differs"):
        spz.refine_spz(*args, [a_view(coord=spz.RDF), a_view(coord=spz.RUB)], coord=spz.RDF)
    with pytest.raises(ValueError, match="both as paths or both as bytes"):
        spz.refine_spz(b"abc", "missing_target.spz", None, [a_view()])
    with pytest.raises(ValueError, match="output must be None"):
        spz.refine_spz(b"abc", b"def", out, [a_view()])
    with pytest.raises(ValueError, match="give the output path"):
        spz.refine_spz("missing.spz", "missing_target.spz", None, [a_view()])
    assert not os.path.exists(out)


def test_cli_usage_errors(tmp_path):
    """spz_refine reads its arguments through the tools' one reader and the view arguments spz_prune and spz_compare
    use: malformed rows exit 1 with the usage line, before any file is opened."""
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_refine")
    views = tmp_path / "v.txt"
    views.write_text("64 48 50 50 32 24 1 0 0 0 0 1 0 0 0 0 1 5\n")
    bad_views = tmp_path / "bad.txt"
    bad_views.write_text("64 48 50 50 32 24 1 0 0\n")
    base = ["in.spz", "target.spz", "out.spz"]
    v = ["--views", str(views)]
    for args in [[], ["in.spz"], ["in.spz", "target.spz"], base, ["in.spz", "target.spz", "--views", str(views)],
                 base + v + ["--iters", "-3"], base + v + ["--iters", "2.5"], base + v + ["--iters"],
                 base + v + ["--lambda-dssim", "1.5"], base + v + ["--lambda-dssim", "nan"],
                 base + v + ["--lr-colors", "-1"], base + v + ["--lr-positions", "inf"], base + v + ["--lr-colours", "1"],
                 base + v + ["--train", "colour"], base + v + ["--train", "colors,"], base + v + ["--train", ""],
                 base + v + ["--iters", "3", "--iters", "4"], base + v + ["--coord", "XYZ"],
                 base + v + ["--orbit", "4"], base + ["--orbit", "4", "--size", "64", "48"],
                 base + ["--orbit", "0", "--size", "64", "48", "--fov-y", "50"],
                 base + ["--orbit", "4", "--size", "64", "48", "--fov-y", "50", "--center", "0", "0", "0"],
                 base + ["--views", str(bad_views)], base + ["--views", str(tmp_path / "none.txt")]]:
        r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "Usage: spz_refine" in r.stderr, (args, r.stderr)
        assert not (tmp_path / "out.spz").exists()
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "spz_refine" in r.stderr
