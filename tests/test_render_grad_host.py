"""The render backward without a GPU (include/spz_amd.h "render backward"; DESIGN §8 "Render backward"):
tests/render_grad_ref.py's forward against tests/render_ref.py, its gradients against central differences, and the new
entry points' signatures, argument checks and loud failure without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_grad_ref as GR
import render_ref as RR
from test_gpu_render import view_of

W, H = 40, 36
BG = (0.1, 0.2, 0.3)


def camera_of(cloud, max_sh_degree=3):
    m, fx, fy, cx, cy = view_of(cloud["positions"], width=W, height=H)
    return RR.camera(m, fx, fy, cx, cy, W, H, 0.2, BG, max_sh_degree)


@pytest.mark.parametrize("aa", [False, True])
def test_forward_equals_render_ref(aa):
    """At float64 the torch forward is render_ref.render: with the records rounded to float32 as render_ref rounds
    them, and with no rounding against render_ref's blend of the unrounded records (the decisions are those of the
    rounded ones: no pair of this scene is marginal, so they are the unrounded ones' too)."""
    c = GR.scene(1, 3, clamp_hits=4)
    cam = camera_of(c)
    dec = GR.decisions(c, 3, cam, aa)
    assert dec["visible"].all() and 900 <= dec["entries"] <= 1100 and 18000 <= dec["used"] <= 26000
    assert 190 <= dec["stopped"] <= 300
    with torch.no_grad():
        cloud = GR.as_tensors(c, torch.float64, requires_grad=False)
        img, _ = GR.forward(cloud, 3, cam, dec, aa)
        assert np.abs(img.numpy() - RR.render(c, 3, cam, aa)).max() <= 1e-12
        img, rec9 = GR.forward(cloud, 3, cam, dec, aa, round_records=False)
    rec = dict(dec["rec"])
    r = rec9.numpy()
    rec.update(mean=r[:, 0:2], conic=r[:, 2:5], opacity=r[:, 5], rgb=r[:, 6:9])
    if not aa:  # the antialiased scene has marginal pairs, which the unrounded records may decide the other way
        assert dec["marginal"] == 0
        assert np.abs(img.numpy() - RR.render(c, 3, cam, aa, rec=rec)).max() <= 1e-12


@pytest.mark.parametrize("aa", [False, True])
def test_gradients_equal_central_differences(aa):
    """12 Gaussians, degree 3, no marginal pairs, float64, records not rounded (rounding makes the forward piecewise
    constant).  L = sum(image * G).  With h = 1e-5 a central difference is off by about eps |L| / h ~ 1e-10 from
    rounding and h^2 |L'''| / 6 from truncation, ~1e-7 |L'| for the third derivatives of this forward: the bound is
    1e-6 of the array's largest gradient."""
    c = GR.scene(3, 3, n=12)
    c["scales"] = (c["scales"] + 0.8).astype(np.float32)  # 12 Gaussians must still overlap,
    c["alphas"] = (c["alphas"] + 2.5).astype(np.float32)  # stop some pixels and clamp some alphas
    cam = camera_of(c)
    dec = GR.decisions(c, 3, cam, aa)
    assert dec["marginal"] == 0 and dec["visible"].all() and dec["used"] >= 1500 and dec["stopped"] >= 10
    assert aa or dec["clamped"] >= 1
    G = np.random.default_rng(5).standard_normal((H, W, 4)).astype(np.float32)
    g = GR.gradients(c, 3, cam, dec, G, aa, round_records=False)
    Gt = torch.as_tensor(G).to(torch.float64)
    cloud = GR.as_tensors(c, torch.float64, requires_grad=False)

    def loss():
        with torch.no_grad():
            return float((GR.forward(cloud, 3, cam, dec, aa, round_records=False)[0] * Gt).sum())

    h = 1e-5
    for k in ("positions", "scales", "rotations", "alphas", "colors", "sh"):
        t = cloud[k]
        num = np.zeros(t.numel())
        for e in range(t.numel()):
            x = float(t[e])
            t[e] = x + h
            up = loss()
            t[e] = x - h
            down = loss()
            t[e] = x
            num[e] = (up - down) / (2 * h)
        scale = np.abs(g[k]).max()
        assert scale > 1e-3, k
        err = np.abs(num - g[k]).max()
        print(f"{k}: largest gradient {scale:.3e}, central differences off by {err:.3e}")
        assert err <= 1e-6 * scale, (k, err, scale)


def good_params():
    from spz_amd import abi
    m = RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0])
    return abi.render_params(m, 100.0, 100.0, 50.0, 40.0, 100, 80)


def test_signatures_resolve():
    from spz_amd import abi
    L = abi.load_library()
    for name, restype, nargs in (("spz_amd_render_backward_workspace_bytes", C.c_uint64, 1),
                                 ("spz_amd_render_backward_device", C.c_int, 14)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is restype and len(f.argtypes) == nargs, name
    small, big = (int(L.spz_amd_render_backward_workspace_bytes(n)) for n in (0, 10 ** 6))
    assert small > 0 and big - small >= 10 ** 6 * 9 * 4


def test_bad_arguments_are_refused_and_no_device_is_an_error():
    """Every refusal comes before the first HIP call, so it is the same with and without a device; the pointers that are
    not NULL are never dereferenced.  With every argument in order and no device the answer is ERR_NO_DEVICE: there is
    no CPU path."""
    from spz_amd import abi
    L = abi.load_library()
    p = good_params()
    some = C.c_void_p(4096)
    cl = abi.CloudPtrs(*([4096] * 6))
    no_sh = abi.CloudPtrs(*([4096] * 5), None)

    def call(cloud=cl, n=10, deg=1, aa=0, params=p, m=100, image=None, grad=some, grads=cl, rec=None, status=some,
             rws=some, bws=some):
        return L.spz_amd_render_backward_device(C.byref(cloud) if cloud is not None else None, n, deg, aa,
                                                C.byref(params) if params is not None else None, m, image, grad,
                                                C.byref(grads) if grads is not None else None, rec, status, rws, bws,
                                                None)

    for kw in (dict(cloud=None), dict(params=None), dict(grad=None), dict(grads=None), dict(status=None), dict(rws=None),
               dict(bws=None), dict(deg=4), dict(deg=-1), dict(cloud=no_sh), dict(grads=no_sh), dict(m=2 ** 31)):
        assert call(**kw) == abi.ERR_INVALID_ARG, kw
    assert call(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert call(n=0, cloud=abi.CloudPtrs(), grads=abi.CloudPtrs(), grad=None) == abi.ERR_INVALID_ARG
    for kw in (dict(fx=0.0), dict(width=0), dict(height=16385), dict(near_plane=0.0), dict(max_sh_degree=4), dict(coord=9)):
        q = good_params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert call(params=q) == abi.ERR_INVALID_ARG, kw
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE
        assert call(deg=0, cloud=no_sh, grads=no_sh, image=some, rec=some) == abi.ERR_NO_DEVICE


def test_python_forms_refuse_host_tensors_and_bad_arguments():
    from spz_amd import device as D
    c = GR.scene(1, 1, n=8)
    n = 8
    cloud = {k: torch.as_tensor(v) for k, v in c.items()}
    p = good_params()
    g = torch.zeros((p.height, p.width, 4))
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.render_backward(cloud, n, 1, p, g)
    with pytest.raises(ValueError, match="CUDA tensor"):
        D.render_autograd({k: v.clone().requires_grad_(True) for k, v in cloud.items()}, n, 1, p)
    with pytest.raises(ValueError):
        D.render_backward(cloud, n, 4, p, g)
