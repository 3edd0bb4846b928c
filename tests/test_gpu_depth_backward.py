"""spz_amd_render_depth_backward_device / spz_amd.device.render_depth_backward + render_depth_autograd (include/spz_amd.h
"render depth backward"; DESIGN §8 "Depth fit") on the GPU, against autograd of the float64 restatement in
tests/depth_grad_ref.py.

The scenes, cameras and seeds are test_gpu_render_grad's (300 Gaussians at 40 x 36, no marginal pair; depth adds no
decision), and so is the tolerance, for the same reason: for each of the six arrays, the n x 9 record gradients and the
n depth gradients, |device - ref64| <= 8 max|ref32 - ref64| over the array, ref32 being the same reference in float32
with the same decisions.  An array whose ref32 error is 0 must match exactly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
import render_grad_ref as GR
import test_gpu_render_grad as TG
from test_gpu_render_grad import ARRAYS, BG, CASES, H, W

pytestmark = pytest.mark.gpu

KEYS = ARRAYS + ("records", "depth")


@functools.lru_cache(maxsize=None)
def reference(name, mode="both"):
    """The case's scene and view (test_gpu_render_grad.reference's), G and G_D, and the reference's gradients in
    float64 and float32.  mode: "both" (G and G_D random) or "depth" (G None)."""
    base = TG.reference(name)
    seed = CASES[name][0]
    assert base["dec"]["marginal"] == 0
    G = base["G"] if mode == "both" else None
    GD = np.random.default_rng(200 + seed).standard_normal((H, W)).astype(np.float32)
    args = (base["cloud"], base["deg"], base["cam"], base["dec"], G, GD, base["aa"])
    ref = dict(base)
    ref.update(G=G, GD=GD, g64=DG.gradients(*args, torch.float64), g32=DG.gradients(*args, torch.float32))
    return ref


def check_gradients(got, ref, what, keys=KEYS):
    """got: device tensors keyed like the cloud plus "records" and "depth".  Prints every array's error as a fraction of
    its bound."""
    for k in keys:
        want = ref["g64"][k]
        bound = 8.0 * np.abs(ref["g32"][k] - want).max() if want.size else 0.0
        g = got[k].detach().cpu().numpy().astype(np.float64).reshape(want.shape)
        err = np.abs(g - want).max() if want.size else 0.0
        print(f"{what} {k}: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {bound:.3e}, "
              f"ratio to max|ref32 - ref64| {8.0 * err / bound if bound else 0.0:.3f}")
        if bound == 0.0:
            assert np.array_equal(g, want), f"{what} {k}: must match exactly"
        else:
            assert err <= bound, f"{what} {k}: {err} above {bound}"


def run(ref, cuda, G, GD, **kw):
    from spz_amd import device as D
    cloud = D.to_device(ref["cloud"], cuda)
    return D.render_depth_backward(cloud, ref["n"], ref["deg"], ref["params"],
                                   torch.as_tensor(G).to(cuda) if G is not None else None,
                                   torch.as_tensor(GD).to(cuda), antialiased=ref["aa"], return_record_grads=True, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_match_autograd_of_the_reference(cuda, name):
    ref = reference(name)
    got = run(ref, cuda, ref["G"], ref["GD"])
    for k in ARRAYS:
        assert got[k].dtype == torch.float32 and got[k].numel() == ref["cloud"][k].size
    assert got["records"].shape == (ref["n"], 9) and got["depth"].shape == (ref["n"],)
    assert np.abs(ref["g64"]["depth"]).max() > 1e-2
    check_gradients(got, ref, name)
    if name == "sh1_max0":
        assert not got["sh"].any(), "sh above the used degree gets exactly 0"


@pytest.mark.parametrize("name", ["sh3", "sh0"])
def test_without_an_image_gradient(cuda, name):
    """G = NULL and G = zeros: colours and sh get exactly 0, the rest is within the rule."""
    ref = reference(name, "depth")
    for what, G in (("G NULL", None), ("G zeros", np.zeros((H, W, 4), np.float32))):
        got = run(ref, cuda, G, ref["GD"])
        assert not got["colors"].any() and not got["sh"].any(), what
        assert not got["records"][:, 6:9].any(), what
        check_gradients(got, ref, f"{name} {what}")


def test_without_a_depth_gradient_it_is_the_render_backward(cuda):
    """G_D = 0: the depth gradients are exactly 0 and the six arrays are within the rule of the colour reference."""
    base = TG.reference("sh3")
    got = run(base, cuda, base["G"], np.zeros((H, W), np.float32))
    assert not got["depth"].any()
    TG.check_gradients(got, base, "G_D zeros")


def test_depth_gradients_sum_to_the_depth_map(cuda):
    """With G_D = 1 and G = NULL, dL/dz_i = sum over pixels of w, so sum_i z_i dL/dz_i = sum_p D_p.  The device sums
    each Gaussian's at most 1,440 pixel terms in f32, each addition off by at most 2^-24 relative of the running sum:
    2^-24 * 1,440 ~ 9e-5 of sum |terms| at worst; the terms are all positive, so sum |terms| is the sum itself."""
    from spz_amd import device as D
    ref = TG.reference("sh0")
    got = run(ref, cuda, None, np.ones((H, W), np.float32))
    cloud = D.to_device(ref["cloud"], cuda)
    depth, rec = D.render_depth(cloud, ref["n"], ref["deg"], ref["params"], return_index=False), \
        D.preprocess(cloud, ref["n"], ref["deg"], ref["params"])
    z = rec["depth"].cpu().numpy().astype(np.float64)
    lhs = float((z * got["depth"].cpu().numpy().astype(np.float64)).sum())
    rhs = float(depth[..., 0].cpu().numpy().astype(np.float64).sum())
    bound = 2.0 ** -24 * 1440 * rhs
    print(f"sum z dL/dz {lhs!r}, sum D {rhs!r}, off by {abs(lhs - rhs) / rhs:.3e} relative, bound {bound / rhs:.3e}")
    assert rhs > 100.0 and abs(lhs - rhs) <= bound


def test_max_entries_below_the_total(cuda):
    from spz_amd import abi, device as D
    ref = reference("sh0")
    n, deg, p = ref["n"], ref["deg"], ref["params"]
    cloud = D.to_device(ref["cloud"], cuda)
    G, GD = torch.as_tensor(ref["G"]).to(cuda), torch.as_tensor(ref["GD"]).to(cuda)
    m = ref["dec"]["entries"] - 1
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.render_depth_backward(cloud, n, deg, p, G, GD, max_entries=m)
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.render_depth_autograd({k: v.clone().requires_grad_(True) for k, v in cloud.items()}, n, deg, p, max_entries=m)
    assert D.render_depth_backward(cloud, n, deg, p, G, GD, max_entries=m + 1)["alphas"].abs().max() > 0
    # the C ABI: status 1, and nothing is written
    L = abi.load_library()
    st = torch.cuda.current_stream(cuda)
    ptrs = D._ptrs(cloud, deg, n, cuda)
    ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, m)), dtype=torch.uint8, device=cuda)
    total = torch.empty(1, dtype=torch.int64, device=cuda)
    status = torch.zeros(2, dtype=torch.int32, device=cuda)
    image = torch.full((H, W, 4), -7.0, device=cuda)
    rc = L.spz_amd_render_prepare_cloud_device(C.byref(ptrs), n, deg, 0, C.byref(p), total.data_ptr(), None,
                                               ws.data_ptr(), C.c_void_p(st.cuda_stream))
    assert rc == abi.OK
    rc = L.spz_amd_render_finish_device(n, C.byref(p), m, image.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                        C.c_void_p(st.cuda_stream))
    assert rc == abi.OK
    grads = {k: torch.full_like(cloud[k], -7.0) for k in ARRAYS}
    rec = torch.full((n, 9), -7.0, device=cuda)
    dz = torch.full((n,), -7.0, device=cuda)
    gp = abi.CloudPtrs(*[grads[k].data_ptr() if grads[k].numel() else None for k in ARRAYS])
    bws = torch.empty(int(L.spz_amd_render_depth_backward_workspace_bytes(n)), dtype=torch.uint8, device=cuda)
    rc = L.spz_amd_render_depth_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), m, G.data_ptr(), GD.data_ptr(),
                                                C.byref(gp), rec.data_ptr(), dz.data_ptr(), status[1:].data_ptr(),
                                                ws.data_ptr(), bws.data_ptr(), C.c_void_p(st.cuda_stream))
    assert rc == abi.OK
    torch.cuda.synchronize()
    assert int(total.cpu()[0]) == m + 1 and status.cpu().tolist() == [1, 1]
    for k in ARRAYS:
        assert bool((grads[k] == -7.0).all()), k
    assert bool((rec == -7.0).all()) and bool((dz == -7.0).all()) and bool((image == -7.0).all())


def test_empty_scene_and_everything_behind_the_camera(cuda):
    from spz_amd import abi, device as D
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    p = abi.render_params(m, 50.0, 50.0, 18.5, 10.5, 37, 21, 0.2, BG, 3, 0)
    G, GD = torch.ones((21, 37, 4), device=cuda), torch.ones((21, 37), device=cuda)
    empty = {k: torch.zeros(0, device=cuda) for k in ARRAYS}
    got = D.render_depth_backward(empty, 0, 2, p, G, GD, return_record_grads=True)
    for k in ARRAYS:
        assert got[k].shape == (0,)
    assert got["records"].shape == (0, 9) and got["depth"].shape == (0,)
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(50, 2, 3)
    c["positions"].reshape(-1, 3)[:, 2] = -np.abs(c["positions"].reshape(-1, 3)[:, 2]) - 1.0
    cloud = D.to_device(c, cuda)
    got = D.render_depth_backward(cloud, 50, 2, p, None, GD, return_record_grads=True)
    for k in ARRAYS:
        assert got[k].shape == cloud[k].shape and not got[k].any(), k
    assert not got["records"].any() and got["depth"].shape == (50,) and not got["depth"].any()
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    img, d0 = D.render_depth_autograd(t, 50, 2, p)
    (img.sum() + d0.sum()).backward()
    for k in ARRAYS:
        assert t[k].grad.shape == cloud[k].shape and not t[k].grad.any(), k


@pytest.mark.parametrize("size", [(17, 16), (1, 1)])
def test_partial_tiles(cuda, size):
    """A 17 x 16 view (a second tile column one pixel wide) and a 1 x 1 view, against the reference of that view."""
    from spz_amd import abi
    import render_ref as RR
    from test_gpu_render import view_of
    w, h = size
    cloud = GR.scene(6, 0, n=60)
    m = view_of(cloud["positions"])[0]
    fx = fy = 14.4  # 0.9 * 16, with the principal point at the view's centre: also the 1 x 1 view sees the crowd
    cx, cy = 0.5 * w, 0.5 * h
    params = abi.render_params(m, fx, fy, cx, cy, w, h, 0.2, BG, 3, 0)
    cam = RR.camera(m, fx, fy, cx, cy, w, h, 0.2, BG, 3)
    dec = GR.decisions(cloud, 0, cam)
    assert dec["marginal"] == 0 and dec["used"] >= 1
    rng = np.random.default_rng(w)
    G = rng.standard_normal((h, w, 4)).astype(np.float32)
    GD = rng.standard_normal((h, w)).astype(np.float32)
    ref = {"cloud": cloud, "n": 60, "deg": 0, "aa": False, "params": params,
           "g64": DG.gradients(cloud, 0, cam, dec, G, GD, False, torch.float64),
           "g32": DG.gradients(cloud, 0, cam, dec, G, GD, False, torch.float32)}
    check_gradients(run(ref, cuda, G, GD), ref, f"{w} x {h}")


def test_side_stream(cuda):
    ref = reference("sh3")
    side = torch.cuda.Stream(cuda)
    got = run(ref, cuda, ref["G"], ref["GD"], stream=side)
    side.synchronize()
    check_gradients(got, ref, "side stream")


def test_the_workspace_of_a_depth_render_serves_as_well(cuda):
    """d_render_workspace as render_depth_device left it: through render_depth_autograd, whose forward is that entry
    (run() above goes through render_finish_device)."""
    from spz_amd import device as D
    ref = reference("sh3_aa")
    cloud = {k: v.requires_grad_(True) for k, v in D.to_device(ref["cloud"], cuda).items()}
    img, d0 = D.render_depth_autograd(cloud, ref["n"], ref["deg"], ref["params"], antialiased=True)
    ((img * torch.as_tensor(ref["G"]).to(cuda)).sum() + (d0 * torch.as_tensor(ref["GD"]).to(cuda)).sum()).backward()
    check_gradients({k: cloud[k].grad for k in ARRAYS}, ref, "after render_depth_device", ARRAYS)


@pytest.mark.parametrize("name", ["sh3", "sh3_aa"])
def test_autograd_forward_is_render_and_render_depth(cuda, name):
    from spz_amd import device as D
    ref = reference(name)
    n, deg, p, aa = ref["n"], ref["deg"], ref["params"], ref["aa"]
    cloud = D.to_device(ref["cloud"], cuda)
    for k in ("positions", "alphas"):
        cloud[k].requires_grad_(True)
    img, d0 = D.render_depth_autograd(cloud, n, deg, p, antialiased=aa)
    plain = {k: v.detach() for k, v in cloud.items()}
    want_img = D.render(plain, n, deg, p, antialiased=aa)
    want_depth = D.render_depth(plain, n, deg, p, antialiased=aa, return_index=False)
    assert img.shape == (H, W, 4) and d0.shape == (H, W)
    assert np.array_equal(img.detach().cpu().numpy().view(np.uint32), want_img.cpu().numpy().view(np.uint32))
    assert np.array_equal(d0.detach().cpu().numpy().view(np.uint32),
                          want_depth[..., 0].contiguous().cpu().numpy().view(np.uint32))
    G, GD = torch.as_tensor(ref["G"]).to(cuda), torch.as_tensor(ref["GD"]).to(cuda)
    ((img * G).sum() + (d0 * GD).sum()).backward()
    for k in ARRAYS:
        assert (cloud[k].grad is not None) == (k in ("positions", "alphas")), k
    check_gradients({k: cloud[k].grad for k in ("positions", "alphas")}, ref, "autograd", ("positions", "alphas"))


def autograd_gradients(ref, cuda, loss):
    """The six arrays' gradients of loss(image, depth0) through render_depth_autograd."""
    from spz_amd import device as D
    cloud = {k: v.requires_grad_(True) for k, v in D.to_device(ref["cloud"], cuda).items()}
    img, d0 = D.render_depth_autograd(cloud, ref["n"], ref["deg"], ref["params"], antialiased=ref["aa"])
    loss(img, d0).backward()
    return {k: cloud[k].grad for k in ARRAYS}


def test_autograd_with_the_image_alone_in_the_loss(cuda):
    """Only the image reaches the loss: the six arrays are within the rule of the colour reference (its bound, 8 max|ref32
    - ref64|; check_gradients here is test_gpu_render_grad's rule over the keys given, autograd returns no records)."""
    base = TG.reference("sh3")
    G = torch.as_tensor(base["G"]).to(cuda)
    got = autograd_gradients(base, cuda, lambda img, d0: (img * G).sum())
    check_gradients(got, base, "image alone", ARRAYS)


def test_autograd_with_the_depth_alone_in_the_loss(cuda):
    """Only depth0 reaches the loss: colours and sh get exactly 0, the rest is within the rule of the depth reference."""
    ref = reference("sh3", "depth")
    GD = torch.as_tensor(ref["GD"]).to(cuda)
    got = autograd_gradients(ref, cuda, lambda img, d0: (d0 * GD).sum())
    assert not got["colors"].any() and not got["sh"].any()
    check_gradients(got, ref, "depth alone", ARRAYS)


def test_an_input_changed_in_place_before_the_backward_raises(cuda):
    from spz_amd import device as D
    ref = reference("sh0")
    cloud = D.to_device(ref["cloud"], cuda)
    cloud["positions"].requires_grad_(True)
    _, d0 = D.render_depth_autograd(cloud, ref["n"], ref["deg"], ref["params"])
    with torch.no_grad():
        cloud["positions"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        d0.sum().backward()


def test_five_steps_of_gradient_descent_decrease_a_depth_loss(cuda):
    """test_gpu_render_grad's five steps, on the positions alone, against mean((D - D_target)^2): the step size is the
    largest power of two for which the reference's own run decreases every step."""
    from spz_amd import device as D
    ref = reference("sh0")
    n, deg, p, cam = ref["n"], ref["deg"], ref["params"], ref["cam"]
    rng = np.random.default_rng(78)
    start = {k: v.copy() for k, v in ref["cloud"].items()}
    start["positions"] = (start["positions"] + 0.2 * rng.standard_normal(start["positions"].size)).astype(np.float32)

    def descent(step, target, lr):
        cloud = {k: v.copy() for k, v in start.items()}
        losses = []
        for _ in range(6):
            loss, g = step(cloud, target)
            losses.append(loss)
            if len(losses) > 1 and not losses[-1] < losses[-2]:
                break
            cloud["positions"] = (cloud["positions"] - np.float32(lr) * g.astype(np.float32)).astype(np.float32)
        return losses

    def ref_step(cloud, target):
        dec = GR.decisions(cloud, deg, cam)
        t = GR.as_tensors(cloud, torch.float64)
        _, Dm, _ = DG.forward(t, deg, cam, dec)
        loss = ((Dm - target) ** 2).mean()
        loss.backward()
        return float(loss.detach()), t["positions"].grad.numpy()

    def dev_step(cloud, target):
        t = D.to_device(cloud, cuda)
        t["positions"].requires_grad_(True)
        _, d0 = D.render_depth_autograd(t, n, deg, p)
        loss = ((d0 - target) ** 2).mean()
        loss.backward()
        return float(loss.detach()), t["positions"].grad.cpu().numpy()

    ref_target = torch.as_tensor(ref["g64"]["D"])
    lr = None
    for e in range(4, -21, -1):
        if TG.strictly_decreasing(descent(ref_step, ref_target, 2.0 ** e)):
            lr = 2.0 ** e
            break
    assert lr is not None
    dev_target = D.render_depth(D.to_device(ref["cloud"], cuda), n, deg, p, return_index=False)[..., 0]
    losses = descent(dev_step, dev_target, lr)
    print(f"step size {lr}: device losses {losses}")
    assert TG.strictly_decreasing(losses), losses
