"""spz_amd_render_backward_device / spz_amd.device.render_backward + render_autograd (include/spz_amd.h "render
backward"; DESIGN §8 "Render backward") on the GPU, against autograd of the float64 restatement in
tests/render_grad_ref.py.

The scene: 300 Gaussians of a few pixels each in a 40 x 36 view (3 x 3 tiles, the right and bottom ones partial), all
visible, about 1,000 tile entries, about 21,000 used pairs, 190-290 pixels that reach the stop, 80-105 colour channels
clamped at 0.  Each case's seed was chosen on the CPU so that the reference counts no marginal pair (a pair within a
relative 1e-4 of a decision threshold, which an f32 blend might decide the other way), and asserts it.

Tolerance: for each of the six arrays and for the record gradients, |device - ref64| <= 8 max|ref32 - ref64| over the
array, ref32 being the same reference in float32 with the same decisions.  8: the device sums a Gaussian's up to 1,440
pixel terms in f32 in arbitrary atomic order where torch sums pairwise, and its per-Gaussian chain runs in f64 where
ref32's runs in f32.  An array whose ref32 error is 0 must match exactly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import render_grad_ref as GR
import render_ref as RR
from test_gpu_render import view_of

pytestmark = pytest.mark.gpu

W, H = 40, 36
BG = (0.1, 0.2, 0.3)
ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")
# name: seed, degree, antialiased, max_sh_degree, clamp hits
CASES = {"sh3": (1, 3, False, 3, 4), "sh3_aa": (6, 3, True, 3, 0), "sh1_max0": (5, 1, False, 0, 0),
         "sh0": (6, 0, False, 3, 0)}


def view(cloud, max_sh):
    from spz_amd import abi
    m, fx, fy, cx, cy = view_of(cloud["positions"], width=W, height=H)
    return (abi.render_params(m, fx, fy, cx, cy, W, H, 0.2, BG, max_sh, 0),
            RR.camera(m, fx, fy, cx, cy, W, H, 0.2, BG, max_sh))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's scene, view and image gradient, and the reference's gradients in float64 and float32: computed once
    and shared (nothing changes them)."""
    seed, deg, aa, max_sh, hits = CASES[name]
    cloud = GR.scene(seed, deg, clamp_hits=hits)
    params, cam = view(cloud, max_sh)
    dec = GR.decisions(cloud, deg, cam, aa)
    assert dec["marginal"] == 0, "choose another seed: the reference counts marginal pairs"
    assert dec["visible"].all() and 900 <= dec["entries"] <= 1100 and 18000 <= dec["used"] <= 26000
    assert 190 <= dec["stopped"] <= 300 and (hits == 0 or dec["clamped"] >= 1)
    G = np.random.default_rng(100 + seed).standard_normal((H, W, 4)).astype(np.float32)
    g64 = GR.gradients(cloud, deg, cam, dec, G, aa, torch.float64)
    g32 = GR.gradients(cloud, deg, cam, dec, G, aa, torch.float32)
    return {"cloud": cloud, "n": cloud["alphas"].size, "deg": deg, "aa": aa, "params": params, "cam": cam, "dec": dec,
            "G": G, "g64": g64, "g32": g32}


def check_gradients(got, ref, what):
    """got: device tensors keyed like the cloud plus "records".  Prints every array's error as a fraction of its bound."""
    for k in ARRAYS + ("records",):
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


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_match_autograd_of_the_reference(cuda, name):
    from spz_amd import device as D
    ref = reference(name)
    cloud = D.to_device(ref["cloud"], cuda)
    got = D.render_backward(cloud, ref["n"], ref["deg"], ref["params"], torch.as_tensor(ref["G"]).to(cuda),
                            antialiased=ref["aa"], return_record_grads=True)
    for k in ARRAYS:
        assert got[k].shape == cloud[k].shape and got[k].dtype == torch.float32
    assert got["records"].shape == (ref["n"], 9)
    check_gradients(got, ref, name)
    if name == "sh1_max0":
        assert not got["sh"].any(), "sh above the used degree gets exactly 0"


@pytest.mark.parametrize("name", ["sh3", "sh3_aa"])
def test_autograd_forward_is_render_and_backward_is_render_backward(cuda, name):
    from spz_amd import device as D
    ref = reference(name)
    n, deg, p, aa = ref["n"], ref["deg"], ref["params"], ref["aa"]
    cloud = D.to_device(ref["cloud"], cuda)
    for k in ("positions", "colors", "sh"):
        cloud[k].requires_grad_(True)
    img = D.render_autograd(cloud, n, deg, p, antialiased=aa)
    plain = D.render({k: v.detach() for k, v in cloud.items()}, n, deg, p, antialiased=aa)
    assert np.array_equal(img.detach().cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
    G = torch.as_tensor(ref["G"]).to(cuda)
    (img * G).sum().backward(retain_graph=True)
    for k in ARRAYS:
        assert (cloud[k].grad is not None) == (k in ("positions", "colors", "sh")), k
    first = {k: cloud[k].grad.clone() for k in ("positions", "colors", "sh")}
    # a second backward through the kept graph reads the same workspace: the gradients add up
    (img * G).sum().backward()
    with pytest.raises(RuntimeError):
        (img * G).sum().backward()  # the graph was freed: torch's usual error
    for k in first:
        want, bound = ref["g64"][k], 8.0 * np.abs(ref["g32"][k] - ref["g64"][k]).max()
        assert np.abs(first[k].cpu().numpy() - want).max() <= bound, k
        assert np.abs(cloud[k].grad.cpu().numpy() - 2.0 * want).max() <= 2.0 * bound, k


def test_an_input_changed_in_place_before_the_backward_raises(cuda):
    from spz_amd import device as D
    ref = reference("sh0")
    cloud = D.to_device(ref["cloud"], cuda)
    cloud["colors"].requires_grad_(True)
    img = D.render_autograd(cloud, ref["n"], ref["deg"], ref["params"])
    with torch.no_grad():
        cloud["colors"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        img.sum().backward()


def descent_losses(render, cloud0, target, lr, steps=5):
    """Plain gradient descent on mean((render(cloud) - target)^2) over colours, alphas and positions from cloud0 (numpy,
    float32): the losses at the start and after each step.  render(cloud) -> (loss, grads) with numpy float32 grads."""
    cloud = {k: v.copy() for k, v in cloud0.items()}
    losses = []
    for _ in range(steps + 1):
        loss, grads = render(cloud, target)
        losses.append(loss)
        if len(losses) > 1 and not losses[-1] < losses[-2]:
            break  # no longer decreasing: the caller needs no more
        for k in ("colors", "alphas", "positions"):
            cloud[k] = (cloud[k] - np.float32(lr) * grads[k].astype(np.float32)).astype(np.float32)
    return losses


def strictly_decreasing(v, steps=5):
    return len(v) == steps + 1 and all(b < a for a, b in zip(v, v[1:]))


def test_five_steps_of_gradient_descent_decrease_the_loss(cuda):
    from spz_amd import device as D
    ref = reference("sh1_max0")
    n, deg, p, cam = ref["n"], ref["deg"], ref["params"], ref["cam"]
    rng = np.random.default_rng(77)
    start = {k: v.copy() for k, v in ref["cloud"].items()}
    start["colors"] = (start["colors"] + 0.3 * rng.standard_normal(start["colors"].size)).astype(np.float32)
    start["alphas"] = (start["alphas"] + 0.5 * rng.standard_normal(start["alphas"].size)).astype(np.float32)
    start["positions"] = (start["positions"] + 0.2 * rng.standard_normal(start["positions"].size)).astype(np.float32)

    def ref_step(cloud, target):
        dec = GR.decisions(cloud, deg, cam)
        t = GR.as_tensors(cloud, torch.float64)
        img, _ = GR.forward(t, deg, cam, dec)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        return float(loss.detach()), {k: t[k].grad.numpy() for k in ("colors", "alphas", "positions")}

    def dev_step(cloud, target):
        t = D.to_device(cloud, cuda)
        for k in ("colors", "alphas", "positions"):
            t[k].requires_grad_(True)
        loss = ((D.render_autograd(t, n, deg, p) - target) ** 2).mean()
        loss.backward()
        return float(loss.detach()), {k: t[k].grad.cpu().numpy() for k in ("colors", "alphas", "positions")}

    ref_target = torch.as_tensor(RR.render(ref["cloud"], deg, cam))
    lr = None
    for e in range(20, -21, -1):  # the largest power of two for which the reference's own run decreases every step
        if strictly_decreasing(descent_losses(ref_step, start, ref_target, 2.0 ** e)):
            lr = 2.0 ** e
            break
    assert lr is not None
    dev_target = D.render(D.to_device(ref["cloud"], cuda), n, deg, p)
    losses = descent_losses(dev_step, start, dev_target, lr)
    print(f"step size {lr}: device losses {losses}")
    assert strictly_decreasing(losses), losses


def test_max_entries_below_the_total(cuda):
    from spz_amd import abi, device as D
    ref = reference("sh0")
    n, deg, p = ref["n"], ref["deg"], ref["params"]
    cloud = D.to_device(ref["cloud"], cuda)
    G = torch.as_tensor(ref["G"]).to(cuda)
    m = ref["dec"]["entries"] - 1
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.render_backward(cloud, n, deg, p, G, max_entries=m)
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.render_autograd({k: v.clone().requires_grad_(True) for k, v in cloud.items()}, n, deg, p, max_entries=m)
    assert D.render_backward(cloud, n, deg, p, G, max_entries=m + 1)["alphas"].abs().max() > 0
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
    gp = abi.CloudPtrs(*[grads[k].data_ptr() if grads[k].numel() else None for k in ARRAYS])
    bws = torch.empty(int(L.spz_amd_render_backward_workspace_bytes(n)), dtype=torch.uint8, device=cuda)
    rc = L.spz_amd_render_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), m, image.data_ptr(), G.data_ptr(),
                                          C.byref(gp), rec.data_ptr(), status[1:].data_ptr(), ws.data_ptr(),
                                          bws.data_ptr(), C.c_void_p(st.cuda_stream))
    assert rc == abi.OK
    torch.cuda.synchronize()
    assert int(total.cpu()[0]) == m + 1 and status.cpu().tolist() == [1, 1]
    for k in ARRAYS:
        assert bool((grads[k] == -7.0).all()), k
    assert bool((rec == -7.0).all()) and bool((image == -7.0).all())


def test_empty_scene_and_everything_behind_the_camera(cuda):
    from spz_amd import abi, device as D
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    p = abi.render_params(m, 50.0, 50.0, 18.5, 10.5, 37, 21, 0.2, BG, 3, 0)
    G = torch.ones((21, 37, 4), device=cuda)
    empty = {k: torch.zeros(0, device=cuda) for k in ARRAYS}
    got = D.render_backward(empty, 0, 2, p, G, return_record_grads=True)
    for k in ARRAYS:
        assert got[k].shape == (0,)
    assert got["records"].shape == (0, 9)
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(50, 2, 3)
    c["positions"].reshape(-1, 3)[:, 2] = -np.abs(c["positions"].reshape(-1, 3)[:, 2]) - 1.0
    cloud = D.to_device(c, cuda)
    got = D.render_backward(cloud, 50, 2, p, G, return_record_grads=True)
    for k in ARRAYS:
        assert got[k].shape == cloud[k].shape and not got[k].any(), k
    assert got["records"].shape == (50, 9) and not got["records"].any()
    t = {k: v.clone().requires_grad_(True) for k, v in cloud.items()}
    D.render_autograd(t, 50, 2, p).sum().backward()
    for k in ARRAYS:
        assert t[k].grad.shape == cloud[k].shape and not t[k].grad.any(), k


def test_side_stream(cuda):
    from spz_amd import device as D
    ref = reference("sh3")
    cloud = D.to_device(ref["cloud"], cuda)
    G = torch.as_tensor(ref["G"]).to(cuda)
    side = torch.cuda.Stream(cuda)
    got = D.render_backward(cloud, ref["n"], ref["deg"], ref["params"], G, antialiased=ref["aa"],
                            return_record_grads=True, stream=side)
    side.synchronize()
    check_gradients(got, ref, "side stream")
