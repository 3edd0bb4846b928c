"""spz_amd_render_view_backward_device, spz_amd_render_records_backward_device and the pose fit on the GPU
(include/spz_amd.h "render view backward" and "locate"; DESIGN §8 "Locate"), against tests/view_grad_ref.py.

The scenes, views and image gradients are those of test_gpu_render_grad.CASES (300 Gaussians, 40 x 36, no marginal pair:
reference() asserts it), shared through its cache.

The fit.  Scene GR.scene(1, 1, n=300), the pose rotated by 3 degrees and the camera moved by 3 % of |t|
(view_grad_ref.perturbed, seed 0), 300 iterations, lr_rotation 2e-3, lr_translation 2e-3 |t|.  view_grad_ref.locate,
the float64 loop on the CPU, reaches from 3.0 degrees / 3.0e-2 of the distance (REFERENCE_FIT below):
    lambda_dssim = 0, 40 x 36, levels = 1:                      below 0.001 degrees / 3.4e-5
    lambda_dssim = 0.2 (default), 40 x 36, levels = 1:          below 0.001 degrees / 2.0e-5
    lambda_dssim = 0.2, 64 x 48, levels = 3, 600 iterations:    below 0.001 degrees / 1.1e-4
    lambda_dssim = 0.2, 64 x 48, levels = 3, 300 iterations:    1.07 degrees / 1.6e-2: not enough
The device must end with the rotation error and the camera-centre error each at most a tenth of their initial values:
a condition, not a tuned tolerance; the slack is for f32 records and atomic sums.
Why the levels case runs 600 iterations: at 64 x 48 the coarsest of three levels is a 16 x 12 image, where the 0.3
pixel dilation of every footprint is no longer the box mean of the fine image's; the reference's pose drifts there (to
2.4 degrees after its 100 iterations) and level 0, which starts at 0.22 of the step size, needs more than 100
iterations to come back.  With 200 per level the reference clears the condition by a factor of 30."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import render_grad_ref as GR
import render_ref as RR
import view_grad_ref as VR
from test_gpu_render import view_of
from test_gpu_render_grad import BG, CASES, H, W, reference

pytestmark = pytest.mark.gpu

# what view_grad_ref.locate reached on the CPU: (rotation error in degrees, centre error / |t|)
REFERENCE_FIT = {"l1": (0.0, 3.39e-5), "default": (0.0, 1.98e-5), "levels3": (0.0, 1.06e-4)}


@functools.lru_cache(maxsize=None)
def view_reference(name):
    """The case's view gradients in float64 and float32 and the bound of test 2: computed once."""
    ref = reference(name)
    args = (ref["cloud"], ref["deg"], ref["cam"], ref["dec"], ref["G"], ref["aa"])
    v64 = VR.view_gradient(*args, torch.float64)
    v32 = VR.view_gradient(*args, torch.float32)
    assert np.abs(v64["records"] - ref["g64"]["records"]).max() == 0.0  # the same forward, the same decisions
    return {"v64": v64["view"], "v32": v32["view"], "bound": 8.0 * np.abs(v32["view"] - v64["view"]).max()}


@pytest.mark.parametrize("name", list(CASES))
def test_chain_and_sum_from_given_record_gradients(cuda, name):
    """The reference's float64 record gradients rounded to f32 go in; both sides run the chain in f64 on those values.
    Per entry the orders of 300 terms differ by at most 300 * 2^-53 of sum |contribution|; 1e-10 leaves the rest for
    exp and sqrt.  The sum uses no atomics: two runs give identical bits."""
    from spz_amd import device as D
    ref = reference(name)
    rg = ref["g64"]["records"].astype(np.float32)
    per = VR.chain(ref["cloud"], ref["deg"], ref["cam"], ref["dec"], rg, ref["aa"])
    want, mag = per.sum(axis=0), np.abs(per).sum(axis=0)
    cloud = D.to_device(ref["cloud"], cuda)
    rg_t = torch.as_tensor(rg).to(cuda)
    got = [D.render_view_backward(cloud, ref["n"], ref["deg"], ref["params"], None, antialiased=ref["aa"],
                                  record_grads=rg_t).cpu().numpy() for _ in range(2)]
    assert got[0].shape == (3, 4) and got[0].dtype == np.float64
    err = np.abs(got[0] - want) / mag
    print(f"{name}: |device - ref| / sum|contribution| at most {err.max():.3e} (bound 1e-10)")
    assert np.all(np.abs(got[0] - want) <= 1e-10 * mag)
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_view_gradient_from_the_image_gradient(cuda, name):
    """|device - ref64| <= 8 max|ref32 - ref64| over the 12 entries: test_gpu_render_grad's rule and factor, for its
    reason (f32 atomic sums under an f64 chain).  The records backward's n x 9 output passes that test's bound."""
    from spz_amd import device as D
    ref, vr = reference(name), view_reference(name)
    cloud = D.to_device(ref["cloud"], cuda)
    got, rec = D.render_view_backward(cloud, ref["n"], ref["deg"], ref["params"], torch.as_tensor(ref["G"]).to(cuda),
                                      antialiased=ref["aa"], return_record_grads=True)
    err = np.abs(got.cpu().numpy() - vr["v64"]).max()
    print(f"{name} view: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {vr['bound']:.3e}, "
          f"ratio to max|ref32 - ref64| {8.0 * err / vr['bound']:.3f}")
    assert vr["bound"] > 0.0 and err <= vr["bound"]
    want = ref["g64"]["records"]
    bound = 8.0 * np.abs(ref["g32"]["records"] - want).max()
    rerr = np.abs(rec.cpu().numpy().astype(np.float64) - want).max()
    print(f"{name} records: |device - ref64| {rerr:.3e}, 8 max|ref32 - ref64| {bound:.3e}")
    assert rec.shape == (ref["n"], 9) and rec.dtype == torch.float32 and rerr <= bound


@pytest.mark.parametrize("name", ["sh3", "sh3_aa"])
def test_translating_the_scene_equals_translating_the_camera(cuda, name):
    """p -> p + d for every Gaussian is t -> t + R d, the view direction included, so R^T G_t is the sum of the
    position gradients of render_backward.  Those are rounded to f32 once each (2^-24 of sum |g_p| per component);
    both runs sum their records with f32 atomics (the bound of the test above)."""
    from spz_amd import device as D
    ref, vr = reference(name), view_reference(name)
    cloud = D.to_device(ref["cloud"], cuda)
    G = torch.as_tensor(ref["G"]).to(cuda)
    view = D.render_view_backward(cloud, ref["n"], ref["deg"], ref["params"], G, antialiased=ref["aa"]).cpu().numpy()
    gp = D.render_backward(cloud, ref["n"], ref["deg"], ref["params"], G, antialiased=ref["aa"])["positions"]
    gp = gp.cpu().numpy().astype(np.float64).reshape(-1, 3)
    lhs = ref["cam"]["R"].T @ view[:, 3]
    bound = 2.0 ** -24 * np.abs(gp).sum(axis=0) + vr["bound"]
    print(f"{name}: |R^T G_t - sum g_p| {np.abs(lhs - gp.sum(axis=0))}, bound {bound}")
    assert np.all(np.abs(lhs - gp.sum(axis=0)) <= bound)


def test_empty_scene_and_everything_behind_the_camera(cuda):
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_numpy
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    p = abi.render_params(m, 50.0, 50.0, 18.5, 10.5, 37, 21, 0.2, BG, 3, 0)
    G = torch.ones((21, 37, 4), device=cuda)
    empty = {k: torch.zeros(0, device=cuda) for k in ("positions", "scales", "rotations", "alphas", "colors", "sh")}
    got, rec = D.render_view_backward(empty, 0, 2, p, G, return_record_grads=True)
    assert got.shape == (3, 4) and not got.any() and rec.shape == (0, 9)
    c = make_cloud_numpy(50, 2, 3)
    c["positions"].reshape(-1, 3)[:, 2] = -np.abs(c["positions"].reshape(-1, 3)[:, 2]) - 1.0
    cloud = D.to_device(c, cuda)
    # through the C ABI, for the status word; the outputs prefilled
    L = abi.load_library()
    st = torch.cuda.current_stream(cuda)
    image, ws, total = D._rendered_workspace(L, ("cloud", D._ptrs(cloud, 2, 50, cuda), 50, 2, False), 50, p, cuda, None, st)
    assert total == 0
    rec = torch.full((50, 9), -7.0, device=cuda)
    out = torch.full((3, 4), -7.0, dtype=torch.float64, device=cuda)
    status = torch.full((2,), 5, dtype=torch.int32, device=cuda)
    vws = torch.empty(int(L.spz_amd_render_view_backward_workspace_bytes(50)), dtype=torch.uint8, device=cuda)
    ptrs = D._ptrs(cloud, 2, 50, cuda)
    assert L.spz_amd_render_records_backward_device(50, C.byref(p), 0, G.data_ptr(), rec.data_ptr(), status.data_ptr(),
                                                    ws.data_ptr(), C.c_void_p(st.cuda_stream)) == abi.OK
    assert L.spz_amd_render_view_backward_device(C.byref(ptrs), 50, 2, 0, C.byref(p), 0, rec.data_ptr(), out.data_ptr(),
                                                 status[1:].data_ptr(), ws.data_ptr(), vws.data_ptr(),
                                                 C.c_void_p(st.cuda_stream)) == abi.OK
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and not rec.any() and not out.any()


def test_max_entries_below_the_total(cuda):
    """Status 1, and neither the record gradients nor the view gradient are written."""
    from spz_amd import abi, device as D
    ref = reference("sh0")
    n, deg, p = ref["n"], ref["deg"], ref["params"]
    cloud = D.to_device(ref["cloud"], cuda)
    G = torch.as_tensor(ref["G"]).to(cuda)
    m = ref["dec"]["entries"] - 1
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.render_view_backward(cloud, n, deg, p, G, max_entries=m)
    assert D.render_view_backward(cloud, n, deg, p, G, max_entries=m + 1).abs().max() > 0
    L = abi.load_library()
    st = torch.cuda.current_stream(cuda)
    ptrs = D._ptrs(cloud, deg, n, cuda)
    ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, m)), dtype=torch.uint8, device=cuda)
    total = torch.empty(1, dtype=torch.int64, device=cuda)
    status = torch.zeros(3, dtype=torch.int32, device=cuda)
    image = torch.full((H, W, 4), -7.0, device=cuda)
    assert L.spz_amd_render_prepare_cloud_device(C.byref(ptrs), n, deg, 0, C.byref(p), total.data_ptr(), None,
                                                 ws.data_ptr(), C.c_void_p(st.cuda_stream)) == abi.OK
    assert L.spz_amd_render_finish_device(n, C.byref(p), m, image.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                          C.c_void_p(st.cuda_stream)) == abi.OK
    rec = torch.full((n, 9), -7.0, device=cuda)
    out = torch.full((3, 4), -7.0, dtype=torch.float64, device=cuda)
    vws = torch.empty(int(L.spz_amd_render_view_backward_workspace_bytes(n)), dtype=torch.uint8, device=cuda)
    assert L.spz_amd_render_records_backward_device(n, C.byref(p), m, G.data_ptr(), rec.data_ptr(),
                                                    status[1:].data_ptr(), ws.data_ptr(),
                                                    C.c_void_p(st.cuda_stream)) == abi.OK
    assert L.spz_amd_render_view_backward_device(C.byref(ptrs), n, deg, 0, C.byref(p), m, rec.data_ptr(), out.data_ptr(),
                                                 status[2:].data_ptr(), ws.data_ptr(), vws.data_ptr(),
                                                 C.c_void_p(st.cuda_stream)) == abi.OK
    torch.cuda.synchronize()
    assert int(total.cpu()[0]) == m + 1 and status.cpu().tolist() == [1, 1, 1]
    assert bool((rec == -7.0).all()) and bool((out == -7.0).all()) and bool((image == -7.0).all())


def test_side_stream(cuda):
    from spz_amd import device as D
    ref, vr = reference("sh3"), view_reference("sh3")
    cloud = D.to_device(ref["cloud"], cuda)
    G = torch.as_tensor(ref["G"]).to(cuda)
    side = torch.cuda.Stream(cuda)
    got = D.render_view_backward(cloud, ref["n"], ref["deg"], ref["params"], G, antialiased=ref["aa"], stream=side)
    side.synchronize()
    assert np.abs(got.cpu().numpy() - vr["v64"]).max() <= vr["bound"]


@pytest.mark.parametrize("name", ["sh3", "sh3_aa"])
def test_autograd_with_a_pose_tensor(cuda, name):
    """world_to_camera = the params' own matrix: the image is unchanged to the bit, the cloud's gradients stay within
    test_gpu_render_grad's bounds, and the pose tensor's gradient is render_view_backward's (both within the bound of
    the reference: the records are summed with atomics each time)."""
    from spz_amd import device as D
    from test_gpu_render_grad import check_gradients
    ref, vr = reference(name), view_reference(name)
    n, deg, p, aa = ref["n"], ref["deg"], ref["params"], ref["aa"]
    cloud = D.to_device(ref["cloud"], cuda)
    for t in cloud.values():
        t.requires_grad_(True)
    Wt = torch.tensor(np.array(list(p.world_to_camera)).reshape(3, 4), dtype=torch.float64, device=cuda,
                      requires_grad=True)
    img = D.render_autograd(cloud, n, deg, p, antialiased=aa, world_to_camera=Wt)
    plain = D.render_autograd({k: v.detach() for k, v in cloud.items()}, n, deg, p, antialiased=aa)
    assert np.array_equal(img.detach().cpu().numpy().view(np.uint32), plain.cpu().numpy().view(np.uint32))
    G = torch.as_tensor(ref["G"]).to(cuda)
    (img * G).sum().backward()
    got = {k: cloud[k].grad for k in cloud}
    got["records"] = torch.as_tensor(ref["g64"]["records"])  # not returned by autograd: nothing to compare
    check_gradients(got, ref, name + " with a pose")
    assert Wt.grad.shape == (3, 4) and Wt.grad.dtype == torch.float64
    assert np.abs(Wt.grad.cpu().numpy() - vr["v64"]).max() <= vr["bound"]
    direct = D.render_view_backward({k: v.detach() for k, v in cloud.items()}, n, deg, p, G, antialiased=aa)
    assert np.abs(Wt.grad.cpu().numpy() - direct.cpu().numpy()).max() <= 2.0 * vr["bound"]
    # the pose alone, on the CPU in float32: the gradient comes back in the tensor's own dtype and place
    W32 = torch.tensor(np.array(list(p.world_to_camera)).reshape(3, 4), dtype=torch.float32, requires_grad=True)
    img = D.render_autograd({k: v.detach() for k, v in cloud.items()}, n, deg, p, antialiased=aa, world_to_camera=W32)
    (img * G).sum().backward()
    assert W32.grad.dtype == torch.float32 and not W32.grad.is_cuda
    assert np.abs(W32.grad.numpy() - vr["v64"]).max() <= vr["bound"] + 2.0 ** -24 * np.abs(vr["v64"]).max()
    # a moved pose moves the image
    moved = torch.as_tensor(VR.perturbed(np.array(list(p.world_to_camera)).reshape(3, 4), 1.0, 0.01)).to(cuda)
    other = D.render_autograd({k: v.detach() for k, v in cloud.items()}, n, deg, p, antialiased=aa, world_to_camera=moved)
    q = type(p).from_buffer_copy(p)
    for k, x in enumerate(moved.cpu().reshape(-1).tolist()):
        q.world_to_camera[k] = x
    want = D.render({k: v.detach() for k, v in cloud.items()}, n, deg, q, antialiased=aa)
    assert np.array_equal(other.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


# ---- the fit

@functools.lru_cache(maxsize=None)
def fit_scene(width, height):
    cloud = GR.scene(1, 1, n=300)
    m, fx, fy, cx, cy = view_of(cloud["positions"], width=width, height=height)
    m0 = VR.perturbed(m, 3.0, 0.03, seed=0)
    return {"cloud": cloud, "truth": np.asarray(m, dtype=np.float32), "start": m0, "k": (fx, fy, cx, cy),
            "scale": float(np.linalg.norm(np.asarray(m)[:, 3]))}


def fit_params(s, m, width, height):
    from spz_amd import abi
    return abi.render_params(m, *s["k"], width, height, 0.2, BG, 3, 0)


def check_fit(s, res, what):
    r0, c0 = VR.pose_errors(s["start"], s["truth"])
    r1, c1 = VR.pose_errors(res["world_to_camera"], s["truth"])
    print(f"{what}: rotation {r0:.3f} -> {r1:.5f} degrees, centre {c0:.3e} -> {c1:.3e} of |t|, loss "
          f"{res['history'][0]:.4e} -> {res['history'][-1]:.4e}, psnr {res['before']['psnr']:.2f} -> "
          f"{res['after']['psnr']:.2f}, {res['ms'][1]:.0f} ms")
    assert abs(r0 - 3.0) < 1e-3 and 0.02 < c0 < 0.09
    assert r1 <= 0.1 * r0 and c1 <= 0.1 * c0
    assert all(r <= 0.01 * r0 and c <= 0.01 * c0 for r, c in REFERENCE_FIT.values())  # the reference has room
    assert res["iterations"] == len(res["history"]) and res["history"][-1] < res["history"][0]
    assert res["after"]["psnr"] > res["before"]["psnr"]


@pytest.mark.parametrize("lam", [0.0, None])
def test_fit_recovers_the_pose(cuda, lam):
    from spz_amd import device as D
    s = fit_scene(W, H)
    cloud = D.to_device(s["cloud"], cuda)
    target = D.render(cloud, 300, 1, fit_params(s, s["truth"], W, H))
    p0 = fit_params(s, s["start"], W, H)
    opts = dict(iterations=300, levels=1, lr_translation=2e-3 * s["scale"])
    if lam is not None:
        opts["lambda_dssim"] = lam
    res = D.locate(cloud, 300, 1, p0, target, **opts)
    check_fit(s, res, f"lambda {lam}")
    assert res["iterations"] == 300
    first, _ = D.image_loss(D.render(cloud, 300, 1, p0), target, 0.2 if lam is None else lam)
    assert res["history"][0] == float(first.cpu()[0]), "the first loss is image_loss of the initial render, bit for bit"
    # three channels of target, and no iterations
    res3 = D.locate(cloud, 300, 1, p0, target[..., :3].contiguous(), **dict(opts, iterations=0))
    assert res3["iterations"] == 0 and res3["history"] == [] and res3["before"] == res3["after"]
    assert np.array_equal(res3["world_to_camera"], s["start"])


def test_fit_of_a_packed_stream(cuda):
    """locate_packed: the stream decoded once; the metrics are the packed render's."""
    from spz_amd import abi, device as D
    s = fit_scene(W, H)
    cloud = D.to_device(s["cloud"], cuda)
    stream = D.encode(cloud, 300, 1)
    rc, header = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0
    target = D.render_packed(stream, header, fit_params(s, s["truth"], W, H))
    res = D.locate_packed(stream, header, fit_params(s, s["start"], W, H), target, iterations=300,
                          lr_translation=2e-3 * s["scale"])
    check_fit(s, res, "packed")
    assert res["after"]["psnr"] > 30.0


def test_levels(cuda):
    from spz_amd import abi, device as D
    w, h = 64, 48
    s = fit_scene(w, h)
    cloud = D.to_device(s["cloud"], cuda)
    target = D.render(cloud, 300, 1, fit_params(s, s["truth"], w, h))
    t = target.cpu().numpy()
    for c in (target, target[..., :3].contiguous()):
        half = D.image_halve(c)
        quarter = D.image_halve(half)
        want = VR.box_mean(c.cpu().numpy())
        assert np.array_equal(half.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(quarter.cpu().numpy().view(np.uint32), VR.box_mean(want).view(np.uint32))
    assert t.shape == (h, w, 4)
    res = D.locate(cloud, 300, 1, fit_params(s, s["start"], w, h), target, iterations=600, levels=3,
                   lr_translation=2e-3 * s["scale"])
    check_fit(s, res, "levels 3")
    s40 = fit_scene(W, H)
    with pytest.raises(abi.SpzAmdError) as e:
        D.locate(cloud, 300, 1, fit_params(s40, s40["start"], W, H), torch.zeros((H, W, 4), device=cuda), levels=4)
    assert e.value.args[0] == abi.ERR_INVALID_ARG or "invalid" in str(e.value).lower()


def test_the_layers_agree(cuda, tmp_path):
    """spz_render writes the picture from the true pose; device.locate_packed, spz.locate_spz (path and bytes: both
    spz::locateSpz) and the spz_locate tool fit the same rough pose to it with the same options.  The backward does not
    repeat its bits, so each is held to the fit's condition, not to the others' bits.  The views file spz_locate writes
    is one spz_compare takes."""
    import gzip
    import os
    import subprocess
    import spz_amd.spz as spz
    from conftest import ROOT
    from spz_amd import abi, device as D
    s = fit_scene(W, H)
    cloud = D.to_device(s["cloud"], cuda)
    stream = D.encode(cloud, 300, 1)
    raw = stream.cpu().numpy().tobytes()
    rc, header = abi.peek_header(raw)
    assert rc == 0
    scene = str(tmp_path / "scene.spz")
    with open(scene, "wb") as f:
        f.write(gzip.compress(raw, 6))
    # the eye and target of test_gpu_render.view_of
    p = s["cloud"]["positions"].astype(np.float64).reshape(-1, 3)
    lo, hi = np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)
    c, ext = 0.5 * (lo + hi), float(max(hi - lo))
    eye = c + np.array([0.3 * ext, 0.2 * ext, -2.2 * ext])
    assert np.array_equal(RR.look_at(eye, c, (0.0, 1.0, 0.0)), s["truth"])
    fx, fy, cx, cy = s["k"]
    bin_dir = os.path.join(ROOT, "spz_amd", "bin")
    shots = {}
    for ext_name in ("pfm", "ppm"):
        shots[ext_name] = str(tmp_path / f"truth.{ext_name}")
        run = subprocess.run([os.path.join(bin_dir, "spz_render"), scene, shots[ext_name], "--size", str(W), str(H),
                              "--intrinsics"] + [repr(float(x)) for x in (fx, fy, cx, cy)] + ["--eye"]
                             + [repr(float(np.float32(x))) for x in eye] + ["--target"]
                             + [repr(float(np.float32(x))) for x in c] + ["--background"] + [repr(x) for x in BG],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, (run.stdout, run.stderr)
    truth = D.render_packed(stream, header, fit_params(s, s["truth"], W, H)).cpu().numpy()
    image = spz.load_image(shots["pfm"])
    assert image.shape == (H, W, 3) and image.dtype == np.float32
    assert np.array_equal(image.view(np.uint32), truth[..., :3].view(np.uint32)), "the PFM carries the render's bits"
    want8 = np.floor(np.float32(255.0) * np.clip(truth[..., :3], 0.0, 1.0) + np.float32(0.5)) / np.float32(255.0)
    assert np.array_equal(spz.load_image(shots["ppm"]), want8)
    lt = 2e-3 * s["scale"]
    start = {"world_to_camera": s["start"], "fx": fx, "fy": fy, "cx": cx, "cy": cy, "width": W, "height": H}
    results = {"locate_packed": D.locate_packed(stream, header, fit_params(s, s["start"], W, H),
                                                torch.as_tensor(image).to(cuda), iterations=300, lr_translation=lt)}
    for name, source in (("locate_spz path", scene), ("locate_spz bytes", open(scene, "rb").read())):
        view, rep = spz.locate_spz(source, start, image, iterations=300, lr_translation=lt, background=BG)
        assert (view["fx"], view["width"], view["height"]) == (np.float32(fx), W, H) and rep["lr_translation"] == lt
        results[name] = dict(rep, world_to_camera=view["world_to_camera"])
    # the default translation step: lr_rotation times the distance from the camera to the bounding sphere's centre
    view, rep = spz.locate_spz(scene, start, image, iterations=0, background=BG)
    dec = D.decode(stream, header, 0)["positions"].cpu().numpy().astype(np.float64).reshape(-1, 3)
    centre = 0.5 * (dec.min(axis=0) + dec.max(axis=0))
    m0 = s["start"].astype(np.float64)
    dist = np.linalg.norm(-m0[:, :3].T @ m0[:, 3] - centre)
    assert abs(rep["lr_translation"] - 2e-3 * dist) <= 1e-5 * 2e-3 * dist and rep["iterations"] == 0
    assert np.array_equal(view["world_to_camera"], s["start"])
    views_file, fitted = tmp_path / "views.txt", tmp_path / "fitted.txt"
    views_file.write_text(" ".join([str(W), str(H)] + [repr(float(x)) for x in (fx, fy, cx, cy)]
                                   + [repr(float(x)) for x in s["start"].reshape(-1)]) + "\n")
    run = subprocess.run([os.path.join(bin_dir, "spz_locate"), scene, "--views", str(views_file), "--images",
                          shots["pfm"], "--iterations", "300", "--lr-translation", repr(lt), "--background"]
                         + [repr(x) for x in BG] + ["--out", str(fitted)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    note = run.stdout.strip().split("\n")
    assert len(note) == 1 and note[0].startswith("view 0 psnr ") and note[0].endswith("after 300 iterations")
    rows = [ln for ln in fitted.read_text().split("\n") if ln and not ln.startswith("#")]
    assert len(rows) == 1
    nums = [float(x) for x in rows[0].split()]
    assert nums[:2] == [W, H] and np.array_equal(np.float32(nums[2:6]), np.float32([fx, fy, cx, cy]))  # %.9g
    words = note[0].split()
    results["spz_locate"] = {"world_to_camera": np.array(nums[6:], dtype=np.float32).reshape(3, 4),
                             "before": {"psnr": float(words[3])}, "after": {"psnr": float(words[5])}}
    r0, c0 = VR.pose_errors(s["start"], s["truth"])
    for name, res in results.items():
        r1, c1 = VR.pose_errors(res["world_to_camera"], s["truth"])
        print(f"{name}: rotation {r1:.5f} degrees, centre {c1:.3e} of |t|, psnr {res['before']['psnr']:.2f} -> "
              f"{res['after']['psnr']:.2f}")
        assert r1 <= 0.1 * r0 and c1 <= 0.1 * c0, name
        assert res["after"]["psnr"] > res["before"]["psnr"], name
        assert res["before"]["psnr"] == results["locate_packed"]["before"]["psnr"], "the same first render everywhere"
    run = subprocess.run([os.path.join(bin_dir, "spz_compare"), scene, scene, "--views", str(fitted)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    # view and image counts must match
    run = subprocess.run([os.path.join(bin_dir, "spz_locate"), scene, "--views", str(views_file), "--images",
                          shots["pfm"], shots["ppm"]], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "1 views but 2 images" in run.stderr
