"""The photo loss, the exposure apply and refine against images on the GPU (include/spz_amd.h "photo loss" and "refine
images"; DESIGN §8 "Fit"), against tests/photo_ref.py.

photo_loss: L, l1 and ssim within 1e-7 absolute of the float64 restatement (the image loss's bound); the gradient to
the render within 8 max|ref32 - ref64| of it per image, ref32 being the same restatement in float32 (the rule and the
margin of test_gpu_refine.py), and the 12 exposure gradients likewise; exact equality where that bound is 0.

image_exposure: bit for bit the float32 restatement.

The loop runs on test_gpu_refine.py's scene (restated here): render_grad_ref.scene(4, 1), A = B with noise of seed 11 on
colours, alphas and scales, three 48 x 40 orbit views in the RDF frame, 30 iterations at refine's default rates.  With
B's renders as the images, no weights and no exposure, it is refine: history[0] and the "before" metrics carry
refine_packed's bits, and the conditions are that test's (the loss falls, the mean PSNR rises; its docstring's CPU loop
gave 22.62 -> 28.02 dB).

The exposure fit: A = B, the images are B's renders through E* = [0.8 I | 0.05], colours trained at rate 0, so only the
exposures move, from the identity: max|I - E*| = 0.2.  Before the iteration count was fixed the same loop was run on the
CPU (exposure_reference_loop(): render_ref once per view, photo_ref.photo_loss in float64, photo_ref.
exposure_adam_step); what it gave is in test_exposure_fit_recovers_a_planted_exposure's docstring."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

import photo_ref as PR
import render_grad_ref as GR
import render_ref as RR
from conftest import ROOT, assert_bytes_equal

pytestmark = pytest.mark.gpu

ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")

# ---- photo_loss ----------------------------------------------------------------------------------------------------

SIZES = {"5x7": (5, 7), "29x37": (29, 37), "45x70": (45, 70)}   # H x W: under the window; partial tiles; 3 x 3 tiles
LAMBDAS = (0.2, 1.0, 0.0)
WEIGHTS = ("none", "random", "zero")
EXPOSURES = ("none", "random")


def planted_pair(h, w, ca, cb, seed):
    """test_gpu_refine.py's pair: random images in [-0.2, 1.2] with exact 0s and 1s, NaN, +-inf and a block where a = b."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.2, 1.2, (h, w, ca)).astype(np.float32)
    b = rng.uniform(-0.2, 1.2, (h, w, cb)).astype(np.float32)
    flat = rng.permutation(h * w * 3)
    k = max(2, (h * w * 3) // 20)
    ys, xs, cs = np.unravel_index(flat[:6 * k], (h, w, 3))
    spots = {"zero": (ys[:k], xs[:k], cs[:k]), "one": (ys[k:2 * k], xs[k:2 * k], cs[k:2 * k])}
    a[spots["zero"]] = 0.0
    a[spots["one"]] = 1.0
    a[ys[2 * k], xs[2 * k], cs[2 * k]] = np.nan
    a[ys[2 * k + 1], xs[2 * k + 1], cs[2 * k + 1]] = np.inf
    a[ys[2 * k + 2], xs[2 * k + 2], cs[2 * k + 2]] = -np.inf
    b[ys[2 * k + 3], xs[2 * k + 3], cs[2 * k + 3]] = np.nan
    b[ys[2 * k + 4], xs[2 * k + 4], cs[2 * k + 4]] = np.inf
    b[ys[2 * k + 5], xs[2 * k + 5], cs[2 * k + 5]] = -np.inf
    by, bx = h // 2, w // 2
    b[by:by + 3, bx:bx + 4, :3] = a[by:by + 3, bx:bx + 4, :3]
    return a, b, spots


def weight_map(kind, h, w, seed):
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros((h, w), np.float32)
    rng = np.random.default_rng(seed + 1000)
    m = rng.uniform(-0.2, 1.2, (h, w)).astype(np.float32)
    m[rng.random((h, w)) < 0.05] = np.nan
    m[h // 3:h // 3 + 2, w // 4:w // 4 + 3] = 0.0
    return m


def exposure_of(kind, seed):
    if kind == "none":
        return None
    rng = np.random.default_rng(seed + 2000)
    return PR.IDENTITY + np.concatenate([0.2 * rng.standard_normal((3, 3)), 0.1 * rng.standard_normal((3, 1))], axis=1)


@functools.lru_cache(maxsize=None)
def photo_reference(size, ca, cb, lam, wkind, ekind):
    """The inputs and the restatement in float64 and float32: computed once and shared (nothing changes them)."""
    h, w = SIZES[size]
    seed = 17 * h + w + ca
    a, b, spots = planted_pair(h, w, ca, cb, seed)
    wt, ex = weight_map(wkind, h, w, seed), exposure_of(ekind, seed)
    return {"a": a, "b": b, "spots": spots, "weight": wt, "exposure": ex,
            "r64": PR.photo_loss(a, b, lam, wt, ex, torch.float64), "r32": PR.photo_loss(a, b, lam, wt, ex, torch.float32)}


def within(name, got, r64, r32, label):
    """|got - ref64| <= 8 max|ref32 - ref64|, exact equality where that is 0; prints device, reference and ratio."""
    bound = 8.0 * np.abs(r32 - r64).max()
    err = np.abs(got.astype(np.float64) - r64).max()
    print(f"{label} {name}: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {bound:.3e}, "
          f"ratio to max|ref32 - ref64| {8.0 * err / bound if bound else 0.0:.4f}")
    if bound == 0.0:
        assert np.array_equal(got.astype(np.float64), r64), name
    else:
        assert err <= bound, name


def on(cuda, x):
    return None if x is None else torch.as_tensor(x).to(cuda)


@pytest.mark.parametrize("ekind", EXPOSURES)
@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("ca,cb", [(4, 3), (3, 4)])
@pytest.mark.parametrize("size", list(SIZES))
def test_photo_loss_matches_the_restatement(cuda, size, ca, cb, lam, wkind, ekind):
    from spz_amd import device as D
    ref = photo_reference(size, ca, cb, lam, wkind, ekind)
    a, b, wt, ex, r64, r32 = ref["a"], ref["b"], ref["weight"], ref["exposure"], ref["r64"], ref["r32"]
    a_t, b_t, w_t = on(cuda, a), on(cuda, b), on(cuda, wt)
    loss_t, grad_t, egrad_t = D.photo_loss(a_t, b_t, lam, weight=w_t, exposure=ex)
    assert loss_t.dtype == torch.float64 and tuple(grad_t.shape) == a.shape and grad_t.dtype == torch.float32
    got, g = loss_t.cpu().numpy(), grad_t.cpu().numpy()
    label = f"{size} {ca}/{cb} lambda {lam} weights {wkind} exposure {ekind}"
    for k, name in enumerate(("L", "l1", "ssim")):
        print(f"{label} {name}: device {got[k]!r}, ref64 {r64[name]!r}, off {abs(got[k] - r64[name]):.3e}")
        assert abs(got[k] - r64[name]) <= 1e-7, name
    within("grad", g, r64["grad"], r32["grad"], label)
    if ex is None:
        assert egrad_t is None
    else:
        eg = egrad_t.cpu().numpy()
        assert eg.shape == (3, 4) and eg.dtype == np.float64
        within("exposure_grad", eg, r64["exposure_grad"], r32["exposure_grad"], label)
    if ca == 4:
        assert not g[..., 3].any() and not np.signbit(g[..., 3]).any(), "the alpha channel gets exactly 0"
    if wkind == "zero":
        assert got.tolist() == [0.0, 0.0, 1.0] and not g.any()
        assert ex is None or not egrad_t.cpu().numpy().any()
    # the gate: nothing passes where t is outside [0, 1] or NaN
    rgb = a[..., :3].astype(np.float64)
    if ex is None:
        t = rgb
    else:
        with np.errstate(all="ignore"):
            t = ((ex[:, 3] + ex[:, 0] * rgb[..., 0:1]) + ex[:, 1] * rgb[..., 1:2]) + ex[:, 2] * rgb[..., 2:3]
    closed = np.isnan(t) | (t < 0.0) | (t > 1.0)
    assert closed.sum() > 10
    if ex is None:
        assert not g[..., :3][closed].any(), "the clamp passes nothing outside [0, 1] or for NaN"
        if wkind != "zero":
            for name in ("zero", "one"):
                at = ref["spots"][name]
                want = r64["grad"][at]
                assert wkind == "random" or (want != 0.0).sum() >= 2, "the reference passes gradient at the planted ends"
                assert ((g[at] != 0.0) == (want != 0.0)).all(), f"planted {name}s"
    else:
        all_closed = closed.all(axis=-1)
        assert all_closed.sum() >= 1 and not g[..., :3][all_closed].any(), "a pixel with every gate closed gets nothing"
        # dL/da = M^T (gate . dL/da'): a pixel some of whose gates are open gets what the reference gives it
        some = ~all_closed & closed.any(axis=-1)
        assert some.sum() > 3 and ((g[..., :3][some] != 0.0) == (r64["grad"][..., :3][some] != 0.0)).all()
    # a run repeats its bits, on the current stream and on a side stream
    again = D.photo_loss(a_t, b_t, lam, weight=w_t, exposure=ex, grad=torch.full_like(grad_t, -7.0))
    side = torch.cuda.Stream(cuda)
    aside = D.photo_loss(a_t, b_t, lam, weight=w_t, exposure=ex, stream=side)
    side.synchronize()
    for l2, g2, e2 in (again, aside):
        assert np.array_equal(l2.cpu().numpy().view(np.uint64), got.view(np.uint64))
        assert np.array_equal(g2.cpu().numpy().view(np.uint32), g.view(np.uint32))
        if ex is not None:
            assert np.array_equal(e2.cpu().numpy().view(np.uint64), egrad_t.cpu().numpy().view(np.uint64))
    # without weights and exposure: the image loss's bits
    if wt is None and ex is None:
        loss_i, grad_i = D.image_loss(a_t, b_t, lam)
        assert np.array_equal(loss_i.cpu().numpy().view(np.uint64), got.view(np.uint64))
        assert np.array_equal(grad_i.cpu().numpy().view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize("ekind", EXPOSURES)
def test_photo_loss_gradient_crosses_a_mask_edge_through_the_windows(cuda, ekind):
    """45 x 70 with the weights 0 over columns 0..19: windows centred on columns >= 20 reach back to column 15, so the
    gradient is exactly 0 in columns 0..14 and not in 15..19."""
    from spz_amd import device as D
    h, w = SIZES["45x70"]
    a, b, _ = planted_pair(h, w, 4, 3, 3)
    wt = np.ones((h, w), np.float32)
    wt[:, :20] = 0.0
    _, grad_t, _ = D.photo_loss(on(cuda, a), on(cuda, b), 0.2, weight=on(cuda, wt), exposure=exposure_of(ekind, 3))
    g = grad_t.cpu().numpy()
    assert not g[:, :15].any()
    assert g[:, 15:20, :3].any(), "gradient through the windows"
    ref = PR.photo_loss(a, b, 0.2, wt, exposure_of(ekind, 3))["grad"]
    assert not ref[:, :15].any() and ref[:, 15:20, :3].any()


def test_photo_loss_refuses_bad_arguments(cuda):
    from spz_amd import abi, device as D
    a = torch.zeros((8, 9, 4), device=cuda)
    with pytest.raises(ValueError):
        D.photo_loss(a, torch.zeros((8, 8, 4), device=cuda), 0.2)
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 1.5)
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 0.2, weight=torch.zeros((9, 8), device=cuda))
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 0.2, weight=torch.zeros((8, 9), device=cuda, dtype=torch.float64))
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 0.2, exposure=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 0.2, exposure=np.full((3, 4), np.nan))
    with pytest.raises(ValueError):
        D.photo_loss(a, a, 0.2, grad=torch.zeros((8, 9, 3), device=cuda))
    # at the ABI: refused before a launch, nothing written
    L = abi.load_library()
    loss = torch.full((3,), -7.0, dtype=torch.float64, device=cuda)
    grad = torch.full((8, 9, 4), -7.0, device=cuda)
    ws = torch.empty(int(L.spz_amd_photo_loss_workspace_bytes(9, 8)), dtype=torch.uint8, device=cuda)
    ex = abi.exposure_values(PR.IDENTITY)
    call = lambda **k: L.spz_amd_photo_loss_device(  # noqa: E731
        k.get("a", a.data_ptr()), k.get("ca", 4), a.data_ptr(), 4, k.get("w", None), k.get("ex", None), k.get("wd", 9), 8,
        k.get("lam", 0.2), loss.data_ptr(), k.get("grad", grad.data_ptr()), k.get("eg", None), ws.data_ptr(), None)
    bad_ex = abi.exposure_values(PR.IDENTITY)
    bad_ex[5] = float("inf")
    for k in ({"a": None}, {"ca": 2}, {"wd": 0}, {"lam": float("nan")}, {"grad": None}, {"ex": ex}, {"ex": bad_ex, "eg": 8},
              {"w": a.data_ptr() + 2}, {"a": a.data_ptr() + 1}):
        assert call(**k) == abi.ERR_INVALID_ARG, k
    torch.cuda.synchronize()
    assert (loss == -7.0).all() and (grad == -7.0).all()
    loss_t, grad_t, _ = D.photo_loss(a, a, 0.2)
    assert loss_t.cpu().tolist() == [0.0, 0.0, 1.0] and not grad_t.any()


# ---- image_exposure ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("size", ["5x7", "45x70"])
def test_image_exposure_is_the_f32_restatement_bit_for_bit(cuda, size, ch):
    from spz_amd import device as D
    h, w = SIZES[size]
    a, _, _ = planted_pair(h, w, ch, 3, 7)
    ex = exposure_of("random", 7)
    want = PR.apply_exposure_f32(a, ex)
    a_t = on(cuda, a)
    out = D.image_exposure(a_t, ex)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(a_t.cpu().numpy().view(np.uint32), a.view(np.uint32)), "the input is only read"
    if ch == 4:
        assert np.array_equal(out.cpu().numpy()[..., 3].view(np.uint32), a[..., 3].view(np.uint32)), "alpha is copied"
    same = D.image_exposure(a_t, ex, out=a_t)   # in place
    assert same is a_t and np.array_equal(a_t.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        D.image_exposure(a_t, np.zeros(11))
    with pytest.raises(ValueError):
        D.image_exposure(a_t, ex, out=torch.zeros((h, w, 7 - ch), device=cuda))


# ---- the loop ------------------------------------------------------------------------------------------------------

REFINE_SEED, NOISE_SEED, ITERATIONS = 4, 11, 30
RW, RH = 48, 40
COORD = 6  # RDF
E_STAR = np.array([[0.8, 0.0, 0.0, 0.05], [0.0, 0.8, 0.0, 0.05], [0.0, 0.0, 0.8, 0.05]])
FIT_ITERATIONS, FIT_LR = 120, 0.02


@functools.lru_cache(maxsize=None)
def refine_scene():
    """test_gpu_refine.py's scene: B, A (B with noise on colours, alphas and scales), both packed by the CPU oracle from
    the RDF frame, the three orbit views as dicts, and the position rate (1.6e-4 times the bounding-sphere radius)."""
    import spz_amd.spz as spz
    from oracle.pyoracle import Oracle
    O = Oracle()
    b = GR.scene(REFINE_SEED, 1)
    n = b["alphas"].size
    rng = np.random.default_rng(NOISE_SEED)
    a = {k: v.copy() for k, v in b.items()}
    a["colors"] = (a["colors"] + 0.5 * rng.standard_normal(a["colors"].size)).astype(np.float32)
    a["alphas"] = (a["alphas"] + 1.0 * rng.standard_normal(n)).astype(np.float32)
    a["scales"] = (a["scales"] + 0.3 * rng.standard_normal(a["scales"].size)).astype(np.float32)
    p = b["positions"].reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    views = spz.orbit_views(3, width=RW, height=RH, fov_y=50.0, center=centre.tolist(), radius=radius)
    keep = np.sort(np.random.default_rng(5).permutation(n)[:150])
    sub = {k: b[k].reshape(n, -1)[keep].reshape(-1).copy() for k in ARRAYS}
    return {"n": n, "deg": 1, "a": O.pack(a, n, 1, False, COORD), "b": O.pack(b, n, 1, False, COORD),
            "sub": O.pack(sub, keep.size, 1, False, COORD), "n_sub": int(keep.size), "views": views,
            "lrs": {"positions": 1.6e-4 * radius}, "oracle": O}


def view_params(v, coord=COORD):
    from spz_amd import abi
    return abi.render_params(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                             v["height"], 0.2, (0.0, 0.0, 0.0), 3, coord)


def exposure_reference_loop(iterations=FIT_ITERATIONS, lr=FIT_LR):
    """The exposure fit on the CPU: render_ref's render of B once per view (rounded to float32, as the device's image
    is), the targets through E* with photo_ref.apply_exposure_f32, then per iteration photo_ref.photo_loss in float64
    and photo_ref.exposure_adam_step on that view's 12 values.  Returns (history, max|E - E*| over the views); what it
    gave is in the exposure test's docstring.  Not run by the tests."""
    s = refine_scene()
    _, cloud = s["oracle"].unpack(s["b"], COORD)
    cloud = {k: cloud[k] for k in ARRAYS}
    cams = [RR.camera(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], RW, RH, 0.2, (0, 0, 0), 3)
            for v in s["views"]]
    renders = [RR.render(cloud, 1, cam).astype(np.float32) for cam in cams]
    targets = [PR.apply_exposure_f32(r, E_STAR) for r in renders]
    e = [PR.IDENTITY.reshape(-1).copy() for _ in cams]
    m, v2 = [np.zeros(12) for _ in cams], [np.zeros(12) for _ in cams]
    visits, history = [0] * len(cams), []
    for i in range(iterations):
        v = i % len(cams)
        r = PR.photo_loss(renders[v], targets[v], 0.2, None, e[v].reshape(3, 4))
        history.append(r["L"])
        visits[v] += 1
        e[v], m[v], v2[v] = PR.exposure_adam_step(e[v], r["exposure_grad"].reshape(-1), m[v], v2[v], visits[v], lr)
    return history, max(float(np.abs(x - E_STAR.reshape(-1)).max()) for x in e)


@functools.lru_cache(maxsize=None)
def resident(cuda_index):
    """A, B and the 150-point subset of B on the device with their headers, the views' params, and B's packed renders."""
    from spz_amd import abi, device as D
    s = refine_scene()
    dev = torch.device("cuda", cuda_index)
    out = {}
    for name in ("a", "b", "sub"):
        rc, hdr = abi.peek_header(s[name].tobytes())
        assert rc == 0
        out[name] = (torch.as_tensor(s[name]).to(dev), hdr)
    out["views"] = [view_params(v) for v in s["views"]]
    out["targets"] = [D.render_packed(*out["b"], p) for p in out["views"]]
    return out


def sections(stream, n, deg):
    from spz_amd import abi
    lay = abi.stream_layout(n, deg, 3)
    s = np.asarray(stream)
    return {"header": s[:16], **{name: s[lay.offset[k]:lay.offset[k] + lay.bytes[k]] for k, name in
                                 enumerate(("positions", "alphas", "colors", "scales", "rotations", "sh"))}}


def test_refine_images_with_rendered_targets_is_refine(cuda):
    from spz_amd import device as D
    s = refine_scene()
    r = resident(cuda.index)
    (a_t, ha), (b_t, hb), views, targets = r["a"], r["b"], r["views"], r["targets"]
    with D.refine_packed(a_t, ha, b_t, hb, views, ITERATIONS, lrs=s["lrs"]) as res:
        want = res.report
    with D.refine_packed_images(a_t, ha, views, targets, ITERATIONS, lrs=s["lrs"]) as res:
        rep = res.report
        out = res.tensor().clone()
        assert np.array_equal(res.fetch(), out.cpu().numpy())
    hist = rep["history"]
    before = np.mean([m["psnr"] for m in rep["before"]])
    after = np.mean([m["psnr"] for m in rep["after"]])
    print(f"history {hist[0]:.6f} -> {hist[-1]:.6f}; mean PSNR {before:.3f} -> {after:.3f} dB; skipped {rep['skipped']}; "
          f"ms {rep['ms']}")
    assert len(hist) == ITERATIONS and hist[0] == want["history"][0]
    assert rep["before"] == want["before"]
    assert hist[-1] < hist[0]
    assert after > before
    assert rep["out_bytes"] == s["a"].size == out.numel() and rep["num_points"] == s["n"]
    assert_bytes_equal(out.cpu().numpy()[:16], s["a"][:16], "the output header is A's")
    assert np.array_equal(rep["exposures"], np.broadcast_to(PR.IDENTITY, (3, 3, 4)))
    for k, p in enumerate(views):
        m = D.image_metrics(D.render_packed(out, ha, p), targets[k]).cpu().numpy()
        assert rep["after"][k] == dict(zip(("mse", "psnr", "ssim", "l1", "max_abs"), m.tolist())), k


def write_pfm(path, rgb):
    """A colour PFM as spz_render writes it (little-endian, scale -1.0, rows bottom to top): float32 values, exactly."""
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n" + f"{w} {h}\n".encode() + b"-1.0\n")
        f.write(np.ascontiguousarray(rgb[::-1]).astype("<f4").tobytes())


def test_refine_images_through_the_file_layers(cuda, tmp_path):
    """spz.refine_spz_to_images and spz_fit, file to file, on the same images written as PFM: history[0] and the "before"
    metrics are the resident loop's (both come before any step); the report's "after" is the written file's."""
    import spz_amd.spz as spz
    from spz_amd import device as D
    s = refine_scene()
    r = resident(cuda.index)
    (a_t, ha), views, targets = r["a"], r["views"], r["targets"]
    with D.refine_packed_images(a_t, ha, views, targets, ITERATIONS, lrs=s["lrs"]) as res:
        want = res.report
    before = np.mean([m["psnr"] for m in want["before"]])
    images = [t.cpu().numpy()[..., :3].copy() for t in targets]
    # three channels in place of the render's four: the loss and the metrics read the first three
    fa, fo, fc = (str(tmp_path / x) for x in ("a.spz", "out.spz", "cli.spz"))
    with open(fa, "wb") as f:
        f.write(gzip.compress(s["a"].tobytes(), 6))
    rep = spz.refine_spz_to_images(fa, fo, s["views"], images, iterations=ITERATIONS, coord=spz.RDF, lrs=s["lrs"])
    assert len(rep["history"]) == ITERATIONS and rep["history"][0] == want["history"][0]
    assert rep["history"][-1] < rep["history"][0]
    assert [m["psnr"] for m in rep["before"]] == [m["psnr"] for m in want["before"]]
    assert np.mean([m["psnr"] for m in rep["after"]]) > before
    assert np.array_equal(rep["exposures"], np.broadcast_to(PR.IDENTITY, (3, 3, 4))) and rep["num_points"] == s["n"]
    with gzip.open(fo, "rb") as f:
        written = np.frombuffer(f.read(), np.uint8)
    assert_bytes_equal(written[:16], s["a"][:16], "refine_spz_to_images' header")
    out_t = torch.as_tensor(written.copy()).to(cuda)
    for k, p in enumerate(views):
        m = D.image_metrics(D.render_packed(out_t, ha, p), targets[k]).cpu().numpy()
        assert rep["after"][k]["psnr"] == m[1] and rep["after"][k]["ssim"] == m[2], "after is the written file's"
    # bytes in, bytes out
    rb = spz.refine_spz_to_images(gzip.compress(s["a"].tobytes(), 6), None, s["views"], images, iterations=2,
                                  coord=spz.RDF, lrs=s["lrs"])
    assert rb["history"][0] == want["history"][0] and len(gzip.decompress(rb["data"])) == s["a"].size
    # the tool
    views_file = tmp_path / "views.txt"
    views_file.write_text("".join(
        " ".join([str(v["width"]), str(v["height"])] + [repr(float(x)) for x in (v["fx"], v["fy"], v["cx"], v["cy"])]
                 + [repr(float(x)) for x in np.asarray(v["world_to_camera"]).reshape(-1)]) + "\n" for v in s["views"]))
    pfms = []
    for k, img in enumerate(images):
        pfms.append(str(tmp_path / f"view{k}.pfm"))
        write_pfm(pfms[-1], img)
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_fit")
    run = subprocess.run([tool, fa, fc, "--views", str(views_file), "--images"] + pfms +
                         ["--iters", str(ITERATIONS), "--coord", "RDF", "--lr-positions", repr(s["lrs"]["positions"])],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 5 and lines[0].startswith("view 0 psnr ") and lines[3].startswith("mean psnr ")
    mean = lines[3].split()
    assert float(mean[2]) == before and float(mean[4]) > before
    assert float(lines[4].split()[1]) == want["history"][0]
    assert os.path.getsize(fc) > 0
    # masks and a fitted exposure through the tool: the left half does not count, the exposures are written
    mask = np.ones((RH, RW, 3), np.float32)
    mask[:, :RW // 2] = 0.0
    mask_file, ex_file = str(tmp_path / "mask.pfm"), str(tmp_path / "exposures.txt")
    write_pfm(mask_file, mask)
    run = subprocess.run([tool, fa, fc, "--views", str(views_file), "--images"] + pfms + ["--masks"] + [mask_file] * 3 +
                         ["--fit-exposure", "--lr-exposure", "0.02", "--exposures-out", ex_file, "--iters", "6", "--coord",
                          "RDF", "--lr-positions", repr(s["lrs"]["positions"])], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    wt = torch.as_tensor(mask[..., 0].copy()).to(cuda)
    with D.refine_packed_images(a_t, ha, views, targets, 1, weights=[wt] * 3, fit_exposure=True, lrs=s["lrs"]) as res:
        assert float(run.stdout.strip().split("\n")[4].split()[1]) == res.report["history"][0]
    ex = np.loadtxt(ex_file)
    assert ex.shape == (3, 12) and not np.array_equal(ex[0], PR.IDENTITY.reshape(-1))
    assert np.abs(ex - PR.IDENTITY.reshape(-1)).max() < 0.1, "two visits per view at 0.02 move each value by about 0.04"


def test_refine_images_weights_enter_the_loss(cuda):
    """The weights 0 on the left half of every view: history[0] is photo_loss of the two forward renders with them."""
    from spz_amd import abi, device as D
    s = refine_scene()
    r = resident(cuda.index)
    (a_t, ha), views, targets = r["a"], r["views"], r["targets"]
    wt = torch.ones((RH, RW), device=cuda)
    wt[:, :RW // 2] = 0.0
    with D.refine_packed_images(a_t, ha, views, targets, 3, weights=[wt, wt, wt], lrs=s["lrs"]) as res:
        hist = res.report["history"]
    img = D.render(D.decode(a_t, ha, COORD), s["n"], s["deg"], views[0], antialiased=False)
    loss0, _, _ = D.photo_loss(img, targets[0], abi.refine_options(0).lambda_dssim, weight=wt)
    assert hist[0] == float(loss0.cpu()[0])
    plain, _ = D.image_loss(img, targets[0], abi.refine_options(0).lambda_dssim)
    assert hist[0] != float(plain.cpu()[0])


def test_exposure_fit_recovers_a_planted_exposure(cuda):
    """A = B, the images B's renders through E*, colours trained at rate 0: only the exposures move.  The reference loop
    alone (exposure_reference_loop(), two seconds on a CPU) at lr_exposure 0.02: max|E - E*| over the three views 0.1063
    after 15 iterations, 0.0963 after 60, 0.0620 after 90, 0.0346 after 105, 0.0209 after 120, 0.0148 after 150 (at
    3DGS's 0.01 it is still 0.0488 after 150); the loss of the views' first visits 0.0767, 0.0853, 0.0891, of their last
    of 120 iterations 0.0015, 0.0030, 0.0016.  So 120 iterations at 0.02: the reference alone is under a quarter of
    max|I - E*| = 0.2 with a factor 2.4 to spare.  The device is asked for half of it, a factor 2 over the reference's
    quarter for the cloud's f32 render."""
    from spz_amd import device as D
    s = refine_scene()
    r = resident(cuda.index)
    (b_t, hb), views = r["b"], r["views"]
    targets = [D.image_exposure(t, E_STAR) for t in r["targets"]]
    for t in targets:
        assert 0.0 <= float(t[..., :3].min()) and float(t[..., :3].max()) <= 1.0
    kw = dict(train=("colors",), lrs={"colors": 0.0})
    with D.refine_packed_images(b_t, hb, views, targets, FIT_ITERATIONS, fit_exposure=True, lr_exposure=FIT_LR, **kw) as res:
        rep = res.report
    err = float(np.abs(rep["exposures"] - E_STAR).max())
    start = float(np.abs(PR.IDENTITY - E_STAR).max())
    hist = rep["history"]
    print(f"max|E - E*| {start:.4f} -> {err:.5f}; history {hist[0]:.6f} -> {hist[-3]:.6f} {hist[-2]:.6f} {hist[-1]:.6f}; "
          f"mean PSNR {np.mean([m['psnr'] for m in rep['before']]):.3f} -> {np.mean([m['psnr'] for m in rep['after']]):.3f}")
    assert err < 0.5 * start
    assert hist[-3] < hist[0] and hist[-2] < hist[1] and hist[-1] < hist[2], "every view's loss fell"
    # the after metrics: the output's packed render through the fitted exposure
    out_np = None
    with D.refine_packed_images(b_t, hb, views, targets, 6, fit_exposure=True, lr_exposure=FIT_LR, **kw) as res:
        out_np, rep6 = res.tensor().clone(), res.report
    for k, p in enumerate(views):
        img = D.image_exposure(D.render_packed(out_np, hb, p), rep6["exposures"][k])
        m = D.image_metrics(img, targets[k]).cpu().numpy()
        assert rep6["after"][k] == dict(zip(("mse", "psnr", "ssim", "l1", "max_abs"), m.tolist())), k
    # without the fit: the identity, and a rate of 0 leaves the colours' bytes alone
    with D.refine_packed_images(b_t, hb, views, targets, 6, fit_exposure=False, **kw) as res:
        assert np.array_equal(res.report["exposures"], np.broadcast_to(PR.IDENTITY, (3, 3, 4)))
        got = sections(res.fetch(), s["n"], s["deg"])
    want = sections(s["b"], s["n"], s["deg"])
    assert_bytes_equal(got["colors"], want["colors"], "colours at rate 0")


def test_refine_images_densify_keeps_its_structure(cuda):
    """A is a 150-point subset of B: structure only (no CPU reference of this loop with densify has been run)."""
    from spz_amd import abi, device as D
    s = refine_scene()
    r = resident(cuda.index)
    (sub_t, hs), views, targets = r["sub"], r["views"], r["targets"]
    dn = {"interval": 10, "from_iter": 0, "until_iter": ITERATIONS, "max_points": s["n"]}
    with D.refine_packed_images(sub_t, hs, views, targets, ITERATIONS, lrs=s["lrs"], densify=dn) as res:
        rep, out = res.report, res.fetch()
    assert len(rep["rounds"]) == ITERATIONS // 10
    assert 0 < rep["num_points"] <= s["n"] and rep["origin"].size == rep["num_points"]
    rc, hdr = abi.peek_header(out.tobytes())
    assert rc == 0 and hdr.num_points == rep["num_points"] and out.size == rep["out_bytes"]
    rc, cloud = s["oracle"].unpack(out, COORD)
    assert rc == 0 and cloud["alphas"].size == rep["num_points"]
    with pytest.raises(abi.SpzAmdError) as e:
        D.refine_packed_images(sub_t, hs, views, targets, ITERATIONS, lrs=s["lrs"], densify=dict(dn, max_points=0))
    assert e.value.status == abi.ERR_INVALID_ARG


def test_refine_images_refusals_and_close(cuda):
    import ctypes as C
    from spz_amd import abi, device as D
    r = resident(cuda.index)
    (a_t, ha), views, targets = r["a"], r["views"], r["targets"]
    L = abi.load_library()
    arr = (abi.RenderParams * 3)(*views)
    opts, popts = abi.refine_options(2), abi.photo_options()

    def call(tptrs, channels=4, wptrs=None, photo=popts):
        ctx, nbytes, bad = C.c_void_p(), C.c_uint64(), C.c_int32(-1)
        hist = (C.c_double * 2)()
        rc = L.spz_amd_refine_images_open(a_t.data_ptr(), a_t.numel(), C.byref(ha), arr, 3, tptrs, channels, wptrs,
                                          C.byref(opts), C.byref(photo) if photo is not None else None, None,
                                          cuda.index, C.byref(ctx), C.byref(nbytes), hist, None, None, None, None,
                                          C.byref(bad), None, None, 0, None, None, None)
        assert ctx.value is None and nbytes.value == 0
        return rc, bad.value

    good = [t.data_ptr() for t in targets]
    assert call(None) == (abi.ERR_INVALID_ARG, -1)
    assert call((C.c_void_p * 3)(good[0], None, good[2])) == (abi.ERR_INVALID_ARG, 1)
    assert call((C.c_void_p * 3)(*good), wptrs=(C.c_void_p * 3)(None, None, good[2] + 2)) == (abi.ERR_INVALID_ARG, 2)
    assert call((C.c_void_p * 3)(*good), channels=2) == (abi.ERR_INVALID_ARG, -1)
    assert call((C.c_void_p * 3)(*good), photo=None) == (abi.ERR_INVALID_ARG, -1)
    for lr in (-1.0, float("nan")):
        bad = abi.PhotoOptions(1, 0, lr)
        assert call((C.c_void_p * 3)(*good), photo=bad) == (abi.ERR_INVALID_ARG, -1)
        with pytest.raises(ValueError):
            D.refine_packed_images(a_t, ha, views, targets, 2, fit_exposure=True, lr_exposure=lr)
    with pytest.raises(ValueError):
        D.refine_packed_images(a_t, ha, views, targets[:2], 2)
    with pytest.raises(ValueError):
        D.refine_packed_images(a_t, ha, views, [targets[0], targets[1], targets[2][:, :-1].contiguous()], 2)
    with pytest.raises(ValueError):
        D.refine_packed_images(a_t, ha, views, targets, 2, weights=[None, None])
    res = D.refine_packed_images(a_t, ha, views, targets, 1)
    assert res.tensor().numel() == res.out_bytes
    res.close()
    res.close()  # closing twice is harmless
    with pytest.raises(RuntimeError, match="closed"):
        res.tensor()
    with pytest.raises(RuntimeError, match="closed"):
        res.fetch()
    assert res._ctx is None
