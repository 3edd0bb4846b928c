"""The image loss, the Adam step and refine on the GPU (include/spz_amd.h "image loss", "adam step", "refine"; DESIGN §8
"Refine"), against tests/loss_ref.py.

image_loss: L, l1 and ssim within 1e-7 absolute of the float64 restatement (the metrics contract's own SSIM bound; L is
a convex combination of l1 and 1 - ssim); the gradient within 8 max|ref32 - ref64| of it per image, ref32 being the same
restatement in float32 (the rule and the margin of test_gpu_render_grad.py: the device filters in f64 and rounds once,
ref32 filters in f32).

adam_step: bit for bit the float32 restatement, operation by operation.

refine: the scene is render_grad_ref.scene(REFINE_SEED, 1): 300 Gaussians of a few pixels, SH1, seen from 3 orbit views
of 48 x 40 in the RDF frame.  B is the scene; A is B with seeded noise on colours, alphas and scales, encoded again.
Before the seeds, the rates and the 30 iterations were fixed, the same loop was run on the CPU with render_grad_ref (the
forward and autograd in float64), loss_ref.loss_terms and loss_ref.adam_step from A's decoded floats: the reference
alone lowered the loss at every view's next visit (view 0 over its ten visits: 0.0853, 0.0757, 0.0685, ... 0.0406; the
last three steps 0.0406, 0.0376, 0.0356) and raised the mean PSNR of the three views from 22.62 dB to 28.02 dB on the
floats (see reference_loop(), five seconds on a CPU)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as LR
import metrics_ref as MR
import render_grad_ref as GR
import render_ref as RR
from conftest import ROOT, assert_bytes_equal

pytestmark = pytest.mark.gpu

ARRAYS = LR.ARRAYS


# ---- image_loss ----------------------------------------------------------------------------------------------------

SIZES = {"5x7": (5, 7), "29x37": (29, 37), "45x70": (45, 70)}   # H x W: under the window; partial tiles; 3 x 3 tiles
LAMBDAS = (0.2, 1.0, 0.0)


def planted_pair(h, w, ca, cb, seed):
    """Random images in [-0.2, 1.2] with exact 0s and 1s, NaN, +-inf and a block where a = b."""
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


@functools.lru_cache(maxsize=None)
def loss_reference(size, ca, cb, lam):
    """The pair and the restatement in float64 and float32: computed once and shared (nothing changes them)."""
    h, w = SIZES[size]
    a, b, spots = planted_pair(h, w, ca, cb, 17 * h + w + ca)
    return {"a": a, "b": b, "spots": spots, "r64": LR.loss(a, b, lam, torch.float64),
            "r32": LR.loss(a, b, lam, torch.float32)}


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("ca,cb", [(4, 3), (3, 4)])
@pytest.mark.parametrize("size", list(SIZES))
def test_image_loss_matches_the_restatement(cuda, size, ca, cb, lam):
    from spz_amd import device as D
    ref = loss_reference(size, ca, cb, lam)
    a, b, r64, r32 = ref["a"], ref["b"], ref["r64"], ref["r32"]
    a_t, b_t = torch.as_tensor(a).to(cuda), torch.as_tensor(b).to(cuda)
    loss_t, grad_t = D.image_loss(a_t, b_t, lam)
    assert loss_t.dtype == torch.float64 and tuple(grad_t.shape) == a.shape and grad_t.dtype == torch.float32
    got = loss_t.cpu().numpy()
    g = grad_t.cpu().numpy()
    for k, name in enumerate(("L", "l1", "ssim")):
        print(f"{size} {ca}/{cb} lambda {lam} {name}: device {got[k]!r}, ref64 {r64[name]!r}, off {abs(got[k] - r64[name]):.3e}")
        assert abs(got[k] - r64[name]) <= 1e-7, name
    # l1 and ssim are the metrics' own bits
    m = D.image_metrics(a_t, b_t).cpu().numpy()
    assert got[2] == m[2] and got[1] == m[3]
    bound = 8.0 * np.abs(r32["grad"] - r64["grad"]).max()
    err = np.abs(g.astype(np.float64) - r64["grad"]).max()
    print(f"{size} {ca}/{cb} lambda {lam} grad: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {bound:.3e}, "
          f"ratio to max|ref32 - ref64| {8.0 * err / bound if bound else 0.0:.4f}")
    if bound == 0.0:
        assert np.array_equal(g.astype(np.float64), r64["grad"])
    else:
        assert err <= bound
    if ca == 4:
        assert not g[..., 3].any() and not np.signbit(g[..., 3]).any(), "the alpha channel gets exactly 0"
    rgb = a[..., :3]
    outside = np.isnan(rgb) | (rgb < 0.0) | (rgb > 1.0)
    assert outside.sum() > 10 and not g[..., :3][outside].any(), "the clamp passes nothing outside [0, 1] or for NaN"
    for name in ("zero", "one"):
        at = ref["spots"][name]
        want = r64["grad"][at]
        assert (want != 0.0).sum() >= 2, "the reference passes gradient at the planted ends"
        assert ((g[at] != 0.0) == (want != 0.0)).all(), f"planted {name}s"
    # a run repeats its bits, on the current stream and on a side stream
    again_l, again_g = D.image_loss(a_t, b_t, lam, grad=torch.full_like(grad_t, -7.0))
    side = torch.cuda.Stream(cuda)
    side_l, side_g = D.image_loss(a_t, b_t, lam, stream=side)
    side.synchronize()
    for l2, g2 in ((again_l, again_g), (side_l, side_g)):
        assert np.array_equal(l2.cpu().numpy().view(np.uint64), got.view(np.uint64))
        assert np.array_equal(g2.cpu().numpy().view(np.uint32), g.view(np.uint32))


def test_image_loss_refuses_bad_arguments(cuda):
    from spz_amd import device as D
    a = torch.zeros((8, 9, 4), device=cuda)
    with pytest.raises(ValueError):
        D.image_loss(a, torch.zeros((8, 8, 4), device=cuda), 0.2)
    with pytest.raises(ValueError):
        D.image_loss(a, a, 1.5)
    with pytest.raises(ValueError):
        D.image_loss(a, a.cpu(), 0.2)
    with pytest.raises(ValueError):
        D.image_loss(a, a, 0.2, grad=torch.zeros((8, 9, 3), device=cuda))
    loss_t, grad_t = D.image_loss(a, a, 0.2)
    assert loss_t.cpu().tolist() == [0.0, 0.0, 1.0] and not grad_t.any()


# ---- adam_step -----------------------------------------------------------------------------------------------------

LRS = (1.6e-3, 5e-3, 1e-3, 5e-2, 2.5e-3, 1.25e-4)


def adam_state(n, deg, seed):
    """A cloud, gradients and moments (as after some steps) with planted zeros in g and +-inf and NaN in p and in g;
    `planted`: per array the indices of the elements a step must leave alone."""
    from spz_amd.synth import make_cloud_numpy
    rng = np.random.default_rng(seed)
    p = make_cloud_numpy(n, deg, seed)
    g, m, v, planted = {}, {}, {}, {}
    for k in ARRAYS:
        cnt = p[k].size
        g[k] = (rng.standard_normal(cnt) * 10.0 ** rng.uniform(-6, 1, cnt)).astype(np.float32)
        m[k] = (0.1 * rng.standard_normal(cnt)).astype(np.float32)
        v[k] = (0.01 * rng.standard_normal(cnt) ** 2).astype(np.float32)
        g[k][rng.random(cnt) < 0.1] = 0.0
        bad = []
        if cnt:
            idx = rng.permutation(cnt)[:min(cnt, 6)]
            for j, e in enumerate(idx):
                target = p[k] if j % 2 == 0 else g[k]
                target[e] = (np.inf, -np.inf, np.nan)[j % 3]
                bad.append(int(e))
        planted[k] = np.array(sorted(bad), dtype=np.int64)
    return p, g, m, v, planted


@pytest.mark.parametrize("t", [1, 100])
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_adam_step_is_the_f32_restatement_bit_for_bit(cuda, n, deg, t):
    from spz_amd import device as D
    p, g, m, v, planted = adam_state(n, deg, 1000 * n + 10 * deg + t)
    if t == 1:
        m = {k: np.zeros_like(x) for k, x in m.items()}
        v = {k: np.zeros_like(x) for k, x in v.items()}
    dev = [D.to_device(x, cuda) for x in (p, g, m, v)]
    skipped = D.adam_step(*dev, n, deg, t, LRS)
    total = 0
    for i, k in enumerate(ARRAYS):
        p1, m1, v1, bad = LR.adam_step(p[k], g[k], m[k], v[k], t, LRS[i])
        total += bad
        assert bad == planted[k].size
        for name, got, want, before in (("p", dev[0][k], p1, p[k]), ("m", dev[2][k], m1, m[k]), ("v", dev[3][k], v1, v[k])):
            got = got.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, name)
            assert np.array_equal(got[planted[k]].view(np.uint32), before[planted[k]].view(np.uint32)), (k, name)
        assert np.array_equal(dev[1][k].cpu().numpy().view(np.uint32), g[k].view(np.uint32)), "gradients are only read"
    assert int(skipped.cpu()[0]) == total
    # the counter adds up over steps
    D.adam_step(*dev, n, deg, t + 1, LRS, skipped=skipped)
    assert int(skipped.cpu()[0]) == 2 * total


def test_adam_step_unaligned_arrays_take_scalar_heads_and_tails(cuda):
    """Arrays that begin 4, 8 and 12 bytes past a 16-byte boundary, of lengths around the vector width."""
    from spz_amd import device as D
    rng = np.random.default_rng(5)
    for n, shift in ((1, 1), (2, 3), (5, 2), (67, 1), (130, 3)):
        host, dev = [], []
        for j in range(4):
            c = {k: rng.standard_normal(n * f).astype(np.float32) for k, f in
                 zip(ARRAYS, (3, 3, 4, 1, 3, 9))}
            if j == 3:
                c = {k: x * x for k, x in c.items()}
            host.append(c)
            d = {}
            for k, x in c.items():
                big = torch.zeros(x.size + 8, device=cuda)
                view = big[shift:shift + x.size]
                view.copy_(torch.as_tensor(x))
                assert view.data_ptr() % 16 == 4 * shift
                d[k] = view
            dev.append(d)
        D.adam_step(*dev, n, 1, 7, LRS)
        for i, k in enumerate(ARRAYS):
            p1, m1, v1, _ = LR.adam_step(host[0][k], host[1][k], host[2][k], host[3][k], 7, LRS[i])
            assert np.array_equal(dev[0][k].cpu().numpy().view(np.uint32), p1.view(np.uint32)), (n, k)
            assert np.array_equal(dev[2][k].cpu().numpy().view(np.uint32), m1.view(np.uint32)), (n, k)
            assert np.array_equal(dev[3][k].cpu().numpy().view(np.uint32), v1.view(np.uint32)), (n, k)


def test_adam_step_colours_only_touches_nothing_else(cuda):
    from spz_amd import device as D
    n, deg = 257, 3
    p, g, m, v, _ = adam_state(n, deg, 99)
    dev = [D.to_device(x, cuda) for x in (p, g, m, v)]
    sentinel = [{k: x.clone() for k, x in c.items()} for c in dev]
    D.adam_step(*dev, n, deg, 3, LRS, train=("colors",))
    for k in ARRAYS:
        for j in range(4):
            same = torch.equal(dev[j][k].view(torch.int32), sentinel[j][k].view(torch.int32))
            assert same == (k != "colors" or j == 1), (k, j)
    # the untrained arrays may be absent altogether
    only = [{"colors": D.to_device(x, cuda)["colors"]} for x in (p, g, m, v)]
    D.adam_step(*only, n, deg, 3, LRS, train=("colors",))
    assert torch.equal(only[0]["colors"].view(torch.int32), dev[0]["colors"].view(torch.int32))


# ---- refine --------------------------------------------------------------------------------------------------------

REFINE_SEED, NOISE_SEED, ITERATIONS = 4, 11, 30
RW, RH = 48, 40
COORD = 6  # RDF


@functools.lru_cache(maxsize=None)
def refine_scene():
    """B (the scene), A (B with noise on colours, alphas and scales), both packed by the CPU oracle from the RDF frame,
    the three orbit views as dicts, and the position rate (1.6e-4 times the bounding-sphere radius)."""
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
    return {"n": n, "deg": 1, "a": O.pack(a, n, 1, False, COORD), "b": O.pack(b, n, 1, False, COORD), "views": views,
            "lrs": {"positions": 1.6e-4 * radius}, "oracle": O}


def view_params(v, coord=COORD):
    from spz_amd import abi
    return abi.render_params(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                             v["height"], 0.2, (0.0, 0.0, 0.0), 3, coord)


def reference_loop(iterations=ITERATIONS):
    """The loop on the CPU, from A's decoded floats: render_grad_ref's forward and autograd in float64, loss_ref's loss,
    loss_ref.adam_step with refine's default rates.  Returns (history, mean PSNR before, mean PSNR after); what it gave
    is in this module's docstring.  Not run by the tests."""
    from spz_amd import abi
    s = refine_scene()
    O = s["oracle"]
    _, cloud = O.unpack(s["a"], COORD)
    _, target = O.unpack(s["b"], COORD)
    cloud = {k: cloud[k] for k in ARRAYS}
    cams = [RR.camera(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], RW, RH, 0.2, (0, 0, 0), 3)
            for v in s["views"]]
    targets = [RR.render({k: target[k] for k in ARRAYS}, 1, cam) for cam in cams]
    o = abi.refine_options(iterations, lrs=s["lrs"])
    psnr = lambda c: float(np.mean([MR.metrics(RR.render(c, 1, cam), t)[0]["psnr"]  # noqa: E731
                                    for cam, t in zip(cams, targets)]))
    before = psnr(cloud)
    m = {k: np.zeros_like(x) for k, x in cloud.items()}
    v = {k: np.zeros_like(x) for k, x in cloud.items()}
    history = []
    for i in range(iterations):
        cam, tgt = cams[i % 3], targets[i % 3]
        dec = GR.decisions(cloud, 1, cam)
        t = GR.as_tensors(cloud, torch.float64)
        img, _ = GR.forward(t, 1, cam, dec)
        L = LR.loss_terms(img, tgt, o.lambda_dssim)[0]
        L.backward()
        history.append(float(L.detach()))
        for j, k in enumerate(ARRAYS):
            g = (t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])).numpy().astype(np.float32)
            cloud[k], m[k], v[k], _ = LR.adam_step(cloud[k], g, m[k], v[k], i + 1, o.lr[j])
    return history, before, psnr(cloud)


@functools.lru_cache(maxsize=None)
def resident(cuda_index):
    from spz_amd import abi
    s = refine_scene()
    dev = torch.device("cuda", cuda_index)
    a_t, b_t = torch.as_tensor(s["a"]).to(dev), torch.as_tensor(s["b"]).to(dev)
    rc, ha = abi.peek_header(s["a"].tobytes())
    assert rc == 0
    rc, hb = abi.peek_header(s["b"].tobytes())
    assert rc == 0
    return a_t, ha, b_t, hb, [view_params(v) for v in s["views"]]


def sections(stream, n, deg):
    from spz_amd import abi
    lay = abi.stream_layout(n, deg, 3)
    s = np.asarray(stream)
    return {"header": s[:16], **{name: s[lay.offset[k]:lay.offset[k] + lay.bytes[k]] for k, name in
                                 enumerate(("positions", "alphas", "colors", "scales", "rotations", "sh"))}}


def test_refine_lowers_the_loss_and_raises_the_psnr_of_the_file(cuda, tmp_path):
    from spz_amd import abi, device as D
    import spz_amd.spz as spz
    s = refine_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    with D.refine_packed(a_t, ha, b_t, hb, views, ITERATIONS, lrs=s["lrs"]) as res:
        rep = res.report
        out = res.tensor().clone()
        assert np.array_equal(res.fetch(), out.cpu().numpy())
    hist = rep["history"]
    before = np.mean([m["psnr"] for m in rep["before"]])
    after = np.mean([m["psnr"] for m in rep["after"]])
    print(f"history {hist[0]:.6f} -> {hist[-1]:.6f}; mean PSNR {before:.3f} -> {after:.3f} dB; "
          f"mean SSIM {np.mean([m['ssim'] for m in rep['before']]):.4f} -> {np.mean([m['ssim'] for m in rep['after']]):.4f}; "
          f"skipped {rep['skipped']}; ms {rep['ms']}")
    assert len(hist) == ITERATIONS and hist[-1] < hist[0]
    assert after > before
    assert rep["out_bytes"] == s["a"].size == out.numel()
    out_np = out.cpu().numpy()
    assert_bytes_equal(out_np[:16], s["a"][:16], "the output header is A's")
    # the after (and before) metrics: of the packed renders against the target's, bit for bit
    for k, p in enumerate(views):
        tgt = D.render_packed(b_t, hb, p)
        for name, stream in (("before", a_t), ("after", out)):
            m = D.image_metrics(D.render_packed(stream, ha, p), tgt).cpu().numpy()
            got = rep[name][k]
            want = dict(zip(("mse", "psnr", "ssim", "l1", "max_abs"), m.tolist()))
            assert got == want, (name, k)
    # history[0]: the loss of the two forward renders, before any step
    o = abi.refine_options(0)
    cloud = D.decode(a_t, ha, COORD)
    img = D.render(cloud, s["n"], s["deg"], views[0], antialiased=False)
    loss0, _ = D.image_loss(img, D.render_packed(b_t, hb, views[0]), o.lambda_dssim)
    assert hist[0] == float(loss0.cpu()[0])
    # the same through the file layers: spz.refine_spz and spz_refine, file to file
    fa, fb, fo, fc = (str(tmp_path / x) for x in ("a.spz", "b.spz", "out.spz", "cli.spz"))
    import gzip
    for path, stream in ((fa, s["a"]), (fb, s["b"])):
        with open(path, "wb") as f:
            f.write(gzip.compress(stream.tobytes(), 6))
    r = spz.refine_spz(fa, fb, fo, s["views"], iterations=ITERATIONS, coord=spz.RDF, lrs=s["lrs"])
    assert len(r["history"]) == ITERATIONS and r["history"][0] == hist[0] and r["history"][-1] < r["history"][0]
    assert [m["psnr"] for m in r["before"]] == [m["psnr"] for m in rep["before"]]
    assert np.mean([m["psnr"] for m in r["after"]]) > before
    with gzip.open(fo, "rb") as f:
        written = np.frombuffer(f.read(), np.uint8)
    assert_bytes_equal(written[:16], s["a"][:16], "refine_spz's header")
    again = spz.compare_spz(fo, fb, s["views"], coord=spz.RDF)
    assert [m["psnr"] for m in again] == [m["psnr"] for m in r["after"]], "the report's after is the written file's"
    views_file = tmp_path / "views.txt"
    views_file.write_text("".join(
        " ".join([str(v["width"]), str(v["height"])] + [repr(float(x)) for x in (v["fx"], v["fy"], v["cx"], v["cy"])]
                 + [repr(float(x)) for x in np.asarray(v["world_to_camera"]).reshape(-1)]) + "\n" for v in s["views"]))
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_refine")
    run = subprocess.run([tool, fa, fb, fc, "--views", str(views_file), "--iters", str(ITERATIONS), "--coord", "RDF",
                          "--lr-positions", repr(s["lrs"]["positions"])], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 5 and lines[0].startswith("view 0 psnr ") and lines[3].startswith("mean psnr ")
    mean = lines[3].split()
    assert float(mean[2]) == before and float(mean[4]) > before
    assert os.path.getsize(fc) > 0


def test_refine_colours_only_keeps_the_other_sections_bytes(cuda):
    from spz_amd import device as D
    s = refine_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    with D.refine_packed(a_t, ha, b_t, hb, views, 6, train=("colors",)) as res:
        out = sections(res.fetch(), s["n"], s["deg"])
        rep = res.report
    want = sections(s["a"], s["n"], s["deg"])
    for name in ("header", "positions", "alphas", "scales", "rotations", "sh"):
        assert_bytes_equal(out[name], want[name], name)
    assert not np.array_equal(out["colors"], want["colors"])
    assert rep["history"][3] < rep["history"][0], "view 0's second visit"


def test_refine_zero_iterations_returns_the_input(cuda):
    from spz_amd import device as D
    s = refine_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    with D.refine_packed(a_t, ha, b_t, hb, views, 0) as res:
        assert_bytes_equal(res.fetch(), s["a"], "iterations = 0")
        assert res.report["history"] == [] and res.report["after"] == res.report["before"]
        assert res.report["skipped"] == 0


def test_refine_keeps_infinite_alphas(cuda):
    """Alpha bytes 0 and 255 decode to -inf and +inf: the steps leave them alone (and count them), and they encode to
    the same bytes."""
    from spz_amd import abi, device as D
    s = refine_scene()
    _, ha, b_t, hb, views = resident(cuda.index)
    a = s["a"].copy()
    lay = abi.stream_layout(s["n"], s["deg"], 3)
    at = lay.offset[abi.SEC_ALPHAS]
    a[at:at + 4] = (0, 255, 0, 255)
    iters = 4
    with D.refine_packed(torch.as_tensor(a).to(cuda), ha, b_t, hb, views, iters) as res:
        out = res.fetch()
        assert res.report["skipped"] == 4 * iters
    assert out[at:at + 4].tolist() == [0, 255, 0, 255]
    assert not np.array_equal(out[at + 4:at + s["n"]], a[at + 4:at + s["n"]])


def test_refine_names_a_bad_view_and_close_drops_the_result(cuda):
    from spz_amd import abi, device as D
    a_t, ha, b_t, hb, views = resident(cuda.index)
    worse = abi.RenderParams.from_buffer_copy(views[1])
    worse.fx = -1.0
    with pytest.raises(abi.SpzAmdError, match="view 1") as e:
        D.refine_packed(a_t, ha, b_t, hb, [views[0], worse, views[2]], 2)
    assert e.value.view == 1 and e.value.status == abi.ERR_INVALID_ARG
    other = abi.RenderParams.from_buffer_copy(views[2])
    other.coord = abi.RUB
    with pytest.raises(abi.SpzAmdError, match="view 2") as e:
        D.refine_packed(a_t, ha, b_t, hb, [views[0], views[1], other], 2)
    assert e.value.view == 2
    with pytest.raises(ValueError):
        D.refine_packed(a_t, ha, b_t, hb, [], 2)
    with pytest.raises(ValueError):
        D.refine_packed(a_t, ha, b_t, hb, views, 2, train=())
    res = D.refine_packed(a_t, ha, b_t, hb, views, 1)
    assert res.tensor().numel() == res.out_bytes
    res.close()
    res.close()  # closing twice is harmless
    with pytest.raises(RuntimeError, match="closed"):
        res.tensor()
    with pytest.raises(RuntimeError, match="closed"):
        res.fetch()
    assert res._ctx is None
