"""The rasteriser's kernels on views from inside the scene (tests/frustum_ref.py; DESIGN §8 "Render", "Render backward",
"Locate"): the arms of the per-Gaussian chain that a camera outside the cloud never takes.  Every scene asserts, from
the reference alone, that it reaches them: Gaussians behind the camera, inside near, off the image and non-finite ones
shuffled among the visible ones of every wave; quotients of J clamped at each of the four lim values and at two at once,
on Gaussians wide enough to be used by 20 and more pixels; tile rectangles cut at each edge of the grid; under
antialiasing, discs whose det0 spans more than four decades.  tests/test_render_frustum_host.py runs the same scenes
without a GPU, the CPU build of the two per-Gaussian chains among them.

The rules are the suite's, unchanged, and no constant is new:
  records      test_gpu_render.check_records, and the visible set equal to the reference's over the whole class table
  images       test_gpu_render_scale.check_pixels (1e-4; 0.05 at a pixel with a marginal pair), check_accumulated,
               test_gpu_prune.check_scores; the scenes have no marginal pair (at most 1 % would be allowed)
  gradients    test_gpu_render_grad's: per array |device - ref64| <= 8 max|ref32 - ref64|, over all Gaussians, and
               then over the clamped class alone and the cut-rect class alone, each against the same ref32 / ref64
               pair restricted to the class, so that a small class cannot hide under the crowd's maximum; an exact 0
               in every entry of an invisible Gaussian (the six arrays, the record rows, the depth row); all finite
  view         test_gpu_locate's two: 1e-10 of sum |contribution| from given record gradients (two runs repeat their
               bits), 8 max|ref32 - ref64| from the image gradient; the clamped class carries 5 % and more of
               sum |contribution| of some pose entry, or the test could not see the clamp
  order        the invisible Gaussians moved to the end or to the front of the input leave the image's bits, and the
               gradients gathered back meet the gradient rule

What these scenes found.  A NaN alpha on an otherwise visible Gaussian.  The opacity was not among the preprocess
kernel's finiteness tests, so the record carried opacity = NaN, and fminf(0.99f, NaN) = 0.99f made every blend kernel
take the Gaussian as an opaque one over its whole rectangle, where numpy's minimum keeps the NaN and the reference
dropped every pair; the blend backward then formed da * NaN, and the preprocess backward 0 * NaN.  Read from the code
(spz_render.hip, spz_render_backward.hip) and measured on the MI355X before the change: the image off by 0.70 (plain)
and 1.01 (antialiased) where 1e-4 is allowed, the visible sets unequal, every array of render_backward and
render_depth_backward with NaN rows, all 12 entries of the view gradient NaN; 11 of this module's 13 tests failed.  After
it all 13 pass, with the figures below.  The rule is "non-finite inputs become invisible
Gaussians": spz_render_preprocess_kernel and render_ref.preprocess now test the opacity with the other values, the
Gaussian is invisible on both sides, and its gradients are exact zeros.

Measured (MI355X; the worst ratio of an error to max|ref32 - ref64| over the arrays, bound 8; per class all / clamped /
cut):
  render_backward         plain 1.56 / 0.70 / 0.60   antialiased 0.75 / 0.93 / 0.43   strip 0.23 / 0.46 / 0.09
  render_depth_backward   plain 0.57 / 0.57 / 0.68   antialiased 0.57 / 0.81 / 0.43
  records backward        plain 0.66 / 0.66 / 0.34   antialiased 0.36 / 0.36 / 0.27
  with the invisible Gaussians at the end or at the front: render_backward's figures again, digit for digit
  view from the image gradient   plain 0.30, antialiased 0.07
  view from given record gradients   1.8e-16 and 3.1e-16 of sum |contribution| (bound 1e-10); the clamped class
                          carries up to 0.08 (plain) and 0.16 (antialiased) of a pose entry's sum |contribution|
  images and accumulated depth   at most 0.006 of their 1e-4; no pixel has a marginal pair"""
import functools

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
import depth_ref as DR
import frustum_ref as F
import prune_ref as PR
import render_grad_ref as GR
import render_ref as RR
import view_grad_ref as VR
from test_gpu_prune import check_scores
from test_gpu_render import check_records
from test_gpu_render_grad import ARRAYS
from test_gpu_render_scale import check_accumulated, check_pixels

pytestmark = pytest.mark.gpu

SMALL = ("plain", "aa")


def params_of(s):
    from spz_amd import abi
    m, fx, fy, cx, cy = s["view"]
    cam = s["cam"]
    return abi.render_params(m, fx, fy, cx, cy, cam["width"], cam["height"], F.NEAR, F.BG, 3, 0)


@functools.lru_cache(maxsize=None)
def reference(variant, depth=True, view=True):
    """The variant's scene, image gradients and float64 / float32 reference gradients: computed once and shared
    (nothing changes them)."""
    s = F.scene(variant)
    cloud, deg, cam, dec, aa = s["cloud"], s["deg"], s["cam"], s["dec"], s["aa"]
    rng = np.random.default_rng(300 + len(variant))
    G = rng.standard_normal((cam["height"], cam["width"], 4)).astype(np.float32)
    GD = rng.standard_normal((cam["height"], cam["width"])).astype(np.float32)
    ref = {"s": s, "G": G, "GD": GD, "params": params_of(s),
           "colour": {"g64": GR.gradients(cloud, deg, cam, dec, G, aa, torch.float64),
                      "g32": GR.gradients(cloud, deg, cam, dec, G, aa, torch.float32)}}
    if depth:
        ref["depth"] = {"g64": DG.gradients(cloud, deg, cam, dec, G, GD, aa, torch.float64),
                        "g32": DG.gradients(cloud, deg, cam, dec, G, GD, aa, torch.float32)}
    if view:
        ref["view"] = {"v64": VR.view_gradient(cloud, deg, cam, dec, G, aa, torch.float64)["view"],
                       "v32": VR.view_gradient(cloud, deg, cam, dec, G, aa, torch.float32)["view"]}
    return ref


def class_rows(s):
    return {"all": np.arange(s["n"]), "clamped": F.members(s["labels"], "clamp"), "cut": F.members(s["labels"], "cut")}


def check_gradients(got, ref, s, what, keys, gather=None):
    """test_gpu_render_grad.check_gradients' rule over all Gaussians, then over the clamped class and the cut-rect class
    alone (bounds from the same ref32 / ref64 pair restricted to the class); exact zeros for the invisible Gaussians;
    everything finite.  gather: the permutation the device's cloud was stored in (row j of got is Gaussian gather[j]).
    Returns {class: the worst ratio of an error to max|ref32 - ref64|}."""
    n = s["n"]
    hidden = ~s["dec"]["visible"]
    rows = class_rows(s)
    worst = {}
    for k in keys:
        g = F.rows_of(got[k].detach().cpu().numpy(), n)
        if gather is not None:
            back = np.empty_like(g)
            back[gather] = g
            g = back
        want, low = F.rows_of(ref["g64"][k], n), F.rows_of(ref["g32"][k], n)
        assert np.isfinite(g).all(), f"{what} {k}: a value is not finite"
        assert not g[hidden].any(), f"{what} {k}: an invisible Gaussian's entry is not an exact 0"
        for name, r in rows.items():
            bound = 8.0 * np.abs(low[r] - want[r]).max()
            err = np.abs(g[r] - want[r]).max()
            ratio = 8.0 * err / bound if bound else 0.0
            print(f"{what} {k} [{name}]: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {bound:.3e}, "
                  f"ratio to max|ref32 - ref64| {ratio:.3f}")
            if bound == 0.0:
                assert np.array_equal(g[r], want[r]), f"{what} {k} [{name}]: must match exactly"
            else:
                assert err <= bound, f"{what} {k} [{name}]: {err} above {bound}"
            worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"{what}: worst ratio to max|ref32 - ref64| per class (bound 8): "
          + ", ".join(f"{name} {v:.2f}" for name, v in worst.items()))
    return worst


def check_visibility(rec_t, rec, s, what):
    """check_records, and the visible set equal over the whole class table (the scene has no r3 near an integer)."""
    check_records(rec_t, rec)
    got = np.isfinite(rec_t["depth"].cpu().numpy())
    wrong = np.nonzero(got != rec["visible"])[0]
    assert wrong.size == 0, f"{what}: visibility differs for {[(int(i), str(s['labels'][i])) for i in wrong]}"
    assert int(rec_t["total"].cpu()[0]) == RR.entry_count(rec)


@pytest.mark.parametrize("variant", SMALL)
def test_preprocess_of_the_float_cloud(cuda, variant):
    """The records and the visible set, the non-finite Gaussians included: all eight are invisible on the device as in
    the reference, the NaN alpha among them (the module's docstring)."""
    from spz_amd import device as D
    s = F.scene(variant)
    rec_t = D.preprocess(D.to_device(s["cloud"], cuda), s["n"], s["deg"], params_of(s), antialiased=s["aa"])
    check_visibility(rec_t, s["dec"]["rec"], s, variant)
    got = np.isfinite(rec_t["depth"].cpu().numpy())
    assert not got[F.members(s["labels"], "nonfinite")].any()
    for k in ("mean", "conic", "opacity", "rgb"):
        assert torch.isfinite(rec_t[k]).all(), f"{k}: a stored record value is not finite"
    print(f"{variant}: {got.sum()} of {s['n']} visible, classes {s['counts']}")


@pytest.mark.parametrize("variant", SMALL)
def test_preprocess_of_the_packed_stream(cuda, variant):
    """The finite classes through a v3 stream: the class table is asserted again on the decoded floats (quantisation
    moves things), and the packed preprocess gives the records and the visible set of their reference."""
    from spz_amd import abi, device as D
    s = F.scene(variant)
    f = F.finite_part(s)
    stream = D.encode(D.to_device(f["cloud"], cuda), f["n"], f["deg"], s["aa"], abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0 and h.num_points == f["n"]
    floats = {k: v.cpu().numpy() for k, v in D.decode(stream, h, abi.RUB).items()}
    rec = RR.preprocess(floats, f["deg"], f["cam"], s["aa"])
    counts = F.check_classes(f, rec)
    r3 = rec["r3"][rec["visible"]]
    assert (np.abs(r3 - np.round(r3)) >= 1e-4).all(), "a decoded Gaussian's r3 lies within 1e-4 of an integer"
    p = params_of(s)
    check_visibility(D.preprocess_packed(stream, h, p), rec, f, f"{variant} packed")
    print(f"{variant} packed: classes {counts}")


@pytest.mark.parametrize("variant", SMALL)
def test_render_depth_and_score(cuda, variant):
    from spz_amd import device as D
    ref = reference(variant)
    s = ref["s"]
    cloud_np, n, deg, cam, aa, dec, p = s["cloud"], s["n"], s["deg"], s["cam"], s["aa"], s["dec"], ref["params"]
    rec = dec["rec"]
    marginal = dec["marginal_mask"]
    assert marginal.mean() <= 0.01, "more than 1 % of the pixels have a marginal pair in the reference"
    cloud = D.to_device(cloud_np, cuda)
    img = D.render(cloud, n, deg, p, antialiased=aa)
    assert torch.isfinite(img).all()
    check_pixels(img.cpu().numpy(), ref["colour"]["g64"]["image"], marginal, f"{variant} image")
    depth, _ = D.render_depth(cloud, n, deg, p, antialiased=aa)
    want = DR.render_depth(cloud_np, deg, cam, aa, rec=rec)
    z = rec["depth"][rec["visible"]]
    check_accumulated(depth[..., 0].cpu().numpy(), want["accumulated"], marginal, float(z.max() - z.min()),
                      f"{variant} accumulated depth")
    wsum, wmax = D.score(cloud, n, deg, [p], antialiased=aa)
    want_sum, want_max, _ = PR.view_scores(cloud_np, deg, cam, aa, rec=rec)
    check_scores(wsum.cpu().numpy(), wmax.cpu().numpy(), want_sum, want_max)
    hidden = ~dec["visible"]
    assert not wsum.cpu().numpy()[hidden].any() and not wmax.cpu().numpy()[hidden].any()


@pytest.mark.parametrize("variant", SMALL)
def test_render_backward_and_render_depth_backward(cuda, variant):
    from spz_amd import device as D
    ref = reference(variant)
    s = ref["s"]
    n, deg, aa, p = s["n"], s["deg"], s["aa"], ref["params"]
    cloud = D.to_device(s["cloud"], cuda)
    G, GD = torch.as_tensor(ref["G"]).to(cuda), torch.as_tensor(ref["GD"]).to(cuda)
    got = D.render_backward(cloud, n, deg, p, G, antialiased=aa, return_record_grads=True)
    check_gradients(got, ref["colour"], s, f"{variant} render_backward", ARRAYS + ("records",))
    got = D.render_depth_backward(cloud, n, deg, p, G, GD, antialiased=aa, return_record_grads=True)
    check_gradients(got, ref["depth"], s, f"{variant} render_depth_backward", ARRAYS + ("records", "depth"))
    if aa:
        disc = F.members(s["labels"], "disc")
        flat = s["dec"]["rec"]["det0"][disc] <= 0
        assert not got["alphas"].cpu().numpy()[disc][flat].any(), "a disc with det0 <= 0 has an alpha gradient"


@pytest.mark.parametrize("variant", SMALL)
def test_render_view_backward(cuda, variant):
    from spz_amd import device as D
    ref = reference(variant)
    s = ref["s"]
    cloud_np, n, deg, cam, aa, dec, p = s["cloud"], s["n"], s["deg"], s["cam"], s["aa"], s["dec"], ref["params"]
    cloud = D.to_device(cloud_np, cuda)
    # from given record gradients: both sides run the chain in f64 on the same f32 values
    rg = ref["colour"]["g64"]["records"].astype(np.float32)
    per = VR.chain(cloud_np, deg, cam, dec, rg, aa, forward_mode=True)
    want, mag = per.sum(axis=0), np.abs(per).sum(axis=0)
    share = np.abs(per[F.members(s["labels"], "clamp")]).sum(axis=0) / mag
    print(f"{variant}: the clamped class carries up to {share.max():.3f} of sum |contribution| of a pose entry")
    assert share.max() >= 0.05, "the clamped class carries too little of the pose gradient to be seen"
    rg_t = torch.as_tensor(rg).to(cuda)
    got = [D.render_view_backward(cloud, n, deg, p, None, antialiased=aa, record_grads=rg_t).cpu().numpy()
           for _ in range(2)]
    assert got[0].shape == (3, 4) and got[0].dtype == np.float64 and np.isfinite(got[0]).all()
    err = np.abs(got[0] - want) / mag
    print(f"{variant}: |device - ref| / sum|contribution| at most {err.max():.3e} (bound 1e-10)")
    assert np.all(np.abs(got[0] - want) <= 1e-10 * mag)
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)), "two runs differ"
    # from the image gradient
    v64, v32 = ref["view"]["v64"], ref["view"]["v32"]
    bound = 8.0 * np.abs(v32 - v64).max()
    view, rec = D.render_view_backward(cloud, n, deg, p, torch.as_tensor(ref["G"]).to(cuda), antialiased=aa,
                                       return_record_grads=True)
    err = np.abs(view.cpu().numpy() - v64).max()
    print(f"{variant} view: |device - ref64| {err:.3e}, 8 max|ref32 - ref64| {bound:.3e}, "
          f"ratio to max|ref32 - ref64| {8.0 * err / bound:.3f}")
    assert bound > 0.0 and err <= bound
    check_gradients({"records": rec}, ref["colour"], s, f"{variant} records backward", ("records",))


@pytest.mark.parametrize("variant", SMALL)
def test_the_place_of_the_invisible_gaussians_in_the_input_does_not_matter(cuda, variant):
    """The same cloud with its invisible Gaussians moved to the end, and to the front (both stable, so equal depths keep
    their order): the same image bits, and gradients that meet the rule once gathered back."""
    from spz_amd import device as D
    ref = reference(variant)
    s = ref["s"]
    n, deg, aa, p = s["n"], s["deg"], s["aa"], ref["params"]
    vis = s["dec"]["visible"]
    G = torch.as_tensor(ref["G"]).to(cuda)
    img = D.render(D.to_device(s["cloud"], cuda), n, deg, p, antialiased=aa)
    for where, order in (("end", np.argsort(~vis, kind="stable")), ("front", np.argsort(vis, kind="stable"))):
        moved = {k: np.ascontiguousarray(v.reshape(n, -1)[order]).reshape(-1) for k, v in s["cloud"].items()}
        cloud = D.to_device(moved, cuda)
        again = D.render(cloud, n, deg, p, antialiased=aa)
        assert torch.equal(again.view(torch.int32), img.view(torch.int32)), f"invisible at the {where}: other bits"
        got = D.render_backward(cloud, n, deg, p, G, antialiased=aa, return_record_grads=True)
        check_gradients(got, ref["colour"], s, f"{variant} invisible at the {where}", ARRAYS + ("records",),
                        gather=order)


def test_render_backward_past_one_strip_of_the_image(cuda):
    """40 x 292: 19 tile rows, the same classes along the long axis, so a rectangle cut at the far edge of the grid and
    a clamped y quotient are taken with tiles_y that is not tiny."""
    from spz_amd import device as D
    ref = reference("strip", depth=False, view=False)
    s = ref["s"]
    assert RR.tiles(s["cam"]) == (3, 19)
    n, deg, p = s["n"], s["deg"], ref["params"]
    cloud = D.to_device(s["cloud"], cuda)
    rec_t = D.preprocess(cloud, n, deg, p)
    check_visibility(rec_t, s["dec"]["rec"], s, "strip")
    got = D.render_backward(cloud, n, deg, p, torch.as_tensor(ref["G"]).to(cuda), return_record_grads=True)
    check_gradients(got, ref["colour"], s, "strip render_backward", ARRAYS + ("records",))
