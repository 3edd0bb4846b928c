"""spz_amd_refine_images_depth_open / spz_amd.device.refine_packed_images(depths=...) on the GPU (include/spz_amd.h
"refine images with depth"; DESIGN §8 "Depth fit").

The scene is tests/depth_grad_ref.fit_scene's: B, the 300-Gaussian SH0 scene; A, B with its positions moved by seeded
Gaussian noise; two views at 40 x 36; the images are B's renders and the depth maps B's expected depth where alpha >=
0.5 and +inf elsewhere, both from the float64 references rounded to float32, so that the device and the reference loop
are given the same bits.  Positions alone are trained, depth weight 1, L1.

The reference loop (depth_grad_ref.fit_loop, run on the CPU by that file's __main__, about twenty seconds) wrote
tests/golden/depth_fit_expected.json.  Its inputs (noise 1.0, rate 3e-2, 120 iterations) were chosen by two conditions
on the reference alone, both asserted before the file is written.  Within at most 120 iterations the reference brings
the mean depth error to at most half of its start.  And the depth error is large enough for the 1e-6 relative bound
below to be one a float32 blend can meet: the reference's own forward in float32 is off by up to 3.1e-7 absolute in a
view's depth error whatever the noise, and 1e-6 of 0.70 and 0.68 is more than twice that (with noise 0.25, a depth
error of 0.16, the float32 reference missed the bound by itself: 1.87e-6).  Measured on an MI355X, relative to the
float64 reference: history[0] 3.3e-7, the depth error before 3.7e-7 and 6.4e-7; these come from the forward alone,
which repeats its bits.  Mean depth error 0.692 -> 0.0254 with the depth term (the reference: 0.0255) and -> 0.5007
with weight 0 (the reference: 0.5010)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
from conftest import ROOT
from test_gpu_refine import view_params

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(ROOT, "tests", "golden", "depth_fit_expected.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def scene():
    return DG.fit_scene(expected()["noise"])


def run(cuda, depths="maps", **kw):
    """refine_packed_images on the fit scene: the report.  depths: "maps", "nones" (a list of None) or None."""
    from spz_amd import abi, device as D
    s, e = scene(), expected()
    a_t = torch.as_tensor(s["a"]).to(cuda)
    rc, ha = abi.peek_header(s["a"].tobytes())
    assert rc == 0
    views = [view_params(v, DG.FIT_COORD) for v in s["views"]]
    images = [torch.as_tensor(x).to(cuda) for x in s["images"]]
    maps = {"maps": [torch.as_tensor(x).to(cuda) for x in s["depths"]], "nones": [None, None], None: None}[depths]
    with D.refine_packed_images(a_t, ha, views, images, kw.pop("iterations", e["iterations"]),
                                lrs={"positions": e["lr_positions"]}, train=("positions",), depths=maps, **kw) as res:
        return res.report


def test_no_depth_is_the_path_of_refine_images(cuda):
    """Through the depth entry with no map at all, history and before carry the other entry's bits."""
    old = run(cuda, None, iterations=1)
    new = run(cuda, "nones", iterations=1)
    assert "depth_history" not in old and "depth_error" not in old
    assert np.float64(new["history"][0]).tobytes() == np.float64(old["history"][0]).tobytes()
    for a, b in zip(new["before"], old["before"]):
        assert a.keys() == b.keys()
        for k in a:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k
    assert new["depth_history"] == [0.0] and np.array_equal(new["depth_error"], np.full((2, 2), -1.0))
    # weight 0 with maps: today's path as well, but the errors are reported
    zero = run(cuda, "maps", iterations=1, depth_weight=0.0)
    assert np.float64(zero["history"][0]).tobytes() == np.float64(old["history"][0]).tobytes()
    assert zero["depth_history"] == [0.0] and (zero["depth_error"] > 0).all()


def run_every_option(cuda, iterations, densify):
    """Photo loss with a weight map, a fitted exposure, a depth map on view 0 alone, every array trained and, when given,
    densify with the opacity reset: (report, output stream, A's header, views, images, weight map, depth map)."""
    from spz_amd import abi, device as D
    s, e = scene(), expected()
    a_t = torch.as_tensor(s["a"]).to(cuda)
    rc, ha = abi.peek_header(s["a"].tobytes())
    assert rc == 0
    views = [view_params(v, DG.FIT_COORD) for v in s["views"]]
    images = [torch.as_tensor(x).to(cuda) for x in s["images"]]
    weight = torch.zeros((DG.FIT_H, DG.FIT_W), dtype=torch.float32, device=cuda)
    weight[:, DG.FIT_W // 2:] = 1.0
    depth = torch.as_tensor(s["depths"][0]).to(cuda)
    with D.refine_packed_images(a_t, ha, views, images, iterations, weights=[weight, None], fit_exposure=True,
                                lrs={"positions": e["lr_positions"]}, densify=densify, depths=[depth, None]) as res:
        return res.report, res.tensor().clone(), ha, views, images, weight, depth


def test_every_option_at_once(cuda):
    """Weights, exposure, depth, densify and the opacity reset in one call of 12 iterations: what the forward makes
    repeatable (everything before the first step carries the bits of the one-iteration call without densify; "after" and
    the depth error of the output are those of the output stream rendered again) and the structure of the report.
    Neither growth nor a smaller loss is asserted: nothing on the CPU has shown either for this configuration."""
    from spz_amd import abi, device as D
    dn = {"interval": 4, "from_iter": 0, "until_iter": 12, "opacity_reset_interval": 6, "max_points": 400}
    first = run_every_option(cuda, 1, None)[0]
    rep, out, ha, views, images, weight, depth = run_every_option(cuda, 12, dn)
    bits = lambda x: np.float64(x).tobytes()  # noqa: E731
    assert len(rep["history"]) == len(rep["depth_history"]) == 12
    assert bits(rep["history"][0]) == bits(first["history"][0])
    assert bits(rep["depth_history"][0]) == bits(first["depth_history"][0])
    assert bits(rep["depth_error"][:, 0]) == bits(first["depth_error"][:, 0])
    for a, b in zip(rep["before"], first["before"]):
        assert a.keys() == b.keys() and all(bits(a[k]) == bits(b[k]) for k in a)
    assert all(rep["depth_history"][i] == 0.0 for i in range(1, 12, 2))  # view 1 has no map
    assert rep["depth_error"][1].tolist() == [-1.0, -1.0]
    # the rounds
    n_a = int(ha.num_points)
    assert [r["iteration"] for r in rep["rounds"]] == [3, 7, 11]
    count = n_a
    for r in rep["rounds"]:
        assert r["num_points"] == count - r["culled"] + r["cloned"] + r["split"], r
        count = r["num_points"]
    n = rep["num_points"]
    print(f"rounds {rep['rounds']}; {n_a} -> {n} points; history {rep['history'][0]!r} -> {rep['history'][-1]!r}")
    assert n == count and n <= 400
    origin = rep["origin"]
    assert origin.shape == (n,) and (origin < n_a).all() and (np.diff(origin.astype(np.int64)) >= 0).all()
    # the output stream
    assert out.numel() == rep["out_bytes"] == abi.stream_layout(n, 0, 3).total_bytes
    ho = abi.Header.from_buffer_copy(ha)
    ho.num_points = n
    rc, got = abi.peek_header(out.cpu().numpy().tobytes())
    assert rc == 0 and bytes(got) == bytes(ho), "the output's header is A's except for the count"
    assert np.isfinite(rep["exposures"]).all() and rep["exposures"].shape == (2, 3, 4)
    for v, p in enumerate(views):
        shown = D.image_exposure(D.render_packed(out, ho, p), rep["exposures"][v])
        m = D.image_metrics(shown, images[v]).cpu().numpy()
        assert rep["after"][v] == dict(zip(("mse", "psnr", "ssim", "l1", "max_abs"), m.tolist())), v
    z, image = D.render_depth_packed(out, ho, views[0], return_image=True, return_index=False)
    loss, _ = D.depth_loss(z, image, depth, weight=weight, kind="l1", min_alpha=0.5, scale=1.0)
    assert bits(rep["depth_error"][0, 1]) == bits(loss.cpu().numpy()[0])


@functools.lru_cache(maxsize=None)
def fitted(cuda_index):
    """The run with the depth term, shared by the tests below (nothing changes it)."""
    return run(torch.device("cuda", cuda_index))


def test_the_first_losses_are_the_reference_s(cuda):
    """history[0], the depth error before and depth_history[0] within 1e-6 relative of the reference's."""
    ref = expected()["with_depth"]
    rep = fitted(cuda.index)
    before = rep["depth_error"][:, 0]
    print(f"history[0] {rep['history'][0]!r} (ref {ref['history'][0]!r}); depth_history[0] {rep['depth_history'][0]!r} "
          f"(ref {ref['depth_history'][0]!r}); before {before.tolist()} (ref {ref['before']})")
    assert rep["depth_history"][0] == pytest.approx(before[0], rel=1e-12)  # the same render, the same loss
    assert rep["history"][0] == pytest.approx(ref["history"][0], rel=1e-6)
    assert rep["depth_history"][0] == pytest.approx(ref["depth_history"][0], rel=1e-6)
    for v in range(2):
        assert before[v] == pytest.approx(ref["before"][v], rel=1e-6), v


def test_the_loop_reduces_the_depth_error(cuda):
    """The final depth error is at most sqrt(before * the reference's after), the geometric middle between no progress
    and the reference's progress (f32 atomics and decisions made anew every step let two runs of a hundred steps
    drift).  And, the reference's own runs with the depth term and with weight 0 ending more than 1.5 x apart, the
    device's run with the depth term ends below its run with weight 0."""
    e = expected()
    ref = e["with_depth"]
    rep = fitted(cuda.index)
    before, after = rep["depth_error"][:, 0], rep["depth_error"][:, 1]
    print(f"before {before.tolist()} (ref {ref['before']}); after {after.tolist()} (ref {ref['after']}); "
          f"history {rep['history'][0]!r} -> {rep['history'][-1]!r} (ref {ref['history'][0]!r} -> {ref['history'][-1]!r})")
    assert len(rep["history"]) == len(rep["depth_history"]) == e["iterations"]
    mean_before, mean_after = float(np.mean(before)), float(np.mean(after))
    assert np.mean(ref["after"]) <= 0.5 * np.mean(ref["before"])  # the condition the inputs were chosen by
    assert mean_after <= np.sqrt(mean_before * np.mean(ref["after"])), (mean_before, mean_after)
    zero = run(cuda, depth_weight=0.0)
    mean_zero = float(np.mean(zero["depth_error"][:, 1]))
    print(f"mean depth error after: {mean_after!r} with the depth term, {mean_zero!r} with weight 0 "
          f"(ref {np.mean(ref['after'])!r} and {np.mean(e['weight_0']['after'])!r})")
    if np.mean(e["weight_0"]["after"]) > 1.5 * np.mean(ref["after"]):
        assert mean_after < mean_zero
