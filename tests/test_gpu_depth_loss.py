"""spz_amd_depth_loss_device / spz_amd.device.depth_loss (include/spz_amd.h "depth loss"; DESIGN §8 "Depth fit") on the
GPU against tests/depth_grad_ref.depth_loss, which gets the device's inputs as the same bits.

Images 5 x 7 (one partial workgroup), 29 x 37 (five workgroups, the last partial) and 45 x 70 (thirteen partial sums
for the final reduction).  L and W_v: 1e-12 relative, at most 3,150 float64 terms summed in a tree against math.fsum.
Gradients: each is a handful of float64 operations rounded once to float32, within 2^-22 relative of the reference's
value rounded to float32; exact 0 where invalid."""
import numpy as np
import pytest
import torch

import depth_grad_ref as DG

pytestmark = pytest.mark.gpu

SIZES = ((5, 7), (29, 37), (45, 70))  # (height, width)
MIN_ALPHA = 0.5


def inputs(h, w, weights, seed=0):
    """(depth (h, w, 2), image (h, w, 4), target (h, w), weight or None), float32: about a quarter of the pixels are
    invalid for one reason or another."""
    rng = np.random.default_rng(1000 * h + w + seed)
    alpha = rng.uniform(0.3, 1.0, (h, w)).astype(np.float32)
    t = rng.uniform(1.0, 9.0, (h, w)).astype(np.float32)
    D = (alpha * t * rng.uniform(0.7, 1.4, (h, w))).astype(np.float32)
    t[rng.random((h, w)) < 0.05] = np.inf
    D[rng.random((h, w)) < 0.03] = 0.0
    depth = np.stack([D, rng.standard_normal((h, w)).astype(np.float32)], axis=2)
    image = rng.standard_normal((h, w, 4)).astype(np.float32)
    image[..., 3] = alpha
    if weights == "none":
        wt = None
    elif weights == "zero":
        wt = np.zeros((h, w), np.float32)
    else:
        wt = rng.uniform(-0.2, 1.3, (h, w)).astype(np.float32)
    return depth, image, t, wt


def on_device(cuda, arrays):
    return [torch.as_tensor(a).to(cuda) if a is not None else None for a in arrays]


def check(cuda, depth, image, t, wt, kind, scale, min_alpha=MIN_ALPHA, what=""):
    """Runs the device loss with a grad_image to add into and checks everything against the reference; returns the
    reference and the device's (loss, grad_depth, grad_image) as numpy arrays."""
    from spz_amd import device as D
    ref = DG.depth_loss(depth, image, t, wt, kind, min_alpha, scale)
    d_depth, d_image, d_t, d_w = on_device(cuda, (depth, image, t, wt))
    old = np.random.default_rng(5).standard_normal(image.shape).astype(np.float32)
    old[..., 3] = 0.0
    old[0, 0, 3] = 0.25  # the photo loss writes 0 there; any value must be added to
    gi = torch.as_tensor(old).to(cuda)
    loss, gd = D.depth_loss(d_depth, d_image, d_t, weight=d_w, kind=kind, min_alpha=min_alpha, scale=scale, grad_image=gi)
    loss, gd, gi = loss.cpu().numpy(), gd.cpu().numpy(), gi.cpu().numpy()
    print(f"{what}: L {loss[0]!r} (ref {ref['L']!r}), W_v {loss[1]!r} (ref {ref['W_v']!r}), "
          f"{int(ref['valid'].sum())} of {ref['valid'].size} pixels valid")
    assert abs(loss[0] - ref["L"]) <= 1e-12 * max(1.0, abs(ref["L"]))
    assert abs(loss[1] - ref["W_v"]) <= 1e-12 * max(1.0, abs(ref["W_v"]))
    want_d = ref["g_depth"].astype(np.float32)
    assert gd.shape == want_d.shape and gd.dtype == np.float32
    assert np.all(np.abs(gd.astype(np.float64) - want_d) <= 2.0 ** -22 * np.abs(want_d)), what
    assert not gd[~ref["valid"]].any(), "exact 0 at every invalid pixel"
    # channel 3 is the old value plus g_alpha (one f32 addition of the f32-rounded gradient); channels 0-2 keep their bits
    g_alpha = gi[..., 3].astype(np.float64) - old[..., 3]
    want_a = ref["g_alpha"].astype(np.float32)
    tol = 2.0 ** -22 * np.abs(want_a) + 2.0 ** -23 * np.abs(old[..., 3])  # the addition's own rounding at [0, 0]
    assert np.all(np.abs(g_alpha - want_a) <= tol), what
    assert np.array_equal(gi[..., 3][~ref["valid"]], old[..., 3][~ref["valid"]])
    assert np.array_equal(gi[..., :3].view(np.uint32), old[..., :3].view(np.uint32))
    return ref, loss, gd, gi


@pytest.mark.parametrize("weights", ["none", "random", "zero"])
@pytest.mark.parametrize("kind", ["l1", "inverse"])
@pytest.mark.parametrize("size", SIZES)
def test_loss_and_gradients_match_the_reference(cuda, size, kind, weights):
    h, w = size
    depth, image, t, wt = inputs(h, w, weights)
    for scale in (1.0, 0.37):
        ref, loss, gd, _ = check(cuda, depth, image, t, wt, kind, scale, what=f"{h} x {w} {kind} {weights} scale {scale}")
        if weights == "zero":
            assert loss[0] == 0.0 and loss[1] == 0.0 and not gd.any()
        else:
            assert 0.3 * h * w < ref["valid"].sum() < h * w and ref["L"] > 0.01 and np.abs(gd).max() > 0


@pytest.mark.parametrize("kind", ["l1", "inverse"])
def test_planted_pixels(cuda, kind):
    h, w = 29, 37
    depth, image, t, wt = inputs(h, w, "random", seed=1)
    # a clean row to plant into: valid everywhere, weight 0.5
    depth[3, :, 0] = 2.0
    image[3, :, 3] = 0.8
    t[3, :] = 3.0
    wt[3, :] = 0.5
    ma = np.float32(MIN_ALPHA)
    image[3, 0, 3] = ma                                    # alpha exactly min_alpha: valid
    image[3, 1, 3] = np.nextafter(ma, np.float32(0.0))     # one f32 step below: invalid
    t[3, 2], t[3, 3], t[3, 4], t[3, 5] = 0.0, -1.0, np.nan, np.inf
    depth[3, 6, 0] = 0.0
    # e exactly 0: D / alpha = t and alpha / D = 1 / t in float64 (0.75 * 4 = 3, 0.25 = 0.75 / 3 = 1 / 4)
    image[3, 7, 3], depth[3, 7, 0], t[3, 7] = 0.75, 3.0, 4.0
    wt[3, 8], wt[3, 9], wt[3, 10] = np.nan, -1.0, 2.0
    ref, loss, gd, gi = check(cuda, depth, image, t, wt, kind, 1.0, what=f"planted {kind}")
    valid = ref["valid"]
    assert valid[3, 0] and gd[3, 0] != 0.0
    for x in (1, 2, 3, 4, 5, 6, 8, 9):
        assert not valid[3, x] and gd[3, x] == 0.0 and gi[3, x, 3] == 0.0, x
    assert valid[3, 7] and ref["e"][3, 7] == 0.0 and gd[3, 7] == 0.0 and gi[3, 7, 3] == 0.0
    assert valid[3, 10] and valid[3, 11]
    # the weight 2 counts as 1: twice the gradient of its neighbour of weight 0.5
    assert gd[3, 10] == pytest.approx(2.0 * gd[3, 11], rel=1e-6) and gd[3, 11] != 0.0
    # W_v counts the e == 0 pixel and the clamped weight, and none of the invalid ones
    without = valid.copy()
    without[3, 7] = False
    clamped = np.where(wt > 0, np.minimum(wt, 1.0), 0.0).astype(np.float64)
    assert loss[1] == pytest.approx(clamped[valid].sum(), rel=1e-12)
    assert loss[1] - clamped[without].sum() == pytest.approx(0.5, rel=1e-9)


def test_runs_repeat_their_bits(cuda):
    from spz_amd import device as D
    h, w = 45, 70
    arrays = on_device(cuda, inputs(h, w, "random"))

    def once(stream=None):
        gi = torch.zeros((h, w, 4), device=cuda)
        loss, gd = D.depth_loss(arrays[0], arrays[1], arrays[2], weight=arrays[3], kind="inverse", scale=0.37,
                                grad_image=gi, stream=stream)
        if stream is not None:
            stream.synchronize()
        return [x.cpu().numpy().tobytes() for x in (loss, gd, gi)]

    first = once()
    assert once() == first
    assert once(torch.cuda.Stream(cuda)) == first
