"""The rasteriser (spz_render.hip, spz_render_backward.hip, spz_render_view_backward.hip; DESIGN §8 "Render") at the
sizes where its size-dependent branches leave their first arm, against the float64 references:

  tile-id sort    1, 2 and 3 radix digits (256, 289, 65,536 and 66,049 tiles), and the padding keys behind the last tile
  count scan      more than 256 runs of 1,024 depth-ordered Gaussians (270,000 visible Gaussians: 264 runs)
  blend batches   tile lists of up to ten batches of 256 entries in the five blend kernels (blend, score, depth, blend
                  backward, depth-blend backward); workgroups that leave with batches unstaged because every pixel has
                  stopped; waves that leave while other waves of their workgroup walk on
  view reduce     more than 64 rows of partial view gradients (n = 40,007: 157 rows, three rounds of the stride loop)

Every scene is built on the CPU by a function of this module (sort_view, scan_scene, deep_scene, reduce_scene) that
asserts, from the reference alone, the property that takes it down its path: the tile count, the run count, the list
lengths, the last used list position per tile, the row count.

The image rule (check_pixels): every pixel with no marginal pair within 1e-4 on every channel, a pixel with a marginal
pair (render_ref.walk: a pair within a relative 1e-4 of a decision threshold, which a float32 blend may decide the other
way) within 0.05: test_gpu_render.py's two numbers, here per pixel.  The share of marginal pixels is capped at 1 % per
scene and asserted from the reference.

Which records the reference blends.  At 4,096 pixels a float32 mean carries 2.4e-4 px per ulp, and test_gpu_render's
records check allows 1e-5 relative, 0.04 px there; a Gaussian of sigma 1 px changes by a few 1e-4 per 1e-4 px.  So the
sort views check the device's records against the reference's (check_records), and then compare the image with the
float64 blend of the records the device stored (their float32 values, their rectangles, their depth order); a pixel
counts as marginal when it is so under either set of records.  The scenes of 250 x 190 and 40 x 36 blend the
reference's own records, as the rest of the suite does.

The gradient rule is test_gpu_render_grad's, unchanged: per array |device - ref64| <= 8 max|ref32 - ref64|, ref32 being
the same reference in float32 with the same decisions (it makes the same long float32 sums over a list, so the bound
grows with the depth of the lists by itself); exact where that bound is 0; the scenes have no marginal pair.

What the deep scenes measure under that rule (MI355X; ratio of the worst error to max|ref32 - ref64|, bound 8; the
forward checks of every scene pass with errors below 1 % of their bounds):
  289 tiles   render_backward at most 0.05, render_depth_backward at most 0.04 (lists of at most 23 entries)
  thin        render_backward at most 2.0 (alphas), render_depth_backward at most 0.8 (records)
  wall        render_backward at most 3.1 (alphas), render_depth_backward at most 1.0 (positions)
  wall_aa     render_backward at most 2.3 (records), render_depth_backward at most 2.1 (scales)
  half_wall   render_backward at most 2.2 (alphas), render_depth_backward at most 0.7 (rotations)

What these scenes found.  The depth-blend backward took what lies behind a pair as D_final - D_i, two float32 sums of
up to 155 terms w z with z around 40 in a view whose depths span 23, so the difference kept few of their digits: under
the same rule it measured 3.5 (thin), 6.4 (wall, wall_aa) and 10.5 (half_wall, positions: the x gradient of one Gaussian
with 127 pixel terms, off by 6.8e-5 of -2.44), the last above the bound, where test_gpu_depth_backward's scenes (at most 84 used
pairs per pixel) stay below it.  It was rounding, not a wrong walk: the same Gaussian was the worst of the scenes where
no wave leaves early, and a skipped or repeated batch is off by the order of the values.  The kernel now sums
w (z - z0), z0 the depth of the tile's first entry (spz_render_backward.hip; DESIGN §8 "Depth fit"): the same
derivative without the cancellation, and the figures above are its.  ref32 itself is no strict float32 walk (torch's
float32 scans on the CPU keep their running value in double, and its sums are blocked by thread count, so it moves by
some 40 % between hosts); the margins above leave room for that."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
import depth_ref as DR
import prune_ref as PR
import render_grad_ref as GR
import render_ref as RR
import view_grad_ref as VR
from test_gpu_depth import check_maps
from test_gpu_prune import check_scores
from test_gpu_render import check_records, view_of
from test_gpu_render_grad import ARRAYS

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)
BATCH = 256       # kBlendThreads: the entries a workgroup stages at a time
SCAN_ITEMS = 1024  # kScanItems: the depth-ordered Gaussians per run of the count scan
VIEW_ROWS = 256    # kViewBlock: the Gaussians per row of partial view gradients


# ---- scenes placed by inverse projection under an identity camera ---------------------------------------------------

def identity_view(width, height, max_sh=3):
    """(params, cam): the camera at the origin looking down +z, focal length 0.9 height, the principal point a little
    off the middle."""
    from spz_amd import abi
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    f, cx, cy = 0.9 * height, 0.5 * width + 3.25, 0.5 * height - 2.5
    return (abi.render_params(m, f, f, cx, cy, width, height, 0.2, BG, max_sh, 0),
            RR.camera(m, f, f, cx, cy, width, height, 0.2, BG, max_sh))


def unproject(cam, u, v, z):
    """The points that project to the pixel centres (u, v) at depth z: p = ((u + 0.5 - cx) z / fx, (v + 0.5 - cy) z / fy,
    z), as (n, 3) float64."""
    return np.stack([(u + 0.5 - cam["cx"]) * z / cam["fx"], (v + 0.5 - cam["cy"]) * z / cam["fy"], z], axis=1)


def placed_cloud(rng, cam, tile_ids, per_tile, deg):
    """per_tile Gaussians in each tile of tile_ids: means uniform over the tile, depths uniform in [4, 12] (so the tiles'
    lists interleave in the depth order), 2D sizes of sigma 1 to 3.3 px (8 to 22 px across at 3 sigma, so many reach
    into a neighbouring tile), opacities 0.27 to 0.92."""
    tw, _ = RR.tiles(cam)
    t = np.repeat(np.asarray(tile_ids, dtype=np.int64), per_tile)
    n = t.size
    u = np.minimum(16.0 * (t % tw) + rng.uniform(0.0, 15.0, n), cam["width"] - 1.0)
    v = np.minimum(16.0 * (t // tw) + rng.uniform(0.0, 15.0, n), cam["height"] - 1.0)
    z = rng.uniform(4.0, 12.0, n)
    sigma = rng.uniform(1.0, 3.3, n) * z / cam["fx"]
    q = rng.standard_normal((n, 4))
    return {"positions": unproject(cam, u, v, z).astype(np.float32).reshape(-1),
            "scales": (np.log(sigma)[:, None] + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32).reshape(-1),
            "rotations": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32).reshape(-1),
            "alphas": rng.uniform(-1.0, 2.5, n).astype(np.float32),
            "colors": rng.uniform(-1.5, 1.5, 3 * n).astype(np.float32),
            "sh": (0.3 * rng.standard_normal(n * RR.SH_DIM[deg] * 3)).astype(np.float32)}


# name: width = height, the populated tiles, Gaussians per tile, degree, seed
def _tiles_256(tw):
    return np.arange(256)


def _tiles_289(tw):
    return np.arange(289)


def _tiles_65536(tw):
    rng = np.random.default_rng(65536)
    return np.unique(np.concatenate([[0, 255, 256, 65279, 65280, 65534, 65535], rng.integers(0, 65536, 300)]))


def _tiles_66049(tw):
    rng = np.random.default_rng(66049)
    rows = np.concatenate([r * tw + np.arange(tw) for r in (0, 1, 254, 255, 256)])
    return np.unique(np.concatenate([rows, rng.integers(0, 66049, 300)]))


SORT_VIEWS = {"256_tiles": (256, _tiles_256, 3, 0, 1), "289_tiles": (272, _tiles_289, 3, 1, 268),
              "65536_tiles": (4096, _tiles_65536, 3, 0, 3), "66049_tiles": (4112, _tiles_66049, 2, 0, 4)}
SORT_DIGITS = {"256_tiles": 1, "289_tiles": 2, "65536_tiles": 2, "66049_tiles": 3}


@functools.lru_cache(maxsize=None)
def sort_view(name):
    """The view's cloud, camera and reference records, with what takes it down its arm of the tile-id sort."""
    size, tiles_of, per_tile, deg, seed = SORT_VIEWS[name]
    params, cam = identity_view(size, size)
    tw, th = RR.tiles(cam)
    ids = tiles_of(tw)
    cloud = placed_cloud(np.random.default_rng(seed), cam, ids, per_tile, deg)
    rec = RR.preprocess(cloud, deg, cam)
    lists = RR.tile_lists(rec, cam)
    n_tiles = tw * th
    digits = 1 if n_tiles <= 256 else (2 if n_tiles <= 65536 else 3)
    assert n_tiles == int(name.split("_")[0]) and digits == SORT_DIGITS[name]
    assert rec["visible"].all() and set(ids.tolist()) <= set(lists)
    assert all(len(lists[int(t)]) >= 2 for t in ids), "every populated tile has several Gaussians"
    assert n_tiles - 1 in lists, "the last tile has a list: its id is the padding keys' low digits"
    if digits >= 2:  # tiles that a sort of one digit fewer would merge
        step = 256 if digits == 2 else 65536
        pairs = [t for t in lists if t + step in lists]
        assert len(pairs) >= (33 if name == "289_tiles" else 1), pairs
    if name == "289_tiles":
        assert len(lists) == 289, "every tile is touched"
    if name == "66049_tiles":
        assert sum(1 for t in lists if t >= 65536) >= 500 and sum(1 for t in lists if t < 512) >= 500
    home = np.repeat(ids, per_tile)[RR.depth_order(rec)]  # the Gaussians' own tiles along the depth order
    assert (np.diff(home) < 0).mean() > 0.3, "the tiles' lists interleave in the depth order"
    return {"cloud": cloud, "n": cloud["alphas"].size, "deg": deg, "params": params, "cam": cam, "rec": rec,
            "lists": lists, "tiles": n_tiles, "entries": RR.entry_count(rec)}


def device_records(rec_t):
    """The records the device stored, as a render_ref record dict: the float32 values, the rectangles, visibility."""
    r = {k: rec_t[k].cpu().numpy() for k in ("mean", "conic", "opacity", "rgb", "depth")}
    r["rect"] = rec_t["rect"].cpu().numpy().astype(np.int64)
    r["visible"] = np.isfinite(r["depth"])
    return r


def check_pixels(got, want, marginal, what):
    """The module's image rule over arrays of pixels (..., channels) and their marginal mask (...).  Returns the worst
    errors of the two classes as fractions of their bounds."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max(axis=-1)
    clean = ~marginal
    worst = float(err[clean].max()) if clean.any() else 0.0
    worst_m = float(err[marginal].max()) if marginal.any() else 0.0
    print(f"{what}: worst pixel without a marginal pair {worst:.3e} ({worst / 1e-4:.3f} of 1e-4), with one "
          f"{worst_m:.3e} ({worst_m / 0.05:.3f} of 0.05); {marginal.sum()} of {marginal.size} pixels marginal")
    assert worst <= 1e-4, f"{what}: a pixel without a marginal pair is off by {worst}"
    assert worst_m <= 0.05, f"{what}: a marginal pixel is off by {worst_m}"
    return worst / 1e-4, worst_m / 0.05


def check_sorted_view(s, img, rec_t, what):
    """img (device, h x w x 4) against the float64 blend of the device's records over the touched tiles; every other
    tile must be the background, compared on the device: only the touched tiles are copied to the host."""
    cam = s["cam"]
    tw, th = RR.tiles(cam)
    rec = device_records(rec_t)
    ids = sorted(RR.tile_lists(rec, cam))
    marg_dev, marg_ref = {}, {}
    want = RR.render_tiles(rec, cam, ids, marginal=marg_dev)
    RR.render_tiles(s["rec"], cam, ids, marginal=marg_ref)
    share = sum(int((m > 0).sum()) for m in marg_ref.values()) / (256.0 * len(ids))
    assert share <= 0.01, f"{what}: {share:.4f} of the touched pixels are marginal in the reference"
    assert cam["width"] % 16 == 0 and cam["height"] % 16 == 0
    by_tile = img.view(th, 16, tw, 16, 4).permute(0, 2, 1, 3, 4)
    touched = torch.zeros(th * tw, dtype=torch.bool, device=img.device)
    touched[torch.as_tensor(ids, device=img.device)] = True
    touched = touched.view(th, tw)
    got = by_tile[touched].cpu().numpy()  # in tile-id order, as ids
    bg = torch.tensor(list(np.float32(BG)) + [0.0], dtype=torch.float32, device=img.device)
    assert bool((by_tile[~touched] == bg).all()), f"{what}: an untouched tile is not the background"
    want = np.stack([want[t] for t in ids])
    marginal = np.stack([(marg_dev[t] > 0) | (marg_ref[t] > 0) for t in ids])
    print(f"{what}: {len(ids)} touched tiles of {tw * th}, marginal share {share:.5f}")
    return check_pixels(got, want, marginal, what)


def test_one_digit_and_padding_keys_behind_tile_255(cuda):
    """256 tiles: one digit.  With max_entries above the total the padding keys' only sorted digit, 0xff, is tile 255's:
    only the sort's stability keeps them behind its entries."""
    from spz_amd import device as D
    s = sort_view("256_tiles")
    cloud = D.to_device(s["cloud"], cuda)
    rec_t = D.preprocess(cloud, s["n"], s["deg"], s["params"])
    check_records(rec_t, s["rec"])
    assert int(rec_t["total"].cpu()[0]) == s["entries"]
    img, total, status = D.render(cloud, s["n"], s["deg"], s["params"], return_info=True)
    assert int(total.cpu()[0]) == s["entries"] and int(status.cpu()[0]) == 0
    check_sorted_view(s, img, rec_t, "256 tiles")
    padded, _, status = D.render(cloud, s["n"], s["deg"], s["params"], max_entries=s["entries"] + 1000, return_info=True)
    assert int(status.cpu()[0]) == 0
    assert torch.equal(padded.view(torch.int32), img.view(torch.int32)), "the padded workspace renders other bits"


@functools.lru_cache(maxsize=None)
def gradient_reference(kind, name):
    """A scene's decisions, image gradients and float64 / float32 reference gradients of the image (and of the image and
    the accumulated depth under "depth"): computed once and shared."""
    s = sort_view(name) if kind == "sort" else deep_scene(name)
    cloud, deg, cam, aa = s["cloud"], s["deg"], s["cam"], s.get("aa", False)
    dec = s["dec"] if "dec" in s else GR.decisions(cloud, deg, cam, aa, vectorised=True)
    assert dec["marginal"] == 0, "choose another seed: the reference counts marginal pairs"
    assert dec["visible"].all()
    H, W = cam["height"], cam["width"]
    rng = np.random.default_rng(100 + len(name))
    G = rng.standard_normal((H, W, 4)).astype(np.float32)
    GD = rng.standard_normal((H, W)).astype(np.float32)
    ref = {"dec": dec, "G": G, "GD": GD}
    ref["colour"] = {"g64": GR.gradients(cloud, deg, cam, dec, G, aa, torch.float64),
                     "g32": GR.gradients(cloud, deg, cam, dec, G, aa, torch.float32)}
    ref["depth"] = {"g64": DG.gradients(cloud, deg, cam, dec, G, GD, aa, torch.float64),
                    "g32": DG.gradients(cloud, deg, cam, dec, G, GD, aa, torch.float32)}
    return ref


def check_gradients(got, ref, what, keys):
    """test_gpu_render_grad.check_gradients' rule over `keys`; returns the worst ratio of an error to its bound."""
    worst = 0.0
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
            worst = max(worst, err / bound)
    return worst


def check_accumulated(got, want, marginal, span, what):
    """The image rule for the accumulated depth, scaled as test_gpu_depth scales it: a pixel with no marginal pair
    within 1e-4 max(1, |D|), a marginal one within 5 % of the scene's depth range."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    rel = err / np.maximum(1.0, np.abs(want))
    worst = float(rel[~marginal].max()) if (~marginal).any() else 0.0
    worst_m = float(err[marginal].max()) if marginal.any() else 0.0
    print(f"{what}: worst pixel without a marginal pair {worst:.3e} of max(1, |D|) ({worst / 1e-4:.3f} of 1e-4), with "
          f"one {worst_m:.3e} ({worst_m / (0.05 * span):.3f} of 5 % of the depth range {span:.3g})")
    assert worst <= 1e-4 and worst_m <= 0.05 * span


def check_five_kernels(cuda, s, ref, what, forward_rec=None):
    """Render, depth, score, render backward and depth backward of the scene s against their references; no pixel is
    marginal.  The forward references blend the reference's own records, or forward_rec (the device's records as a
    render_ref dict, from a caller that has compared the image itself: see the module's docstring)."""
    from spz_amd import device as D
    cloud_np, n, deg, p, cam, aa = s["cloud"], s["n"], s["deg"], s["params"], s["cam"], s.get("aa", False)
    dec = ref["dec"]
    rec = dec["rec"]
    cloud = D.to_device(cloud_np, cuda)
    rec_t = D.preprocess(cloud, n, deg, p, antialiased=aa)
    check_records(rec_t, rec)
    assert int(rec_t["total"].cpu()[0]) == dec["entries"]
    none = np.zeros((cam["height"], cam["width"]), dtype=bool)
    if forward_rec is None:
        # render: the float64 autograd forward is render_ref's image (test_render_grad_host)
        img = D.render(cloud, n, deg, p, antialiased=aa)
        check_pixels(img.cpu().numpy(), ref["colour"]["g64"]["image"], none, f"{what} image")
    else:
        rec = forward_rec
    # depth: every pixel's accumulated depth within 1e-4 max(1, |D|), and test_gpu_depth's rules for the median
    depth, index = D.render_depth(cloud, n, deg, p, antialiased=aa)
    want = DR.render_depth(cloud_np, deg, cam, aa, rec=rec)
    span = float(dec["rec"]["depth"].max() - dec["rec"]["depth"].min())
    check_accumulated(depth[..., 0].cpu().numpy(), want["accumulated"], none, span, f"{what} accumulated depth")
    check_maps(depth.cpu().numpy(), index.cpu().numpy(), want, rec_t["depth"].cpu().numpy())
    # score: test_gpu_prune's bounds
    wsum, wmax = D.score(cloud, n, deg, [p], antialiased=aa)
    want_sum, want_max, _ = PR.view_scores(cloud_np, deg, cam, aa, rec=rec)
    check_scores(wsum.cpu().numpy(), wmax.cpu().numpy(), want_sum, want_max)
    # the two backward kernels
    G, GD = torch.as_tensor(ref["G"]).to(cuda), torch.as_tensor(ref["GD"]).to(cuda)
    got = D.render_backward(cloud, n, deg, p, G, antialiased=aa, return_record_grads=True)
    a = check_gradients(got, ref["colour"], f"{what} render_backward", ARRAYS + ("records",))
    got = D.render_depth_backward(cloud, n, deg, p, G, GD, antialiased=aa, return_record_grads=True)
    b = check_gradients(got, ref["depth"], f"{what} render_depth_backward", ARRAYS + ("records", "depth"))
    print(f"{what}: worst gradient error {max(a, b):.3f} of its bound")


def test_two_digits_at_289_tiles_through_all_five_blend_kernels(cuda):
    """289 tiles: two digits, every tile touched, so each tile t < 33 has a partner t + 256 that one digit would merge
    with it.  The view is small enough to run everything that reads the sorted entries."""
    from spz_amd import device as D
    s = sort_view("289_tiles")
    cloud = D.to_device(s["cloud"], cuda)
    rec_t = D.preprocess(cloud, s["n"], s["deg"], s["params"])
    img, total, status = D.render(cloud, s["n"], s["deg"], s["params"], return_info=True)
    assert int(total.cpu()[0]) == s["entries"] and int(status.cpu()[0]) == 0
    check_sorted_view(s, img, rec_t, "289 tiles")
    check_five_kernels(cuda, s, gradient_reference("sort", "289_tiles"), "289 tiles", forward_rec=device_records(rec_t))


@pytest.mark.parametrize("name", ["65536_tiles", "66049_tiles"])
def test_two_and_three_digits_at_sixty_five_thousand_tiles(cuda, name):
    """65,536 tiles: still two digits, and with max_entries above the total the padding keys' low 16 bits are the last
    tile's.  66,049 tiles: three digits (the third pass writes over the first one's key plane), with tiles t and
    t + 65,536 that two digits would merge.  The image is 270 MB: it is freed before the next test."""
    from spz_amd import device as D
    s = sort_view(name)
    cloud = D.to_device(s["cloud"], cuda)
    rec_t = D.preprocess(cloud, s["n"], s["deg"], s["params"])
    check_records(rec_t, s["rec"])
    assert int(rec_t["total"].cpu()[0]) == s["entries"]
    img, total, status = D.render(cloud, s["n"], s["deg"], s["params"], max_entries=s["entries"] + 1000,
                                  return_info=True)
    try:
        assert int(total.cpu()[0]) == s["entries"] and int(status.cpu()[0]) == 0
        check_sorted_view(s, img, rec_t, name.replace("_", " "))
    finally:
        del img
        torch.cuda.empty_cache()


# ---- the count scan past 256 runs, and lists of several batches -----------------------------------------------------

def thin_cloud(rng, cam, n):
    """n degree-0 Gaussians by inverse projection: means uniform over the image, depths uniform in [4, 12], log scales in
    [-6, -5] (the 2D footprint is the 0.3 px blur: mostly one tile), alphas uniform in [-5, -3.5] (opacity 0.007 to 0.03:
    no pixel stops)."""
    u, v = rng.uniform(0.0, cam["width"] - 1.0, n), rng.uniform(0.0, cam["height"] - 1.0, n)
    z = rng.uniform(4.0, 12.0, n)
    return {"positions": unproject(cam, u, v, z).astype(np.float32).reshape(-1),
            "scales": rng.uniform(-6.0, -5.0, 3 * n).astype(np.float32),
            "rotations": np.tile(np.float32([0, 0, 0, 1]), n),
            "alphas": rng.uniform(-5.0, -3.5, n).astype(np.float32),
            "colors": rng.uniform(-1.5, 1.5, 3 * n).astype(np.float32), "sh": np.zeros(0, np.float32)}


@functools.lru_cache(maxsize=None)
def scan_scene():
    """270,000 visible Gaussians at 250 x 190: 264 runs of the count scan, so its one workgroup scans two runs per
    thread (per = 2), and tile lists of four to eleven batches.  With the float64 references of the image, the
    accumulated depth and the scores, walked once per tile (render_ref.walk)."""
    n = 270000
    params, cam = identity_view(250, 190)
    cloud = thin_cloud(np.random.default_rng(3), cam, n)
    rec = RR.preprocess(cloud, 0, cam)
    runs = (n + SCAN_ITEMS - 1) // SCAN_ITEMS
    assert rec["visible"].all() and runs == 264 > 256, "only visible Gaussians reach the late runs"
    lists = RR.tile_lists(rec, cam)
    lengths = np.array([len(lists[t]) for t in sorted(lists)])
    assert len(lists) == 16 * 12 and lengths.min() > 3 * BATCH and lengths.max() > 8 * BATCH, (lengths.min(), lengths.max())
    H, W = cam["height"], cam["width"]
    image, acc = np.zeros((H, W, 4)), np.zeros((H, W))
    marginal, last_batch = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    wsum, wmax = np.zeros(n), np.zeros(n)

    def one_tile(t):
        sel = lists[t]
        vv, uu = RR.tile_pixels(cam, t)
        wk = RR.walk(rec, sel, uu, vv)
        C, T = RR._colours(rec, sel, wk, uu.shape)
        image[vv, uu, :3] = C + T[..., None] * cam["background"]
        image[vv, uu, 3] = 1.0 - T
        acc[vv, uu] = (wk["w"] * rec["depth"][sel].astype(np.float64)[:, None]).sum(axis=0).reshape(uu.shape)
        marginal[vv, uu] = (wk["marginal"] > 0).reshape(uu.shape)
        last_batch[vv, uu] = (wk["last"] >= (len(sel) - 1) // BATCH * BATCH).reshape(uu.shape)
        assert not wk["stopped"].any()
        return sel, wk["w"].sum(axis=1), wk["w"].max(axis=1), float(T.min())

    t_min = 1.0
    with ThreadPoolExecutor(8) as pool:  # numpy releases the lock inside its loops; the tiles write disjoint pixels
        for sel, s_sum, s_max, t_tile in pool.map(one_tile, sorted(lists)):
            wsum[sel] += s_sum  # a Gaussian is once in a tile's list
            wmax[sel] = np.maximum(wmax[sel], s_max)
            t_min = min(t_min, t_tile)
    assert t_min > 0.5, "no pixel is near the stop, so every workgroup walks every batch"
    assert last_batch.mean() > 0.5, "most pixels use an entry of their tile's last batch"
    share = float(marginal.mean())
    assert share <= 0.01, f"{share:.4f} of the pixels are marginal"
    return {"cloud": cloud, "n": n, "params": params, "cam": cam, "rec": rec, "entries": RR.entry_count(rec),
            "image": image, "accumulated": acc, "marginal": marginal, "wsum": wsum, "wmax": wmax, "runs": runs,
            "lengths": lengths, "share": share}


def test_count_scan_over_264_runs_and_lists_of_up_to_eleven_batches(cuda):
    """A wrong run offset misplaces whole runs of entries across all tiles; the image, the accumulated depth (of
    which the expected depth is the quotient by the image's alpha) and the scores then show it differently."""
    from spz_amd import device as D
    s = scan_scene()
    n, p = s["n"], s["params"]
    cloud = D.to_device(s["cloud"], cuda)
    rec_t = D.preprocess(cloud, n, 0, p)
    check_records(rec_t, s["rec"])
    assert int(rec_t["total"].cpu()[0]) == s["entries"]
    img, total, status = D.render(cloud, n, 0, p, return_info=True)
    assert int(total.cpu()[0]) == s["entries"] and int(status.cpu()[0]) == 0
    print(f"{s['runs']} runs, {s['entries']} entries, lists of {s['lengths'].min()} to {s['lengths'].max()}, marginal "
          f"share {s['share']:.5f}")
    check_pixels(img.cpu().numpy(), s["image"], s["marginal"], "270,000 Gaussians image")
    depth, index, dimg = D.render_depth(cloud, n, 0, p, return_image=True)
    assert torch.equal(dimg.view(torch.int32), img.view(torch.int32)), "the depth kernel's image is not the render's"
    span = float(s["rec"]["depth"].max() - s["rec"]["depth"].min())
    check_accumulated(depth[..., 0].cpu().numpy(), s["accumulated"], s["marginal"], span, "270,000 Gaussians depth")
    assert bool((index == -1).all()) and bool(torch.isposinf(depth[..., 1]).all()), "no pixel of this scene has a median"
    wsum, wmax = D.score(cloud, n, 0, [p])
    check_scores(wsum.cpu().numpy(), wmax.cpu().numpy(), s["wsum"], s["wmax"])


# ---- deep lists and early exits in the five blend kernels -----------------------------------------------------------

DEEP_W, DEEP_H = 40, 36
# name: seed of the crowd, variant, antialiased, seed of the wall's jitter.  Chosen on the CPU among crowd seeds 0 to 79
# and jitter seeds 0 to 7 as the first whose reference counts no marginal pair (a scene of 3,000 entries has three or
# four on average) and at most 0.5 % of the pixels within 1e-4 of the median threshold.
DEEP_CASES = {"thin": (27, "thin", False, 0), "wall": (27, "wall", False, 0), "half_wall": (27, "half", False, 2),
              "wall_aa": (1, "wall", True, 2)}


def deep_cloud(seed, variant, jitter):
    """render_grad_ref.scene(seed, 1, n=900) with alphas - 3 (opacity about 0.1: the thin crowd), and its view.  "wall":
    plus 12 Gaussians at the view's target, in the middle of the crowd's depths, with log scale ln(2 ext) and alpha +4:
    every pixel stops there.  "half": the 12 instead 0.83 ext wide and 0.2 ext high, 4.5 px below the target: they stop
    the upper rows of the centre tile only.  The view is the crowd's alone."""
    c = GR.scene(seed, 1, n=900)
    c["alphas"] = (c["alphas"] - 3.0).astype(np.float32)
    m, fx, fy, cx, cy = view_of(c["positions"], width=DEEP_W, height=DEEP_H)
    if variant != "thin":
        p = c["positions"].reshape(-1, 3).astype(np.float64)
        lo, hi = np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)
        target, ext = 0.5 * (lo + hi), float(max(hi - lo))
        rng = np.random.default_rng(5000 + jitter)
        k = 12
        if variant == "wall":
            at = target[None, :] + 0.01 * ext * rng.standard_normal((k, 3))
            scales = np.full((k, 3), np.log(2.0 * ext))
            alpha = 4.0
        else:
            up = m[1, :3].astype(np.float64)  # the image's +v direction in the world
            per_px = np.linalg.norm(m[:, :3] @ target + m[:, 3]) / fy
            at = target[None, :] + 4.5 * per_px * up[None, :] + 0.01 * ext * rng.standard_normal((k, 3))
            scales = np.log(np.tile([0.83 * ext, 0.2 * ext, 0.05 * ext], (k, 1)))
            alpha = 4.0
        e = GR.scene(seed + 1000, 1, n=k)
        e["positions"] = at.astype(np.float32).reshape(-1)
        e["scales"] = scales.astype(np.float32).reshape(-1)
        e["rotations"] = np.tile(np.float32([0, 0, 0, 1]), k)
        e["alphas"] = np.full(k, alpha, np.float32)
        c = {key: np.concatenate([c[key], e[key]]) for key in c}
    return c, (m, fx, fy, cx, cy)


def batch_facts(dec):
    """Per tile of the decisions: the list length, the last used list position of any pixel, and per band of four pixel
    rows (one wave of the workgroup) whether every pixel stopped and the last used position in the band."""
    out = []
    for tile in dec["tiles"]:
        L = len(tile["sel"])
        take = tile["take"]  # (pixels, L)
        used = take.any(axis=1)
        last = np.where(used, L - 1 - np.argmax(take[:, ::-1], axis=1), -1) if L else np.full(take.shape[0], -1)
        rows = tile["v"] - tile["v"].min()
        bands = []
        for b in range(4):
            sel = rows // 4 == b
            if sel.any():
                bands.append({"pixels": int(sel.sum()), "last": int(last[sel].max())})
        out.append({"length": L, "last": int(last.max()), "bands": bands})
    return out


@functools.lru_cache(maxsize=None)
def deep_scene(name):
    """The case's cloud, view and decisions, with the facts about its batches asserted from the reference."""
    from spz_amd import abi
    seed, variant, aa, jitter = DEEP_CASES[name]
    cloud, (m, fx, fy, cx, cy) = deep_cloud(seed, variant, jitter)
    params = abi.render_params(m, fx, fy, cx, cy, DEEP_W, DEEP_H, 0.2, BG, 3, 0)
    cam = RR.camera(m, fx, fy, cx, cy, DEEP_W, DEEP_H, 0.2, BG, 3)
    dec = GR.decisions(cloud, 1, cam, aa, vectorised=True)
    assert dec["visible"].all()
    gap = DR.render_depth(cloud, 1, cam, aa, rec=dec["rec"])["gap"]
    assert (gap < 1e-4).mean() <= 0.005, "choose another seed: test_gpu_depth's cap on pixels at the median threshold"
    stopped = stopped_pixels(dec)
    facts = batch_facts(dec)
    deepest = max(facts, key=lambda f: f["length"])
    assert deepest["length"] > 3 * BATCH, "the deepest tile takes four batches"
    if variant == "thin":
        # every batch is walked and the last one is partial
        assert deepest["length"] % BATCH != 0 and deepest["last"] >= deepest["length"] // BATCH * BATCH
        assert sum(f["length"] > BATCH and f["last"] >= (f["length"] - 1) // BATCH * BATCH for f in facts) >= 4
    elif variant == "wall":
        # every pixel stops, and some workgroup leaves with at least one whole batch unstaged
        assert stopped.all()
        early = [f for f in facts if f["last"] < 2 * BATCH <= f["length"] - BATCH]
        assert early, [(f["length"], f["last"]) for f in facts]
    else:
        # in one workgroup a whole band (wave) has stopped before the last batch and another band walks into it
        split = []
        for tile, f in zip(dec["tiles"], facts):
            first_of_last = (f["length"] - 1) // BATCH * BATCH
            rows = (tile["v"] - tile["v"].min()) // 4
            gone = [b for b in range(4) if (rows == b).any() and stopped[tile["v"], tile["u"]][rows == b].all()
                    and f["bands"][b]["last"] < first_of_last]
            on = [b for b in range(4) if (rows == b).any() and f["bands"][b]["last"] >= first_of_last]
            if f["length"] > BATCH and gone and on:
                split.append((f["length"], gone, on))
        assert split, "no tile has a stopped band beside a band that reaches the last batch"
        assert not stopped.all()
    return {"cloud": cloud, "n": cloud["alphas"].size, "deg": 1, "aa": aa, "params": params, "cam": cam, "dec": dec,
            "facts": facts}


def stopped_pixels(dec):
    """(H, W) bool: the pixels that reached the stop, from the decisions: a pixel stops at the first pair it considers
    but does not use although it passes the alpha test, which is where T would fall below 1e-4."""
    rec = dec["rec"]
    H = max(int(t["v"].max()) for t in dec["tiles"]) + 1
    W = max(int(t["u"].max()) for t in dec["tiles"]) + 1
    out = np.zeros((H, W), dtype=bool)
    for t in dec["tiles"]:
        wk = RR.walk(rec, t["sel"], t["u"], t["v"])
        assert np.array_equal(wk["take"].T, t["take"])
        out[t["v"], t["u"]] = wk["stopped"]
    return out


@pytest.mark.parametrize("name", list(DEEP_CASES))
def test_deep_lists_and_early_exits_in_the_five_blend_kernels(cuda, name):
    """thin: every batch of a four-batch list is walked, the last one partial.  wall: every pixel stops and a workgroup
    leaves with a whole batch unstaged, in the forward kernels and in both walks of the backward ones.  half_wall:
    waves of a workgroup leave while others walk on to the last batch.  wall_aa: the wall antialiased.
    The module's docstring has the measured ratios, and what the depth-blend backward measured before it summed
    w (z - z0)."""
    s = deep_scene(name)
    print(f"{name}: lists {[f['length'] for f in s['facts']]}, last used {[f['last'] for f in s['facts']]}, "
          f"{s['dec']['stopped']} pixels stop")
    check_five_kernels(cuda, s, gradient_reference("deep", name), name)


# ---- the view-gradient reduce past 64 rows --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reduce_scene():
    """40,007 thin Gaussians (thin_cloud) at 40 x 36: 157 rows of partial view gradients, which the reduce's 64 groups
    of lanes take in three rounds (the third partial), and random record gradients."""
    n = 40007
    params, cam = identity_view(DEEP_W, DEEP_H)
    cloud = thin_cloud(np.random.default_rng(4), cam, n)
    rec = RR.preprocess(cloud, 0, cam)
    rows = (n + VIEW_ROWS - 1) // VIEW_ROWS
    assert rows == 157 and 2 * 64 < rows < 3 * 64 and n % VIEW_ROWS != 0
    assert rec["visible"].all()
    rg = np.random.default_rng(40007).standard_normal((n, 9)).astype(np.float32)
    per = VR.chain(cloud, 0, cam, {"visible": rec["visible"]}, rg, forward_mode=True)
    return {"cloud": cloud, "n": n, "params": params, "rg": rg, "want": per.sum(axis=0),
            "mag": np.abs(per).sum(axis=0)}


def test_view_gradient_reduce_over_157_rows(cuda):
    """test_gpu_locate.test_chain_and_sum_from_given_record_gradients at n = 40,007, with its tolerance rule: both sides
    run the chain in f64 on the same f32 record gradients, and the orders of the 40,007 terms differ by at most
    40,007 * 2^-53 = 4.4e-12 of sum |contribution|, so its 1e-10 still leaves the rest for exp and sqrt."""
    from spz_amd import device as D
    s = reduce_scene()
    cloud = D.to_device(s["cloud"], cuda)
    rg_t = torch.as_tensor(s["rg"]).to(cuda)
    got = [D.render_view_backward(cloud, s["n"], 0, s["params"], None, record_grads=rg_t).cpu().numpy()
           for _ in range(2)]
    assert got[0].shape == (3, 4) and got[0].dtype == np.float64
    assert (s["mag"] > 0).all()
    err = np.abs(got[0] - s["want"]) / s["mag"]
    print(f"157 rows: |device - ref| / sum|contribution| at most {err.max():.3e} ({err.max() / 1e-10:.3f} of 1e-10)")
    assert np.all(np.abs(got[0] - s["want"]) <= 1e-10 * s["mag"])
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
