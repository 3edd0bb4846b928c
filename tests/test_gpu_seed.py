"""spz_amd_seed_view_device / spz_amd_seed_open, spz_amd.device.seed_view + seed, spz.seed_spz and spz_seed
(include/spz_amd.h "seed"; DESIGN §8 "Seed") on the GPU against the numpy restatement of tests/seed_ref.py.  The contract
fixes every operation's order and precision, so flags, counts, positions, rotations, alphas, colours and sh are compared
bit for bit; the log scales alone may differ by one float32 step (two f64 `log` implementations, each good to under one
f64 ulp, can round to neighbouring floats)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import render_ref as RR
import seed_ref as SR
from conftest import ROOT
from seed_ref import write_pfm, write_views

pytestmark = pytest.mark.gpu

W, H, F = 64, 48, 60.0
STRIDES = (1, 2, 3)       # 3 divides neither side; 64 x 48 at stride 1 is 12 blocks of 256 samples


@pytest.fixture(scope="module")
def D(cuda):
    from spz_amd import device
    return device


def u32(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def params(m, near=0.2, coord=0, width=W, height=H):
    from spz_amd import abi
    return abi.render_params(m, F, F, 0.5 * width, 0.5 * height, width, height, near, coord=coord)


def ref_view(p):
    return SR.view(np.array(list(p.world_to_camera), np.float32).reshape(3, 4), p.fx, p.fy, p.cx, p.cy, p.width, p.height,
                   p.near_plane)


def assert_cloud_equal(got, want, n, sh_degree, what=""):
    """The first n Gaussians of two clouds under the rule of the module's docstring; returns the number of log scales
    that differ (by one step)."""
    per = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3, "sh": 3 * SR.SH_DIM[sh_degree]}
    for k in ("positions", "rotations", "alphas", "colors", "sh"):
        a, b = u32(got[k])[: n * per[k]], u32(want[k])[: n * per[k]]
        assert a.shape == b.shape and np.array_equal(a, b), f"{what} {k}: {(a != b).sum()} of {a.size} values differ"
    a = (got["scales"].cpu().numpy() if hasattr(got["scales"], "cpu") else got["scales"])[: 3 * n]
    b = want["scales"][: 3 * n]
    dist = SR.ulp_distance(a, b)
    differ = int((dist != 0).sum())
    assert dist.size == 3 * n and (dist <= 1).all(), \
        f"{what} scales: {differ} of {dist.size} log scales differ, the largest by {int(dist.max())} float32 steps"
    return differ


def upload(cloud, cuda):
    import torch
    return {k: torch.from_numpy(v.copy()).to(cuda) for k, v in cloud.items()}


# ---- select and emit against hand-made maps --------------------------------------------------------------------------
def hand_made(seed, W=W, H=H):
    """A view with maps that reach every branch of the select."""
    rng = np.random.default_rng(seed)
    p = params(RR.look_at([0.3, -0.2, -2.5], [0.1, 0, 0], [0, 1, 0]), near=0.35, width=W, height=H)
    depth = rng.uniform(0.5, 4.0, size=(H, W)).astype(np.float32)
    for value, share in ((np.inf, 0.04), (np.nan, 0.03), (0.0, 0.03), (-1.5, 0.03), (0.2, 0.03), (0.35, 0.02)):
        depth[rng.random((H, W)) < share] = value                     # 0.2 < near, 0.35 == near: not > near
    weights = rng.uniform(0.0, 1.0, size=(H, W)).astype(np.float32)
    weights[rng.random((H, W)) < 0.05] = 0.5                          # exactly 0.5 does not count
    image = rng.uniform(-0.2, 1.3, size=(H, W, 4)).astype(np.float32)
    for value in (np.nan, np.inf):
        hit = rng.random((H, W, 3)) < 0.01
        image[..., :3][hit] = value
    alpha = rng.uniform(0.2, 1.0, size=(H, W)).astype(np.float32)     # some below cover_alpha = 0.5
    alpha[rng.random((H, W)) < 0.06] = 0.0                            # acc / 0: an infinite expected depth
    ratio = rng.uniform(0.9, 1.1, size=(H, W)).astype(np.float32)     # both sides of the 5 % tolerance
    valid_depth = np.where(np.isfinite(depth), depth, np.float32(1.0))
    cover_depth = np.zeros((H, W, 2), np.float32)
    cover_depth[..., 0] = valid_depth * ratio * alpha
    cover_depth[..., 0][alpha == 0] = 1.0
    cover_depth[..., 1] = np.inf
    cover_image = np.concatenate([rng.uniform(0, 1, size=(H, W, 3)).astype(np.float32), alpha[..., None]], axis=-1)
    return p, np.ascontiguousarray(image), depth, weights, np.ascontiguousarray(cover_image), cover_depth


def seed_view_raw(cuda, cloud_t, n, capacity, sh_degree, p, opts, image, depth, weights, cover_image, cover_depth):
    """spz_amd_seed_view_device with the caller's maps; returns (flags, counts)."""
    import ctypes as C

    import torch
    from spz_amd import abi, device
    L = abi.load_library()
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    ti, td, tw, tci, tcd = (t(a) for a in (image, depth, weights, cover_image, cover_depth))
    ptrs = device._seed_capacity_ptrs(cloud_t, capacity, sh_degree, cuda)
    ws = torch.zeros(int(L.spz_amd_seed_workspace_bytes(p.width, p.height, opts.stride)), dtype=torch.uint8, device=cuda)
    counts = torch.full((3,), -1, dtype=torch.int64, device=cuda)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    rc = L.spz_amd_seed_view_device(C.byref(ptrs), n, capacity, sh_degree, C.byref(p), C.byref(opts), ptr(ti),
                                    image.shape[2], ptr(td), ptr(tw), ptr(tci), ptr(tcd), counts.data_ptr(), ws.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    abi.check(rc, "spz_amd_seed_view_device")
    torch.cuda.synchronize()
    samples = abi.seed_samples(p.width, p.height, opts.stride)
    off = (-ws.data_ptr()) % 256
    return ws[off: off + samples].cpu().numpy(), tuple(int(x) for x in counts.cpu())


@pytest.mark.parametrize("cover_alpha", [0.5, 0.0])
@pytest.mark.parametrize("stride", STRIDES)
def test_select_and_emit_equal_the_reference(cuda, D, stride, cover_alpha):
    from spz_amd import abi
    sh_degree = 1 if stride == 2 else 0
    p, image, depth, weights, ci, cd = hand_made(40 + stride)
    channels = 4 if stride != 3 else 3
    image = np.ascontiguousarray(image[..., :channels])
    opts = abi.seed_options(stride=stride, opacity=0.3, scale_factor=0.8, cover_alpha=cover_alpha, sh_degree=sh_degree)
    ropts = SR.options(stride=stride, opacity=0.3, scale_factor=0.8, cover_alpha=cover_alpha, sh_degree=sh_degree)
    assert np.float32(opts.alpha) == np.float32(ropts["alpha"])
    samples = SR.samples(W, H, stride)
    n0 = 5
    capacity = n0 + samples
    rng = np.random.default_rng(1)
    start = {k: rng.uniform(-1, 1, v.size).astype(np.float32) for k, v in SR.empty_cloud(capacity, sh_degree).items()}
    cloud_t = upload(start, cuda)
    why = {}
    vw = ref_view(p)
    flags, counts = SR.select(vw, image, depth, weights, ci, cd, ropts, room=capacity - n0, why=why)
    want = {k: v.copy() for k, v in start.items()}
    n_want = SR.emit(vw, image, depth, flags, ropts, want, n0, counts[1])
    got_flags, got_counts = seed_view_raw(cuda, cloud_t, n0, capacity, sh_degree, p, opts, image, depth, weights, ci, cd)
    # every branch the maps were made for was reached
    reach = dict(why)
    if cover_alpha > 0:
        reach.pop("depth_not_finite")   # alpha 0 is below cover_alpha there: the division is not reached
    else:
        reach.pop("alpha_low")
    assert all(v > 0 for v in reach.values()), why
    assert np.array_equal(got_flags, flags), f"{(got_flags != flags).sum()} of {flags.size} flags differ"
    assert got_counts == counts and counts[2] == 0 and n_want == n0 + counts[1]
    differ = assert_cloud_equal(cloud_t, want, n_want, sh_degree, f"stride {stride}")
    print(f"stride {stride} cover_alpha {cover_alpha}: {differ} of {3 * counts[1]} log scales differ by one step")
    # nothing beyond the appended points, and nothing before n0, was written
    for k in SR.FIELDS:
        per = start[k].size // capacity
        a = u32(cloud_t[k])
        assert np.array_equal(a[: n0 * per], u32(start[k])[: n0 * per]), k
        assert np.array_equal(a[n_want * per:], u32(start[k])[n_want * per:]), k


def test_select_and_emit_over_more_blocks_than_offset_lanes(cuda, D):
    """333 x 211 at stride 1 is 275 blocks of 256 samples: more than the 256 lanes of the offsets kernel, so a lane owns
    a run of two blocks; the capacity cuts inside a run."""
    from spz_amd import abi
    w, h = 333, 211
    p, image, depth, weights, ci, cd = hand_made(9, w, h)
    opts, ropts = abi.seed_options(sh_degree=3), SR.options(sh_degree=3)
    samples = SR.samples(w, h, 1)
    assert (samples + 255) // 256 == 275
    vw = ref_view(p)
    total = SR.select(vw, image, depth, weights, ci, cd, ropts)[1][1]
    n0, room = 7, total - 1000
    start = {k: np.full(v.size, 0.25, np.float32) for k, v in SR.empty_cloud(n0 + room, 3).items()}
    cloud_t = upload(start, cuda)
    flags, counts = SR.select(vw, image, depth, weights, ci, cd, ropts, room=room)
    assert counts[1:] == (room, 1000)
    want = {k: v.copy() for k, v in start.items()}
    SR.emit(vw, image, depth, flags, ropts, want, n0, counts[1])
    got_flags, got_counts = seed_view_raw(cuda, cloud_t, n0, n0 + room, 3, p, opts, image, depth, weights, ci, cd)
    assert np.array_equal(got_flags, flags) and got_counts == counts
    assert_cloud_equal(cloud_t, want, n0 + room, 3, "275 blocks")


# ---- edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", STRIDES)
def test_edges(cuda, D, stride):
    import torch
    p, image, depth, weights, ci, cd = hand_made(7)
    samples = SR.samples(W, H, stride)
    ti, td = torch.from_numpy(image).to(cuda), torch.from_numpy(depth).to(cuda)
    vw = ref_view(p)
    # a view that selects nothing: the cloud and n stay, nothing is raised
    capacity = 10 + samples
    rng = np.random.default_rng(2)
    start = {k: rng.uniform(-1, 1, v.size).astype(np.float32) for k, v in SR.empty_cloud(capacity, 0).items()}
    cloud_t = upload(start, cuda)
    nothing = torch.full((H, W), float("inf"), device=cuda)
    n, counts = D.seed_view(cloud_t, 10, capacity, 0, p, ti, nothing, stride=stride, cover=False)
    assert (n, counts) == (10, (0, 0, 0))
    n, counts = D.seed_view(cloud_t, 10, capacity, 0, p, ti, td, weights=torch.zeros((H, W), device=cuda), stride=stride,
                            cover=False)
    assert (n, counts) == (10, (0, 0, 0))
    for k in SR.FIELDS:
        assert np.array_equal(u32(cloud_t[k]), u32(start[k])), k
    # all samples valid with cover off: exactly seed_samples, from an empty cloud
    good_image = np.clip(np.nan_to_num(image, nan=0.5, posinf=0.5), 0, 1).astype(np.float32)
    good_depth = np.where(np.isfinite(depth) & (depth > 0.4), depth, np.float32(2.0)).astype(np.float32)
    tgi, tgd = torch.from_numpy(good_image).to(cuda), torch.from_numpy(good_depth).to(cuda)
    full = D.alloc_cloud(samples, 0, cuda)
    n_full, counts = D.seed_view(full, 0, samples, 0, p, tgi, tgd, stride=stride, cover=False)
    assert (n_full, counts) == (samples, (samples, samples, 0))
    ropts = SR.options(stride=stride, cover=False)
    flags, rcounts = SR.select(vw, good_image, good_depth, None, None, None, ropts)
    want = SR.empty_cloud(samples, 0)
    SR.emit(vw, good_image, good_depth, flags, ropts, want, 0, rcounts[1])
    assert_cloud_equal(full, want, samples, 0, "all valid")
    # n = 0 with cover on takes the no-render path: the same result
    again = D.alloc_cloud(samples, 0, cuda)
    assert D.seed_view(again, 0, samples, 0, p, tgi, tgd, stride=stride, cover=True) == (samples, (samples, samples, 0))
    for k in SR.FIELDS:
        assert np.array_equal(u32(again[k]), u32(full[k])), k
    # capacity cuts mid-view, mid-block: the first capacity - n in lattice order, the rest refused
    n0, room = 3, samples // 2 + 37
    cut_start = {k: rng.uniform(-1, 1, v.size).astype(np.float32) for k, v in SR.empty_cloud(n0 + room, 0).items()}
    cut = upload(cut_start, cuda)
    n_cut, counts = D.seed_view(cut, n0, n0 + room, 0, p, tgi, tgd, stride=stride, cover=False)
    assert (n_cut, counts) == (n0 + room, (samples, room, samples - room))
    for k in SR.FIELDS:
        per = cut_start[k].size // (n0 + room)
        a = u32(cut[k])
        assert np.array_equal(a[: n0 * per], u32(cut_start[k])[: n0 * per]), k
        assert np.array_equal(a[n0 * per:], u32(full[k])[: room * per]), k
    # a full cloud refuses everything and writes nothing
    n_same, counts = D.seed_view(cut, n0 + room, n0 + room, 0, p, tgi, tgd, stride=stride, cover=False)
    assert (n_same, counts) == (n0 + room, (samples, 0, samples))
    with pytest.raises(ValueError, match="depth must be"):
        D.seed_view(full, 0, samples, 0, p, tgi, tgd[:-1], stride=stride)
    with pytest.raises(ValueError, match="at least"):
        D.seed_view(full, 0, samples + 1, 0, p, tgi, tgd, stride=stride)


# ---- the loop --------------------------------------------------------------------------------------------------------
_scene = {}


def scene(cuda, D):
    """A small synthetic scene, three views of it from distinct sides, and their images and depth maps from the device's
    own render_depth (expected depth where alpha >= 0.5, inf elsewhere): made once per module."""
    if not _scene:
        import torch
        rng = np.random.default_rng(11)
        n = 900
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cloud = {"positions": (0.6 * d * [1.0, 0.8, 1.2]).astype(np.float32).ravel(),
                 "scales": np.full(3 * n, np.log(0.05), np.float32),
                 "rotations": np.tile(np.array([0, 0, 0, 1], np.float32), n),
                 "alphas": np.full(n, 3.0, np.float32),
                 "colors": rng.uniform(-1.5, 1.5, 3 * n).astype(np.float32),
                 "sh": np.zeros(0, np.float32)}
        cloud_t = upload(cloud, cuda)
        views = [params(RR.look_at(eye, [0, 0, 0], up)) for eye, up in
                 (([0.2, -0.1, -2.4], [0, 1, 0]), ([2.3, 0.3, 0.4], [0, 1, 0]), ([-0.3, 2.5, 0.2], [0, 0, 1]))]
        images, depths = [], []
        for p in views:
            depth, image = D.render_depth(cloud_t, n, 0, p, return_image=True, return_index=False)
            z = D.expected_depth(depth, image[..., 3])
            z = torch.where(image[..., 3] >= 0.5, z, torch.full_like(z, float("inf")))
            images.append(image.contiguous())
            depths.append(z.contiguous())
        torch.cuda.synchronize()
        _scene.update(views=views, images=images, depths=depths)
    return _scene["views"], _scene["images"], _scene["depths"]


_loops = {}


def loop(cuda, D, stride):
    if stride not in _loops:
        views, images, depths = scene(cuda, D)
        _loops[stride] = D.seed(views, images, depths, stride=stride)
    return _loops[stride]


@pytest.mark.parametrize("stride", STRIDES)
def test_loop_equals_the_reference(cuda, D, stride):
    import torch
    views, images, depths = scene(cuda, D)
    cloud, n, counts = loop(cuda, D, stride)
    np_images = [t.cpu().numpy() for t in images]
    np_depths = [t.cpu().numpy() for t in depths]
    capacity = sum(SR.samples(W, H, stride) for _ in views)
    state = {"k": 0, "n": 0}

    def render_depth(_cloud, n_so_far, vw):
        # the device's own render of the cloud the device built so far: the comparison tests seed, not the rasteriser
        k = state["k"] = state["k"] + 1
        assert n_so_far == sum(c[1] for c in counts[:k]), "the reference and the device disagree on n before this view"
        head = {f: cloud[f][: n_so_far * (3 if f in ("positions", "scales", "colors") else 4 if f == "rotations" else 1)]
                for f in ("positions", "scales", "rotations", "alphas", "colors")}
        view = views[k]
        depth, image = D.render_depth(head, n_so_far, 0, view, return_image=True, return_index=False)
        torch.cuda.synchronize()
        return image.cpu().numpy(), depth.cpu().numpy()

    want, n_want, want_counts = SR.seed_loop([ref_view(p) for p in views], np_images, np_depths, None,
                                             SR.options(stride=stride), capacity, render_depth)
    assert [tuple(c) for c in counts] == [tuple(c) for c in want_counts]
    assert n == n_want == sum(c[1] for c in counts)
    differ = assert_cloud_equal(cloud, want, n, 0, f"loop at stride {stride}")
    print(f"loop at stride {stride}: counts {counts}; {differ} of {3 * n} log scales differ by one step")
    # the cover test did something: the later views append fewer than their valid counts; the first appends them all
    assert counts[0][1] == counts[0][0] > 0
    assert 0 < counts[1][1] < counts[1][0] and 0 < counts[2][1] < counts[2][0]
    assert all(c[2] == 0 for c in counts)
    # a second run repeats its bytes
    cloud2, n2, counts2 = D.seed(views, images, depths, stride=stride)
    assert n2 == n and counts2 == counts
    for k in ("positions", "scales", "rotations", "alphas", "colors"):
        assert np.array_equal(u32(cloud2[k]), u32(cloud[k])), k


# ---- through every layer ---------------------------------------------------------------------------------------------
def gunzip(b):
    return zlib.decompress(b, 16 + 15)


def view_dicts(views):
    return [{"world_to_camera": np.array(list(p.world_to_camera), np.float32).reshape(3, 4), "fx": p.fx, "fy": p.fy,
             "cx": p.cx, "cy": p.cy, "width": p.width, "height": p.height} for p in views]


def files(tmp_path, views, images, depths):
    write_views(tmp_path / "views.txt", view_dicts(views))
    ims, zs = [], []
    for k, (im, z) in enumerate(zip(images, depths)):
        ims.append(str(tmp_path / f"im{k}.pfm"))
        zs.append(str(tmp_path / f"z{k}.pfm"))
        write_pfm(ims[-1], np.ascontiguousarray(im[..., :3]), b"PF")
        write_pfm(zs[-1], z, b"Pf")
    return str(tmp_path / "views.txt"), ims, zs


@pytest.mark.parametrize("stride,sh_degree", [(1, 0), (3, 2)])
def test_through_every_layer(cuda, D, tmp_path, stride, sh_degree):
    """The three views with a mask on the second (its right half does not count): device.seed, spz.seed_spz (a mask
    for that view alone) and spz_seed (a mask file per view, all ones for the others) write the same bytes."""
    import torch
    import spz_amd.spz as spz
    from spz_amd import abi
    views, images, depths = scene(cuda, D)
    np_images = [np.ascontiguousarray(t.cpu().numpy()[..., :3]) for t in images]
    np_depths = [t.cpu().numpy() for t in depths]
    mask = np.zeros((H, W), np.float32)
    mask[:, : W // 2] = 1.0
    cloud, n, counts = D.seed(views, [t[..., :3].contiguous() for t in images], depths, stride=stride, sh_degree=sh_degree,
                              weights=[None, torch.from_numpy(mask).to(cuda), None])
    unmasked = loop(cuda, D, stride)[2]
    assert counts[0] == unmasked[0] and 0 < counts[1][0] < unmasked[1][0], "the mask removed samples of view 1"
    want = D.encode(cloud, n, sh_degree, False, abi.UNSPECIFIED).cpu().numpy().tobytes()
    rep = spz.seed_spz(view_dicts(views), np_images, np_depths, masks=[None, mask, None], stride=stride,
                       sh_degree=sh_degree)
    assert [(v["valid"], v["appended"], v["refused"]) for v in rep["views"]] == [tuple(c) for c in counts]
    assert rep["num_points"] == n == sum(c[1] for c in counts) and len(rep["ms"]) == 3
    assert gunzip(rep["data"]) == want, "spz.seed_spz against the encode of device.seed's cloud"
    vf, ims, zs = files(tmp_path, views, np_images, np_depths)
    ms = []
    for k, m in enumerate((np.ones_like(mask), mask, np.ones_like(mask))):   # the tool reads the first channel
        ms.append(str(tmp_path / f"mask{k}.pfm"))
        write_pfm(ms[-1], np.stack([m, 1.0 - m, np.zeros_like(m)], axis=-1), b"PF")
    out = str(tmp_path / "seeded.spz")
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_seed"), out, "--views", vf, "--images"] + ims +
                       ["--depths"] + zs + ["--masks"] + ms + ["--stride", str(stride), "--sh-degree", str(sh_degree)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"points {n}"
    assert lines[:3] == [f"view {k} valid {c[0]} appended {c[1]} refused {c[2]}" for k, c in enumerate(counts)]
    with open(out, "rb") as f:
        assert f.read() == rep["data"], "spz_seed's file against spz.seed_spz's bytes"
    out2 = str(tmp_path / "seeded2.spz")
    rep2 = spz.seed_spz(view_dicts(views), np_images, np_depths, masks=[None, mask, None], stride=stride,
                        sh_degree=sh_degree, out=out2)
    assert "data" not in rep2 and open(out2, "rb").read() == rep["data"]
    g = spz.load_spz(out)
    assert g.num_points == n and g.sh_degree == sh_degree


def test_a_cover_render_above_max_entries_raises(cuda, D):
    """With status 1 the depth render writes neither map, so seed_view must not decide anything on them."""
    views, images, depths = scene(cuda, D)
    capacity = 2 * SR.samples(W, H, 2)
    cloud = D.alloc_cloud(capacity, 0, cuda)
    n, counts = D.seed_view(cloud, 0, capacity, 0, views[0], images[0], depths[0], stride=2, max_entries=1)
    assert n == counts[1] > 0, "an empty cloud is not rendered: max_entries is not met"
    kept = {k: v.clone() for k, v in cloud.items()}
    with pytest.raises(RuntimeError, match="tile entries is above max_entries = 1"):
        D.seed_view(cloud, n, capacity, 0, views[1], images[1], depths[1], stride=2, max_entries=1)
    with pytest.raises(RuntimeError, match="above max_entries"):
        D.seed(views, images, depths, stride=2, max_entries=1)
    for k in SR.FIELDS:
        assert np.array_equal(u32(cloud[k]), u32(kept[k])), k
    # room for the entries: the result of the default, which sizes the workspace from the total
    n1, counts1 = D.seed_view(cloud, n, capacity, 0, views[1], images[1], depths[1], stride=2, max_entries=1 << 20)
    assert (counts, counts1) == tuple(loop(cuda, D, 2)[2][:2]) and n1 == n + counts1[1]
    with pytest.raises(ValueError, match="max_entries"):
        D.seed_view(cloud, n, capacity, 0, views[1], images[1], depths[1], stride=2, max_entries=-1)


def sections(stream, sh_degree=0):
    """The six sections of a version 3 stream as byte arrays keyed by bytes per point, and the point count."""
    from spz_amd import abi
    rc, h = abi.peek_header(stream)
    assert rc == 0 and h.version == 3 and h.sh_degree == sh_degree
    lay = abi.stream_layout(h.num_points, sh_degree, 3)
    body = np.frombuffer(stream, np.uint8)
    return [body[lay.offset[s]: lay.offset[s] + lay.bytes[s]] for s in range(abi.NUM_SECTIONS)], \
        [lay.bytes_per_point[s] for s in range(abi.NUM_SECTIONS)], h.num_points


_plane = {}


def plane_scene(cuda, D):
    """A textured plane at z = 0 and three views that look straight at it, so that every measured depth is the plane's
    and the cover test turns on the rendered alpha alone, far from its threshold: view 0 from z = -2; view 1 from z = -1.5
    with its whole frame at least two lattice steps inside view 0's footprint (every sample has view 0's Gaussians on
    all sides of it); view 2 from z = -2, three units to the side, 13 lattice steps clear of view 0's
    footprint (alpha 0).  Neither decision lies near a threshold that the 24-bit positions, 8-bit log scales and
    8-bit alphas of a base file could carry it across."""
    if not _plane:
        import torch
        xs, ys = np.arange(-1.3, 4.3, 0.04), np.arange(-1.0, 1.0, 0.04)
        gx, gy = np.meshgrid(xs, ys)
        n = gx.size
        rng = np.random.default_rng(17)
        cloud = {"positions": np.stack([gx.ravel(), gy.ravel(), np.zeros(n)], axis=1).astype(np.float32).ravel(),
                 "scales": np.full(3 * n, np.log(0.04), np.float32),
                 "rotations": np.tile(np.array([0, 0, 0, 1], np.float32), n),
                 "alphas": np.full(n, 3.0, np.float32),
                 "colors": rng.uniform(-1.5, 1.5, 3 * n).astype(np.float32),
                 "sh": np.zeros(0, np.float32)}
        cloud_t = upload(cloud, cuda)
        views = [params(RR.look_at(eye, [eye[0], eye[1], 0.0], [0, 1, 0])) for eye in
                 ([0.0, 0.0, -2.0], [0.1, -0.05, -1.5], [3.0, 0.0, -2.0])]
        images, depths = [], []
        for p in views:
            depth, image = D.render_depth(cloud_t, n, 0, p, return_image=True, return_index=False)
            z = D.expected_depth(depth, image[..., 3])
            z = torch.where(image[..., 3] >= 0.5, z, torch.full_like(z, float("inf")))
            images.append(np.ascontiguousarray(image.cpu().numpy()[..., :3]))
            depths.append(z.cpu().numpy())
        _plane.update(views=views, images=images, depths=depths)
    return _plane["views"], _plane["images"], _plane["depths"]


def test_onto(cuda, D, tmp_path):
    """With a base file equal to the seed of view 0, seeding views 0..2 onto it writes exactly the points the three-view
    loop appended for views 1 and 2, byte for byte in their sections; spz_merge of the base and the new file loads to
    the three-view result.  The scene is plane_scene's: a view does not explain all of itself on a curved surface
    (on the ellipsoid of the loop test, at stride 2, view 0 seeded onto its own Gaussians, as floats or through their
    file alike, appends 41 of its 231 samples again: at the limb the blended depth lies more than 5 % in front of the
    measurement), and the three-view loop never tests view 0 against itself."""
    import spz_amd.spz as spz
    views, np_images, np_depths = plane_scene(cuda, D)
    vd = view_dicts(views)
    whole = spz.seed_spz(vd, np_images, np_depths, stride=2)
    base = spz.seed_spz(vd[:1], np_images[:1], np_depths[:1], stride=2)
    n0 = base["num_points"]
    samples = SR.samples(W, H, 2)
    assert [(v["valid"], v["appended"]) for v in whole["views"]] == [(samples, samples), (samples, 0), (samples, samples)]
    assert n0 == whole["views"][0]["appended"] > 0
    vf, ims, zs = files(tmp_path, views, np_images, np_depths)
    base_file, new_file, merged, whole_file = (str(tmp_path / f) for f in ("base.spz", "new.spz", "merged.spz", "whole.spz"))
    with open(base_file, "wb") as f:
        f.write(base["data"])
    with open(whole_file, "wb") as f:
        f.write(whole["data"])
    tool = os.path.join(ROOT, "spz_amd", "bin")
    r = subprocess.run([os.path.join(tool, "spz_seed"), new_file, "--views", vf, "--images"] + ims + ["--depths"] + zs +
                       ["--stride", "2", "--onto", base_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    print("three views:", whole["views"])
    new_stream = gunzip(open(new_file, "rb").read())
    onto = spz.seed_spz(vd, np_images, np_depths, stride=2, base=base_file)
    assert gunzip(onto["data"]) == new_stream, "spz.seed_spz(base=path) against spz_seed --onto"
    assert spz.seed_spz(vd, np_images, np_depths, stride=2, base=base["data"])["data"] == onto["data"], "base as bytes"
    # the new file's sections are the tails of the three-view file's
    sec_w, bpp, n_w = sections(gunzip(whole["data"]))
    sec_n, _, n_n = sections(new_stream)
    assert [(v["valid"], v["appended"]) for v in onto["views"]] == \
        [(whole["views"][0]["valid"], 0)] + [(v["valid"], v["appended"]) for v in whole["views"][1:]]
    assert n_n == n_w - n0
    for a, b, per in zip(sec_w, sec_n, bpp):
        assert np.array_equal(a[n0 * per:], b), f"the section of {per} bytes per point differs"
    r = subprocess.run([os.path.join(tool, "spz_merge"), base_file, new_file, "-o", merged], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    g, w = spz.load_spz(merged), spz.load_spz(whole_file)
    assert g.num_points == w.num_points == n_w
    for k in ("positions", "scales", "rotations", "alphas", "colors", "sh"):
        assert np.array_equal(u32(np.asarray(getattr(g, k))), u32(np.asarray(getattr(w, k)))), k
