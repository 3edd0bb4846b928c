"""spz_amd_tsdf_integrate_device / spz_amd_mesh_count_device + _emit_device / spz_amd_mesh_open, spz_amd.device.tsdf_* +
mesh_packed, spz.mesh_spz and spz_mesh (include/spz_amd.h "mesh"; DESIGN §8 "Mesh") on the GPU, bit for bit against the
numpy restatement of tests/mesh_ref.py: the contract fixes every operation's order and precision, so nothing here has a
tolerance but the one geometric bound of the analytic fuse (a vertex lies within `truncation` of the surface)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import mesh_ref as MR
import render_ref as RR
from conftest import ROOT
from test_mesh_host import read_mesh_ply

pytestmark = pytest.mark.gpu

DIMS, LO, VOXEL, TRUNC = (28, 26, 30), (-1.37, -1.29, -1.46), 0.1, 0.4     # not multiples of the 64 x 4 block
W, H, F = 64, 48, 60.0


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


@pytest.fixture(scope="module")
def D(cuda):
    from spz_amd import device
    return device


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def u32(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def params(m, near=0.2, width=W, height=H, f=F, coord=0):
    from spz_amd import abi
    return abi.render_params(m, f, f, 0.5 * width, 0.5 * height, width, height, near, coord=coord)


def ref_view(p):
    """The view of an abi.RenderParams as mesh_ref takes it: the same float32 values."""
    return {"world_to_camera": np.array(list(p.world_to_camera), np.float32).reshape(3, 4), "fx": p.fx, "fy": p.fy,
            "cx": p.cx, "cy": p.cy, "width": p.width, "height": p.height, "near": p.near_plane}


def volumes():
    from spz_amd import abi
    return abi.tsdf_volume(LO, DIMS, VOXEL, TRUNC), MR.volume(LO, DIMS, VOXEL, TRUNC)


def assert_grid_equal(got, want):
    g = got.cpu().numpy()
    for k, name in enumerate(("W", "S", "Cr", "Cg", "Cb")):
        assert np.array_equal(u32(g[k]), u32(want[k])), \
            f"plane {name}: {(u32(g[k]) != u32(want[k])).sum()} of {g[k].size} values differ"


def assert_mesh_equal(got, want, what=""):
    for a, b, name in zip(got, want, ("vertices", "colors", "triangles")):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        assert a.shape == b.shape, f"{what} {name}: shape {a.shape} != {b.shape}"
        assert np.array_equal(u32(a), u32(b)), f"{what} {name}: {(u32(a) != u32(b)).sum()} of {a.size} values differ"


# ---- the fuse --------------------------------------------------------------------------------------------------------
def hand_made_views(ms=None):
    """Three views of the lattice (or the poses `ms`, the second one with the farther near plane) with depth and image
    arrays that reach every branch of the fuse."""
    rng = np.random.default_rng(23)
    if ms is None:
        ms = [RR.look_at([0.1, -0.05, -3.0], [0, 0, 0], [0, 1, 0]),        # outside: the lattice overflows the image
              RR.look_at([0.2, 0.1, -0.5], [0.1, 0.3, 1.0], [0, 1, 0]),    # inside the lattice: points behind `near`
              RR.look_at([3.1, 0.4, 0.3], [0, 0, 0], [0, 0, 1])]           # from +x, z up
    out = []
    for k, m in enumerate(ms):
        p = params(m, near=0.2 if k != 1 else 0.35)
        dist = float(np.linalg.norm(np.asarray(m)[:, 3]))
        median = rng.uniform(dist - 1.6, dist + 1.6, size=(H, W)).astype(np.float32)     # sdf on both sides of +-trunc
        median[rng.random((H, W)) < 0.08] = np.inf
        median[rng.random((H, W)) < 0.02] = 0.0
        median[rng.random((H, W)) < 0.02] = -1.5
        median[rng.random((H, W)) < 0.02] = np.nan
        alpha = rng.uniform(0.2, 1.0, size=(H, W)).astype(np.float32)                    # some below min_alpha = 0.5
        alpha[rng.random((H, W)) < 0.05] = 0.0
        expected = rng.uniform(dist - 1.6, dist + 1.6, size=(H, W)).astype(np.float32)
        depth = np.stack([expected * alpha, median], axis=-1).astype(np.float32)
        image = np.concatenate([rng.uniform(-0.2, 1.3, size=(H, W, 3)).astype(np.float32), alpha[..., None]], axis=-1)
        out.append((p, depth, np.ascontiguousarray(image)))
    return out


def fuse_views_and_compare(cuda, D, grid, want, vol, rvol, views, kind):
    """Fuses `views` into the device's `grid` and the reference's `want`, comparing after every view.  Returns what the
    views reach, from the reference's own intermediate values, and the lattice points some view updated."""
    import torch
    rk = MR.MEDIAN if kind == "median" else MR.EXPECTED
    reached = {"near": False, "off_image": False, "behind": False, "front": False, "updated": False}
    touched = np.zeros(want.shape[1:], bool)
    for p, depth, image in views:
        D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda), depth_kind=kind,
                         min_alpha=0.5)
        before = want.copy()
        ok = MR.integrate(want, rvol, ref_view(p), depth, image, rk, 0.5)
        assert_grid_equal(grid, want)
        pts = MR.lattice_points(rvol)
        M = ref_view(p)["world_to_camera"].astype(np.float64)
        z = pts @ M[2, :3] + M[2, 3]
        reached["near"] |= bool((z <= p.near_plane).any())
        u = np.floor(p.fx * ((pts @ M[0, :3] + M[0, 3]) / z) + p.cx)
        reached["off_image"] |= bool(((z > p.near_plane) & ((u < 0) | (u >= p.width))).any())
        d = (want[1] - before[1])[ok]
        reached["front"] |= bool((d == 1.0).any())                     # sdf > truncation: clamped to 1
        reached["behind"] |= bool((~ok).any())
        reached["updated"] |= bool(ok.any())
        touched |= ok
    return reached, touched


@pytest.mark.parametrize("kind", ["median", "expected"])
def test_integrate_equals_the_reference_bit_for_bit(cuda, D, kind):
    vol, rvol = volumes()
    grid = D.tsdf_alloc(vol, cuda)
    assert tuple(grid.shape) == (5, DIMS[2], DIMS[1], DIMS[0]) and not grid.any()
    want = np.zeros((5, DIMS[2], DIMS[1], DIMS[0]), np.float32)
    reached, _ = fuse_views_and_compare(cuda, D, grid, want, vol, rvol, hand_made_views(), kind)
    assert all(reached.values()), reached
    assert want[0].max() == 3.0 and (want[0] == 0).any()
    # a second pass over the same views accumulates
    fuse_views_and_compare(cuda, D, grid, want, vol, rvol, hand_made_views(), kind)
    assert want[0].max() == 6.0


def test_a_view_that_touches_nothing_leaves_the_grid(cuda, D):
    import torch
    vol, rvol = volumes()
    (p, depth, image), = hand_made_views()[:1]
    grid = D.tsdf_alloc(vol, cuda)
    D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda))
    kept = grid.clone()
    away = params(RR.look_at([0, 0, -3.0], [0, 0, -6.0], [0, 1, 0]))                 # the lattice is behind the camera
    D.tsdf_integrate(grid, vol, away, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda))
    nothing = depth.copy()
    nothing[..., 1] = np.inf                                                        # no median anywhere
    D.tsdf_integrate(grid, vol, p, torch.from_numpy(nothing).to(cuda), torch.from_numpy(image).to(cuda))
    faint = image.copy()
    faint[..., 3] = 0.3                                                             # every alpha below min_alpha
    D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(faint).to(cuda),
                     depth_kind="expected", min_alpha=0.5)
    far = depth.copy()
    far[..., 1] = 0.5                                                               # every sdf below -truncation
    D.tsdf_integrate(grid, vol, p, torch.from_numpy(far).to(cuda), torch.from_numpy(image).to(cuda))
    assert np.array_equal(u32(grid), u32(kept))
    with pytest.raises(ValueError, match="depth must be"):
        D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth[:-1]).to(cuda), torch.from_numpy(image).to(cuda))
    with pytest.raises(ValueError, match="grid must be"):
        D.tsdf_integrate(grid[:4], vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda))


# ---- the extraction --------------------------------------------------------------------------------------------------
_analytic = {}


def analytic(name):
    """The analytic grid, its volume (both forms) and the reference's mesh: made once per module."""
    if not _analytic:
        from spz_amd import abi
        for k, (g, rvol) in MR.analytic_grids().items():
            vol = abi.tsdf_volume(rvol["lo"], rvol["dims"], float(rvol["voxel_size"]), float(rvol["truncation"]))
            _analytic[k] = (g, vol, MR.extract(g, rvol))
    return _analytic[name]


@pytest.mark.parametrize("name", ["sphere", "torus", "half_sphere", "plane"])
def test_extract_equals_the_reference_bit_for_bit(cuda, D, name):
    import torch
    g, vol, want = analytic(name)
    got = D.tsdf_extract(torch.from_numpy(g).to(cuda), vol)
    assert got[0].dtype == torch.float32 and got[2].dtype == torch.int32
    assert_mesh_equal(got, want, name)
    # the invariants, on the device's own output
    v, t = got[0].cpu().numpy(), got[2].cpu().numpy().view(np.uint32)
    assert np.array_equal(np.unique(t), np.arange(len(v))), "every vertex referenced"
    und, dire = MR.edge_counts(t)
    assert set(dire.values()) == {1}
    euler = MR.euler_characteristic(len(v), t)
    if name == "sphere":
        assert (len(v), len(t)) == (2534, 5064) and set(und.values()) == {2} and euler == 2
        out = v[t].astype(np.float64).mean(axis=1) - np.array(MR.SPHERE_C)
        assert ((MR.triangle_normals(v, t) * out).sum(axis=1) > 0).all()
    elif name == "torus":
        assert set(und.values()) == {2} and euler == 0
    elif name == "half_sphere":
        assert set(und.values()) == {1, 2} and euler == 1
        assert v[:, 0].max() <= 9.0, "a triangle in a cube with an invalid corner"
    else:
        assert (v[:, 0] == 7.0).all() and t.max() < len(v)
        area = 0.5 * np.linalg.norm(MR.triangle_normals(v, t), axis=1)
        assert area.sum() == 17 * 21 and (area == 0).any()
    again = D.tsdf_extract(torch.from_numpy(g).to(cuda), vol, stream=torch.cuda.Stream(cuda))
    torch.cuda.synchronize()
    assert_mesh_equal(again, want, name + " (a second run, on a side stream)")


def test_extract_min_weight_and_no_crossing(cuda, D):
    import torch
    g, vol, _ = analytic("sphere")
    nothing = g.copy()
    nothing[1] = np.abs(nothing[1]) + 1.0                       # positive everywhere: no crossing
    for grid in (nothing, np.zeros_like(g)):                    # and a grid no view has touched (W = 0: f is NaN)
        v, c, t = D.tsdf_extract(torch.from_numpy(grid).to(cuda), vol)
        assert tuple(v.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    # W = 2 on one half, 1 on the other: min_weight 2 keeps the cubes of the first half only
    x, _, _ = MR.field_coords()
    two = g.copy()
    two[:, x < 10] *= 2.0
    half = analytic("half_sphere")[2]
    got = D.tsdf_extract(torch.from_numpy(two).to(cuda), vol, min_weight=2.0)
    assert_mesh_equal(got, half, "min_weight 2")
    assert_mesh_equal(D.tsdf_extract(torch.from_numpy(two).to(cuda), vol), analytic("sphere")[2], "min_weight 1")


def test_emit_capacity_one_short_writes_nothing(cuda, D):
    g, vol, want = analytic("sphere")
    check_capacity_one_short(cuda, g, vol, want)


def check_capacity_one_short(cuda, g, vol, want):
    """The count / emit pair of the C ABI on grid `g`: the counts are those of the mesh `want`, an emit whose capacity is
    one short of either is refused and writes nothing, and the emit after it gives `want`."""
    import ctypes as C
    import torch
    from spz_amd import abi
    L = abi.load_library()
    nv, nt = len(want[0]), len(want[2])
    grid = torch.from_numpy(g).to(cuda)
    ws = torch.empty(int(L.spz_amd_mesh_workspace_bytes(C.byref(vol))), dtype=torch.uint8, device=cuda)
    counts = torch.zeros(2, dtype=torch.int64, device=cuda)
    st = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert L.spz_amd_mesh_count_device(C.byref(vol), grid.data_ptr(), 1.0, counts.data_ptr(), ws.data_ptr(), st) == abi.OK
    assert counts.cpu().tolist() == [nv, nt]
    pos = torch.full((nv, 3), 7.0, dtype=torch.float32, device=cuda)
    col = torch.full((nv, 3), 7.0, dtype=torch.float32, device=cuda)
    tri = torch.full((nt, 3), 7, dtype=torch.int32, device=cuda)
    emit = lambda cap_v, cap_t: L.spz_amd_mesh_emit_device(C.byref(vol), grid.data_ptr(), nv, nt, cap_v, cap_t,
                                                           pos.data_ptr(), col.data_ptr(), tri.data_ptr(), ws.data_ptr(), st)
    assert emit(nv - 1, nt) == abi.ERR_CAPACITY and emit(nv, nt - 1) == abi.ERR_CAPACITY
    torch.cuda.synchronize()
    assert (pos == 7.0).all() and (col == 7.0).all() and (tri == 7).all(), "a refused emit wrote something"
    assert emit(nv, nt) == abi.OK
    assert_mesh_equal((pos, col, tri), want, "after the refused calls")


# ---- analytic fuse + extract -----------------------------------------------------------------------------------------
def sphere_views():
    """Six views of the unit sphere at the origin from +-3 on every axis, slightly off-axis, with the median depth of
    the ray-sphere intersection at the pixel centres (+inf off the sphere) and the hit point's normal as colour."""
    out = []
    for k, eye in enumerate([(3, 0.2, -0.1), (-3, 0.1, 0.2), (0.15, 3, 0.1), (-0.1, -3, 0.2), (0.2, -0.1, 3),
                             (0.1, 0.15, -3)]):
        up = (0, 0, 1) if k in (2, 3) else (0, 1, 0)
        p = params(RR.look_at(eye, [0, 0, 0], up))
        M = ref_view(p)["world_to_camera"].astype(np.float64)
        v, u = np.mgrid[0:H, 0:W].astype(np.float64)
        d = np.stack([(u + 0.5 - p.cx) / p.fx, (v + 0.5 - p.cy) / p.fy, np.ones_like(u)], axis=-1)   # z = t along d
        c = M[:, 3]                                                   # the sphere's centre in the camera frame
        a, b, cc = (d * d).sum(-1), -2.0 * (d @ c), float(c @ c) - 1.0
        disc = b * b - 4 * a * cc
        hit = disc > 0
        t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), np.inf)
        world = (np.where(hit, t, 0.0)[..., None] * d - c) @ M[:, :3]   # R^T (p_c - t): the hit point, the unit normal
        depth = np.stack([np.where(hit, t, 0.0), t], axis=-1).astype(np.float32)
        image = np.concatenate([np.where(hit[..., None], 0.5 + 0.5 * world, 0.0), hit[..., None]], axis=-1)
        out.append((p, depth, np.ascontiguousarray(image.astype(np.float32))))
    return out


def test_analytic_sphere_fused_and_extracted(cuda, D):
    import torch
    vol, rvol = volumes()
    grid = D.tsdf_alloc(vol, cuda)
    want = np.zeros((5, DIMS[2], DIMS[1], DIMS[0]), np.float32)
    for p, depth, image in sphere_views():
        D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda))
        MR.integrate(want, rvol, ref_view(p), depth, image)
    assert_grid_equal(grid, want)
    got = D.tsdf_extract(grid, vol)
    ref = MR.extract(want, rvol)
    assert_mesh_equal(got, ref, "the fused sphere")
    v = got[0].cpu().numpy().astype(np.float64)
    off = np.abs(np.linalg.norm(v, axis=1) - 1.0)
    print(f"{len(v)} vertices, {len(got[2])} triangles; farthest vertex {off.max() / VOXEL:.3f} voxels from the sphere, "
          f"mean {off.mean() / VOXEL:.3f}")
    assert len(v) > 1000
    # a zero crossing needs a negative sample, and those exist only within `truncation` behind an observed depth
    assert off.max() <= TRUNC


# ---- end to end ------------------------------------------------------------------------------------------------------
def disc_cloud(n=300):
    """n opaque flat Gaussians on the unit sphere: discs of radius ~0.15 whose thin axis is the normal."""
    k = np.arange(n) + 0.5
    zc = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - zc * zc)
    nrm = np.stack([r * np.cos(phi), r * np.sin(phi), zc], axis=1)
    axis = np.cross([0.0, 0.0, 1.0], nrm)
    s = np.linalg.norm(axis, axis=1)
    theta = np.arctan2(s, nrm[:, 2])
    axis = axis / np.maximum(s, 1e-12)[:, None]
    q = np.concatenate([axis * np.sin(theta / 2)[:, None], np.cos(theta / 2)[:, None]], axis=1)
    return {"positions": nrm.astype(np.float32).reshape(-1),
            "scales": np.tile(np.log(np.float32([0.15, 0.15, 0.01])), n).astype(np.float32),
            "rotations": q.astype(np.float32).reshape(-1), "alphas": np.full(n, 6.0, np.float32),
            "colors": (nrm * 1.2).astype(np.float32).reshape(-1), "sh": np.zeros(0, np.float32)}


def explicit_chain(D, render, views, vol, kind="median", min_alpha=0.5):
    grid = D.tsdf_alloc(vol, "cuda:0")
    for p in views:
        depth, image = render(p)
        D.tsdf_integrate(grid, vol, p, depth, image, depth_kind=kind, min_alpha=min_alpha)
    return tuple(x.cpu().numpy() for x in D.tsdf_extract(grid, vol))


def test_end_to_end_file_python_tool_and_explicit_chain_agree(cuda, spz, D, tmp_path):
    from spz_amd import abi
    n = 300
    stream = D.encode(D.to_device(disc_cloud(n), cuda), n, 0, False, abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0 and h.version == 3
    data = gz(stream.cpu().numpy().tobytes())
    path = str(tmp_path / "discs.spz")
    open(path, "wb").write(data)
    vd = spz.orbit_views(6, width=48, height=48, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=1.0)
    views = [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"])
             for v in vd]
    opts = dict(resolution=24)
    got = D.mesh_packed(stream, h, views, **opts)
    vol = abi.tsdf_volume(got["volume"]["lo"], got["volume"]["dims"], got["volume"]["voxel_size"],
                          got["volume"]["truncation"])
    # the default box is the exact box of the decoded positions, 24 cells along its longest side, truncation 4 voxels
    pos = D.decode(stream, h, 0)["positions"].cpu().numpy().reshape(-1, 3)
    assert np.array_equal(np.float32(got["volume"]["lo"]), pos.min(axis=0))
    side = (pos.max(axis=0).astype(np.float64) - pos.min(axis=0)).max()
    assert got["volume"]["voxel_size"] == np.float32(side / 24) and max(got["volume"]["dims"]) in (25, 26)
    assert got["volume"]["truncation"] == np.float32(4 * (side / 24))
    assert len(got["ms"]) == 3 and got["triangles"].dtype == np.uint32

    def render(p):
        depth, image = D.render_depth_packed(stream, h, p, return_image=True, return_index=False)
        return depth, image
    want = explicit_chain(D, render, views, vol)
    assert len(want[0]) > 500 and len(want[2]) > 1000
    assert_mesh_equal((got["vertices"], got["colors"], got["triangles"]), want, "mesh_packed")
    r = np.linalg.norm(want[0].astype(np.float64), axis=1)
    assert np.abs(r - 1.0).max() <= got["volume"]["truncation"] + 0.05       # discs of thickness 0.01 on the sphere
    for source in (path, data):
        m = spz.mesh_spz(source, vd, **opts)
        assert_mesh_equal((m["vertices"], m["colors"], m["triangles"]), want, "mesh_spz")
        assert m["volume"] == got["volume"] and m["triangles"].dtype == np.uint32
    twice = D.mesh_packed(stream, h, views, **opts)
    for k in ("vertices", "colors", "triangles"):
        assert twice[k].tobytes() == got[k].tobytes(), f"two runs differ in {k}"
    # the tool: the same views through a views file, the PLY parsed back
    vf = tmp_path / "views.txt"
    vf.write_text("".join(" ".join([str(v["width"]), str(v["height"])] + [repr(float(x)) for x in
                                   [v["fx"], v["fy"], v["cx"], v["cy"], *np.asarray(v["world_to_camera"]).reshape(-1)]]) + "\n"
                          for v in vd))
    ply = str(tmp_path / "discs.ply")
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_mesh")
    run = subprocess.run([tool, path, ply, "--views", str(vf), "--resolution", "24"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert f"{len(want[0])} vertices, {len(want[2])} triangles" in run.stdout
    _, pv, pc, pt = read_mesh_ply(ply)
    assert np.array_equal(u32(pv), u32(want[0])) and np.array_equal(pt, want[2].view(np.uint32))
    assert np.array_equal(pc, np.rint(np.float32(255) * np.clip(want[1], 0, 1)).astype(np.uint8))
    # the other options reach the device: an explicit box and voxel size, expected depth, a higher min_weight
    opts2 = dict(box=(-1.2, -1.2, -1.2, 1.2, 1.25, 1.3), voxel_size=0.11, truncation=0.3, depth="expected", min_alpha=0.6,
                 min_weight=2.0)
    vol2 = abi.tsdf_volume_from_box(opts2["box"][:3], opts2["box"][3:], 0.11, 0.3)
    grid = D.tsdf_alloc(vol2, cuda)
    for p in views:
        depth, image = render(p)
        D.tsdf_integrate(grid, vol2, p, depth, image, depth_kind="expected", min_alpha=0.6)
    want2 = tuple(x.cpu().numpy() for x in D.tsdf_extract(grid, vol2, min_weight=2.0))
    m2 = spz.mesh_spz(data, vd, **opts2)
    assert len(want2[2]) > 0 and m2["volume"]["dims"] == tuple(vol2.dims)
    assert_mesh_equal((m2["vertices"], m2["colors"], m2["triangles"]), want2, "mesh_spz with every option")
    with pytest.raises(abi.SpzAmdError) as e:
        D.mesh_packed(stream, h, views + [abi.RenderParams()], **opts)
    assert e.value.view == 6


def test_v2_stream_and_its_decoded_floats_give_the_same_mesh(cuda, D):
    from spz_amd import abi
    n = 300
    stream = D.encode(D.to_device(disc_cloud(n), cuda), n, 0, False, abi.RUB, 2)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0 and h.version == 2
    coord = abi.RDF
    views = [params(RR.look_at(eye, [0, 0, 0], [0, 1, 0]), width=48, height=48, f=50.0, coord=coord)
             for eye in ([2.5, 0.3, 0.2], [-2.5, 0.2, -0.3], [0.3, 0.2, 2.5], [0.2, -0.3, -2.5])]
    got = D.mesh_packed(stream, h, views, voxel_size=0.09)
    vol = abi.tsdf_volume(got["volume"]["lo"], got["volume"]["dims"], got["volume"]["voxel_size"],
                          got["volume"]["truncation"])
    floats = D.decode(stream, h, coord)
    pos = floats["positions"].cpu().numpy().reshape(-1, 3)
    assert np.array_equal(np.float32(got["volume"]["lo"]), pos.min(axis=0)), "the box is taken in the views' frame"

    def render(p):
        depth, image = D.render_depth(floats, n, 0, p, return_image=True, return_index=False)
        return depth, image
    want = explicit_chain(D, render, views, vol)
    assert len(want[2]) > 500
    assert_mesh_equal((got["vertices"], got["colors"], got["triangles"]), want, "a v2 stream against its floats")
