"""The mesh kernels (spz_mesh.hip; DESIGN §8 "Mesh") at the sizes where their size-dependent paths leave their first
arm, bit for bit against tests/mesh_ref.py as test_gpu_mesh.py is: nothing here has a tolerance.

  scan of the block sums   spz_mesh_scan_sums_kernel walks the sums 256 at a time and carries the total of the chunks
                           before: more than 256 blocks of 2048 values, so more than 524,288 lattice points for the
                           triangle scan and more than 74,898 for the edge scan (7 values per point).  The lattices:
                           64 x 64 x 128 (exactly 256 and 7 x 256 blocks: a full last chunk), 83 x 81 x 95 (312 and
                           2,184 blocks: 2 and 9 chunks), 44 x 43 x 45 (42 and 292: the edge scan alone has a second
                           chunk; both faces of a slab, one in each chunk), and the longest lattices the volume
                           check allows.
  the fuse                 a block covers 64 consecutive x and 4 y: lattices of nx = 64, 65, 129 and 2048, ny = 5, 7
                           and 2048, and the 83 x 81 x 95 lattice.
  the box of a stream      spz_mesh_bounds_kernel launches at most 4,096 blocks of 256 and strides: a stream of
                           1,048,576 + 300 points whose extreme coordinates are all among the last 300; and version-1
                           streams (float16 positions) with non-finite positions, which the box leaves out.

Every scene is built on the CPU and the condition that takes it down its path is asserted from the reference alone (the
block counts, the chunks the reference's edge ids and cube indices fall into, the lattice points a view updates, where
in the stream the extremes are), so a scene that stops reaching its path fails instead of passing."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import render_ref as RR
from conftest import load_golden
from test_gpu_mesh import (D, assert_grid_equal, assert_mesh_equal, check_capacity_one_short, disc_cloud,  # noqa: F401
                           explicit_chain, fuse_views_and_compare, hand_made_views, ref_view, sphere_views, spz)

pytestmark = pytest.mark.gpu


# ---- the extraction --------------------------------------------------------------------------------------------------
def _ellipsoid(x, y, z):
    return np.sqrt((x - 31.3) ** 2 + (y - 30.6) ** 2 + ((z - 63.4) / 2.0) ** 2) - 28.7


def _sphere(x, y, z):
    return np.sqrt((x - 41.3) ** 2 + (y - 40.6) ** 2 + (z - 47.4) ** 2) - 38.7


# name: dims, the field, the invalid set (or None), and what the reference must say about it: the blocks of the triangle
# and the edge scan, (vertices, triangles), the least number of triangles per chunk of the triangle scan (0: exactly
# none), the least number of vertices per chunk of the edge scan.
SCENES = {
    "ellipsoid_64x64x128": ((64, 64, 128), _ellipsoid, None, (256, 1792), (79142, 158280), [158280], [5000] * 7),
    "sphere_83x81x95": ((83, 81, 95), _sphere, None, (312, 2184), (84444, 168884), [150000, 17690], [2000] * 8 + [0]),
    "holes_83x81x95": ((83, 81, 95), _sphere, lambda x, y, z: (x + y + z) % 7 == 0, (312, 2184), (49264, 71332),
                       [60000, 7000], [1000] * 8 + [0]),
    "slab_83x81x95": ((83, 81, 95), lambda x, y, z: z - 90.4, None, (312, 2184), (26565, 52480), [0, 52480],
                      [0] * 8 + [26565]),
    "slab_44x43x45": ((44, 43, 45), lambda x, y, z: np.abs(z - 22.0) - 18.4, None, (42, 292), (14790, 28896), [28896],
                      [7395, 7395]),                 # both faces of a slab: the carry into the second chunk is not 0
    "plane_2048x3x3": ((2048, 3, 3), lambda x, y, z: y - 0.4, None, (9, 63), (20475, 32752), [32752], [20475]),
    "plane_3x2048x2": ((3, 2048, 2), lambda x, y, z: x - 0.4, None, (6, 42), (12285, 16376), [16376], [12285]),
    "plane_2x3x2048": ((2, 3, 2048), lambda x, y, z: x - 0.4, None, (6, 42), (20475, 32752), [32752], [20475]),
}
_scenes = {}


def scene(name):
    """(grid, volume, the reference's mesh) of a scene: unit spacing, lo = 0, W = 1 (0 on the invalid set), colours
    i / nx, j / ny, k / nz.  Made once per module; asserts the scene's row of SCENES from the reference's ids."""
    if name not in _scenes:
        from spz_amd import abi
        dims, field, invalid, blocks, counts, tri_floor, edge_floor = SCENES[name]
        x, y, z = MR.field_coords(dims)
        valid = None if invalid is None else ~invalid(x, y, z)
        g = MR.grid_from_field(field(x, y, z), valid=valid, color=MR.field_color(dims))
        rvol = MR.volume((0.0, 0.0, 0.0), dims, 1.0, 4.0)
        v, c, t, used, cubes = MR.extract(g, rvol, return_ids=True)
        n = dims[0] * dims[1] * dims[2]
        assert (MR.scan_blocks(n), MR.scan_blocks(7 * n)) == blocks
        assert (len(v), len(t)) == counts
        tri_chunks, edge_chunks = MR.scan_chunk_counts(cubes, n), MR.scan_chunk_counts(used, 7 * n)
        print(f"{name}: {n} points, {len(v)} vertices, {len(t)} triangles; triangles per chunk {tri_chunks.tolist()}, "
              f"vertices per chunk {edge_chunks.tolist()}")
        for got, floor in ((tri_chunks, tri_floor), (edge_chunks, edge_floor)):
            assert len(got) == len(floor)
            assert all(k >= f if f else k == 0 for k, f in zip(got.tolist(), floor)), (got.tolist(), floor)
        _scenes[name] = (g, abi.tsdf_volume((0.0, 0.0, 0.0), dims, 1.0, 4.0), (v, c, t))
    return _scenes[name]


def check_invariants(v, t, euler, closed):
    """Every vertex referenced, every directed edge once, every undirected edge twice (once or twice when not closed),
    the Euler characteristic.  Returns the boundary edges (m, 2)."""
    assert np.array_equal(np.unique(t), np.arange(len(v))), "every vertex referenced"
    edges, und, dire = MR.edge_multiplicity(t)
    assert (dire == 1).all(), "every directed edge once"
    assert set(np.unique(und).tolist()) == ({2} if closed else {1, 2})
    assert len(v) - len(edges) + len(t) == euler
    return edges[und == 1]


@pytest.mark.parametrize("name", list(SCENES))
def test_extract_past_one_chunk_equals_the_reference(cuda, D, name):
    import torch
    g, vol, want = scene(name)
    got = D.tsdf_extract(torch.from_numpy(g).to(cuda), vol)
    assert_mesh_equal(got, want, name)
    v, t = got[0].cpu().numpy(), got[2].cpu().numpy().view(np.uint32)
    nx, ny, _ = SCENES[name][0]
    if name in ("ellipsoid_64x64x128", "sphere_83x81x95"):
        check_invariants(v, t, 2, closed=True)
    elif name.startswith("slab"):
        rim = check_invariants(v, t, 2 if name == "slab_44x43x45" else 1, closed=False)    # two sheets, one sheet
        on_rim = (v[:, 0] == 0) | (v[:, 0] == nx - 1) | (v[:, 1] == 0) | (v[:, 1] == ny - 1)
        assert len(rim) > 0 and on_rim[rim.reshape(-1)].all(), "boundary edges only on the lattice's rim"


def test_a_second_extraction_on_a_side_stream_gives_the_same(cuda, D):
    import torch
    g, vol, want = scene("sphere_83x81x95")
    grid = torch.from_numpy(g).to(cuda)
    torch.cuda.synchronize()
    for k in range(2):
        again = D.tsdf_extract(grid, vol, stream=torch.cuda.Stream(cuda))
        torch.cuda.synchronize()
        assert_mesh_equal(again, want, f"run {k} on a side stream")


def test_emit_capacity_one_short_writes_nothing_at_scale(cuda):
    g, vol, want = scene("sphere_83x81x95")
    check_capacity_one_short(cuda, g, vol, want)


# ---- the fuse --------------------------------------------------------------------------------------------------------
WIDE = [(64, 5, 3), (64, 7, 3), (65, 5, 4), (65, 7, 3), (129, 5, 3), (129, 7, 2), (2048, 2, 2), (2, 2048, 2),
        (83, 81, 95)]
TRUNC = 0.4


def wide_lattice(dims):
    """(volume, the reference's volume, three poses) of a lattice of `dims` that is 3.6 long along its longest axis a,
    from -2.1 to 1.5, and centred on the others.  The poses are hand_made_views' with the axes renamed: from outside
    across the lattice (a runs along the image, which is 3.2 wide there: the low end is off it), from inside along a
    (what is behind the camera or nearer than `near` is skipped) and obliquely towards the high end."""
    from spz_amd import abi
    d = np.array(dims, np.float64)
    a = int(np.argmax(d))
    b = 2 if a != 2 else 0
    c = 3 - a - b
    s = 3.6 / (d[a] - 1.0)
    lo = -0.5 * (d - 1.0) * s + np.array([0.03, -0.02, 0.04])
    lo[a] = -2.1
    e = np.eye(3)
    poses = [RR.look_at(-3.0 * e[b] + 0.1 * e[a] - 0.05 * e[c], [0, 0, 0], e[c]),
             RR.look_at(0.3 * e[a] + 0.02 * e[b] + 0.01 * e[c], 1.3 * e[a] + 0.05 * e[b] - 0.03 * e[c], e[c]),
             RR.look_at(2.0 * e[a] + 1.5 * e[b] + 0.4 * e[c], 0.9 * e[a], e[c])]
    return abi.tsdf_volume(tuple(lo), dims, s, TRUNC), MR.volume(lo, dims, s, TRUNC), poses


@pytest.mark.parametrize("kind", ["median", "expected"])
@pytest.mark.parametrize("dims", WIDE, ids=["x".join(map(str, d)) for d in WIDE])
def test_integrate_on_lattices_wider_than_a_block(cuda, D, dims, kind):
    nx, ny, nz = dims
    vol, rvol, poses = wide_lattice(dims)
    assert tuple(vol.lo) == tuple(rvol["lo"]) and vol.voxel_size == rvol["voxel_size"]
    grid = D.tsdf_alloc(vol, cuda)
    want = np.zeros((5, nz, ny, nx), np.float32)
    reached, touched = fuse_views_and_compare(cuda, D, grid, want, vol, rvol, hand_made_views(poses), kind)
    assert all(reached.values()), reached
    # updated points past the first block along x and y (i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 +
    # threadIdx.y), in the last block of each axis too, which is a partial one for 65, 129, 5 and 7
    by_i, by_j = touched.any(axis=(0, 1)), touched.any(axis=(0, 2))
    assert nx <= 64 or by_i[64:].any()
    assert nx <= 128 or by_i[128:].any()
    assert ny <= 4 or by_j[4:].any()
    assert by_i[(nx - 1) // 64 * 64:].any() and by_j[(ny - 1) // 4 * 4:].any()
    assert (want[0] == 0).any() and want[0].max() >= 2.0
    once = want.copy()
    fuse_views_and_compare(cuda, D, grid, want, vol, rvol, hand_made_views(poses), kind)
    assert np.array_equal(want[0], 2 * once[0]), "a second pass over the same views accumulates"


def test_analytic_sphere_fused_and_extracted_past_one_chunk(cuda, D):
    import torch
    from spz_amd import abi
    # [-1.4, 1.4]^3 and 16 more layers below it, so that the sphere's top lies in the second chunk of the triangle scan
    dims, voxel = (81, 81, 97), 2.8 / 80
    lo = (-1.4, -1.4, -1.4 - 16 * voxel)
    n = dims[0] * dims[1] * dims[2]
    assert n > MR.SCAN_TILE * MR.SCAN_CHUNK
    vol = abi.tsdf_volume(lo, dims, voxel, 4 * voxel)
    rvol = MR.volume(lo, dims, voxel, 4 * voxel)
    grid = D.tsdf_alloc(vol, cuda)
    want = np.zeros((5, dims[2], dims[1], dims[0]), np.float32)
    for p, depth, image in sphere_views():
        D.tsdf_integrate(grid, vol, p, torch.from_numpy(depth).to(cuda), torch.from_numpy(image).to(cuda))
        MR.integrate(want, rvol, ref_view(p), depth, image)
    assert_grid_equal(grid, want)
    got = D.tsdf_extract(grid, vol)
    v, c, t, used, cubes = MR.extract(want, rvol, return_ids=True)
    tri_chunks, edge_chunks = MR.scan_chunk_counts(cubes, n), MR.scan_chunk_counts(used, 7 * n)
    assert len(tri_chunks) == 2 and tri_chunks.min() >= 1000 and (edge_chunks > 0).sum() >= 6, (tri_chunks, edge_chunks)
    assert_mesh_equal(got, (v, c, t), "the fused sphere")
    off = np.abs(np.linalg.norm(got[0].cpu().numpy().astype(np.float64), axis=1) - 1.0)
    print(f"{len(v)} vertices, {len(t)} triangles; triangles per chunk {tri_chunks.tolist()}, vertices per chunk "
          f"{edge_chunks.tolist()}; farthest vertex {off.max() / voxel:.3f} voxels from the sphere")
    assert len(v) > 10000
    assert off.max() <= 4 * voxel


# ---- the host form's box ---------------------------------------------------------------------------------------------
FIRST_TRIP = 4096 * 256      # the points the bounds kernel's launch covers before it strides
HALF_INF, HALF_NINF, HALF_NAN = 0x7C00, 0xFC00, 0x7E00


def volume_of(got):
    from spz_amd import abi
    v = got["volume"]
    return abi.tsdf_volume(v["lo"], v["dims"], v["voxel_size"], v["truncation"])


def check_box(got, pos, resolution):
    """The host form's volume against the box of the finite rows of the decoded positions `pos`."""
    pos = pos[np.isfinite(pos).all(axis=1)]
    v = got["volume"]
    assert np.array_equal(np.float32(v["lo"]), pos.min(axis=0))
    side = (pos.max(axis=0).astype(np.float64) - pos.min(axis=0)).max()
    assert v["voxel_size"] == np.float32(side / resolution) and v["truncation"] == np.float32(4 * (side / resolution))
    assert v["dims"] == MR.dims_from_box(pos.min(axis=0), pos.max(axis=0), side / resolution)


def orbit(spz, n):
    from spz_amd import abi
    return [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"])
            for v in spz.orbit_views(n, width=48, height=48, fov_y=50.0, center=[0.0, 0.0, 0.0], radius=1.0)]


def test_the_box_of_a_cloud_past_one_trip_of_the_bounds_loop(cuda, spz, D):
    from spz_amd import abi
    inner, outer = disc_cloud(FIRST_TRIP), disc_cloud(300)
    n = FIRST_TRIP + 300
    # the first trip's points on a sphere of radius 0.98, as small discs; the 300 behind them on the unit sphere
    cloud = {k: np.concatenate([inner[k], outer[k]]) for k in inner}
    cloud["positions"][:3 * FIRST_TRIP] *= np.float32(0.98)
    cloud["scales"][:3 * FIRST_TRIP] = np.tile(np.log(np.float32([0.004, 0.004, 0.0005])), FIRST_TRIP)
    stream = D.encode(D.to_device(cloud, cuda), n, 0, False, abi.RUB, 3)
    rc, h = D.peek_header(stream)
    assert rc == 0 and h.version == 3 and h.num_points == n
    pos = D.decode(stream, h, 0)["positions"].cpu().numpy().reshape(-1, 3)
    first, rest = pos[:FIRST_TRIP], pos[FIRST_TRIP:]
    assert (rest.min(axis=0) < first.min(axis=0)).all() and (rest.max(axis=0) > first.max(axis=0)).all(), \
        "an extreme coordinate is among the points of the first trip"
    views = orbit(spz, 3)
    got = D.mesh_packed(stream, h, views, resolution=24)
    check_box(got, pos, 24)
    totals = []

    def render(p):
        depth, image, total, status = D.render_depth_packed(stream, h, p, return_image=True, return_index=False,
                                                            return_info=True)
        totals.append(int(total))
        assert int(status) == 0
        return depth, image
    want = explicit_chain(D, render, views, volume_of(got))
    print(f"entries per view {totals}; {len(want[0])} vertices, {len(want[2])} triangles")
    assert len(totals) == 3 and max(totals) < 4_000_000
    assert len(want[0]) > 500 and len(want[2]) > 1000
    assert_mesh_equal((got["vertices"], got["colors"], got["triangles"]), want, "mesh_packed")


def v1_disc_stream(D, cuda, halfs_of):
    """A version-1 stream of the 300-disc cloud: its version-2 stream with the header's version set to 1 and the
    positions stored as float16, after halfs_of has edited the (300, 3) uint16 array.  Returns (stream, header)."""
    import torch
    from spz_amd import abi
    n = 300
    cloud = disc_cloud(n)
    v2 = D.encode(D.to_device(cloud, cuda), n, 0, False, abi.RUB, 2).cpu().numpy().tobytes()
    l1, l2 = abi.stream_layout(n, 0, 1), abi.stream_layout(n, 0, 2)
    assert list(l1.bytes)[1:] == list(l2.bytes)[1:] and l1.bytes_per_point[0] == 6
    halfs = cloud["positions"].astype(np.float16).view(np.uint16).reshape(n, 3).copy()
    halfs_of(halfs)
    raw = abi.write_header(1, n, 0) + halfs.astype("<u2").tobytes() + v2[l2.offset[abi.SEC_ALPHAS]:]
    assert len(raw) == l1.total_bytes
    rc, h = abi.peek_header(raw)
    assert rc == 0 and h.version == 1
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda), h


def test_the_box_leaves_out_non_finite_positions(cuda, spz, D):
    def some(halfs):
        halfs[5, 0], halfs[17, 1], halfs[40, 2] = HALF_INF, HALF_NINF, HALF_NAN
        halfs[77] = (HALF_NAN, HALF_INF, HALF_NINF)
        halfs[299, 0] = HALF_NAN          # the cloud's lowest z: a point with one non-finite axis is left out whole
        halfs[0, 1] = HALF_INF            # and its highest
    stream, h = v1_disc_stream(D, cuda, some)
    pos = D.decode(stream, h, 0)["positions"].cpu().numpy().reshape(-1, 3)
    finite = np.isfinite(pos).all(axis=1)
    assert (~finite).sum() == 6 and np.isposinf(pos[5, 0]) and np.isneginf(pos[17, 1]) and np.isnan(pos[40, 2])
    assert pos[299, 2] < pos[finite, 2].min() and pos[0, 2] > pos[finite, 2].max()
    views = orbit(spz, 6)
    got = D.mesh_packed(stream, h, views, resolution=24)
    check_box(got, pos, 24)

    def render(p):
        return D.render_depth_packed(stream, h, p, return_image=True, return_index=False)
    want = explicit_chain(D, render, views, volume_of(got))
    print(f"{len(want[0])} vertices, {len(want[2])} triangles")
    assert len(want[0]) > 500 and len(want[2]) > 1000
    assert_mesh_equal((got["vertices"], got["colors"], got["triangles"]), want, "mesh_packed of a v1 stream")


def test_the_golden_v1_stream_gives_the_box_of_its_finite_positions(cuda, spz, D):
    import torch
    from spz_amd import abi
    raw = load_golden("legacy.npz")["v1_stream"].tobytes()       # random bits: 35 of its 300 positions are not finite
    rc, h = abi.peek_header(raw)
    assert rc == 0 and h.version == 1
    stream = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    pos = D.decode(stream, h, 0)["positions"].cpu().numpy().reshape(-1, 3)
    assert 0 < (~np.isfinite(pos).all(axis=1)).sum() < len(pos)
    views = orbit(spz, 2)
    got = D.mesh_packed(stream, h, views, resolution=24)
    check_box(got, pos, 24)

    def render(p):
        return D.render_depth_packed(stream, h, p, return_image=True, return_index=False)
    want = explicit_chain(D, render, views, volume_of(got))
    assert_mesh_equal((got["vertices"], got["colors"], got["triangles"]), want, "mesh_packed of the golden v1 stream")


def test_a_stream_without_a_finite_position_is_refused(cuda, spz, D):
    from spz_amd import abi

    def every(halfs):
        halfs[:] = HALF_NAN
        halfs[::3, 0], halfs[1::3, 1] = HALF_INF, HALF_NINF      # no point is finite, though some of its axes are
        halfs[::3, 1:] = np.float16(0.5).view(np.uint16)
    stream, h = v1_disc_stream(D, cuda, every)
    pos = D.decode(stream, h, 0)["positions"].cpu().numpy().reshape(-1, 3)
    assert not np.isfinite(pos).all(axis=1).any() and np.isfinite(pos).any()
    views = orbit(spz, 2)
    with pytest.raises(abi.SpzAmdError) as e:
        D.mesh_packed(stream, h, views, resolution=24)
    assert e.value.status == abi.ERR_INVALID_ARG and e.value.view == -1
    # the C entry itself: no result is opened, the counts stay 0
    L = abi.load_library()
    arr = (abi.RenderParams * len(views))(*views)
    opts = abi.mesh_options(resolution=24)
    ctx, bad, counts = C.c_void_p(), C.c_int32(7), (C.c_uint64 * 2)(5, 5)
    rc = L.spz_amd_mesh_open(stream.data_ptr(), stream.numel(), C.byref(h), arr, len(views), C.byref(opts), 0,
                             C.byref(ctx), counts, None, None, C.byref(bad))
    assert rc == abi.ERR_INVALID_ARG and not ctx.value and list(counts) == [0, 0] and bad.value == -1
