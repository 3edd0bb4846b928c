"""The mesh feature without a GPU (DESIGN §8 "Mesh"): the volume's checks and sizes, the generated marching-tetrahedra
table, the argument checks of every device entry point, of spz.mesh_spz / spz.save_mesh_ply and of spz_mesh, the PLY
writer's round trip, and tests/mesh_ref.py itself on analytic fields."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import mesh_ref as MR
from conftest import ROOT


@pytest.fixture(scope="module")
def abi():
    from spz_amd import abi as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


def vol_of(abi, dims, lo=(0.0, 0.0, 0.0), s=1.0, t=4.0):
    v = abi.TsdfVolume()
    for a in range(3):
        v.lo[a], v.dims[a] = lo[a], dims[a]
    v.voxel_size, v.truncation = s, t
    return v


# ---- the volume ------------------------------------------------------------------------------------------------------
def test_volume_check_and_bytes_at_the_limits(abi):
    L = abi.load_library()
    ok = lambda v: L.spz_amd_tsdf_check(C.byref(v))
    size = lambda v: L.spz_amd_tsdf_bytes(C.byref(v))
    for dims, good in [((2, 2, 2), True), ((2048, 2, 2), True), ((2, 2048, 2), True), ((2, 2, 2048), True),
                       ((1, 2, 2), False), ((2, 1, 2), False), ((2, 2, 1), False), ((2049, 2, 2), False),
                       ((2, 2049, 2), False), ((2, 2, 2049), False), ((0, 2, 2), False),
                       ((1024, 512, 512), True),            # 2^28 lattice points
                       ((1024, 512, 513), False), ((2048, 2048, 65), False), ((2048, 2048, 64), True)]:
        v = vol_of(abi, dims)
        assert ok(v) == (abi.OK if good else abi.ERR_INVALID_ARG), dims
        assert size(v) == (20 * dims[0] * dims[1] * dims[2] if good else 0), dims
        assert (L.spz_amd_mesh_workspace_bytes(C.byref(v)) > 33 * dims[0] * dims[1] * dims[2]) == good, dims
    nan, inf = float("nan"), float("inf")
    for kw in [dict(s=0.0), dict(s=-1.0), dict(s=nan), dict(s=inf), dict(t=0.0), dict(t=-1.0), dict(t=nan), dict(t=inf),
               dict(lo=(nan, 0, 0)), dict(lo=(0, inf, 0)), dict(lo=(0, 0, -inf))]:
        v = vol_of(abi, (4, 4, 4), **kw)
        assert ok(v) == abi.ERR_INVALID_ARG and size(v) == 0, kw
    assert L.spz_amd_tsdf_check(None) == abi.ERR_INVALID_ARG and L.spz_amd_tsdf_bytes(None) == 0
    assert L.spz_amd_mesh_workspace_bytes(None) == 0
    with pytest.raises(ValueError, match="bad volume"):
        abi.tsdf_volume((0, 0, 0), (1, 2, 2), 1.0)
    v = abi.tsdf_volume((1, 2, 3), (4, 5, 6), 0.5)
    assert tuple(v.lo) == (1.0, 2.0, 3.0) and tuple(v.dims) == (4, 5, 6) and v.truncation == 2.0


def test_volume_from_box(abi):
    L = abi.load_library()
    cases = [((0, 0, 0), (1, 1, 1), 0.1), ((-1.37, -1.29, -1.46), (1.3, 1.2, 1.4), 0.1), ((0, 0, 0), (0, 0, 0), 1.0),
             ((0, 0, 0), (3.0, 2.999999, 3.000001), 1.0), ((-5, 2, 7), (5.5, 2.25, 7.1), 0.25)]
    for lo, hi, s in cases:
        v = abi.tsdf_volume_from_box(lo, hi, s, truncation=0.7)
        assert tuple(v.dims) == MR.dims_from_box(lo, hi, s), (lo, hi, s)
        assert tuple(v.dims) == tuple(int(np.floor((np.float64(h) - np.float64(l)) / s) + 2) for l, h in zip(lo, hi))
        assert tuple(v.lo) == tuple(np.float32(lo)) and v.voxel_size == np.float32(s) and v.truncation == np.float32(0.7)
        # the lattice reaches hi
        assert all(np.float64(l) + (d - 1) * s >= h - 1e-12 for l, h, d in zip(lo, hi, v.dims))
    assert abi.tsdf_volume_from_box((0, 0, 0), (1, 1, 1), 0.5).truncation == 2.0          # four voxels by default
    assert tuple(abi.tsdf_volume_from_box((0, 0, 0), (2046, 1, 1), 1.0).dims) == (2048, 3, 3)
    out = abi.TsdfVolume()
    d3 = C.c_double * 3
    call = lambda lo, hi, s, t=1.0, o=out: L.spz_amd_tsdf_volume_from_box(d3(*lo) if lo else None, d3(*hi) if hi else None,
                                                                        s, t, C.byref(o) if o is not None else None)
    assert call((0, 0, 0), (1, 1, 1), 0.5) == abi.OK
    nan = float("nan")
    for args in [(None, (1, 1, 1), 0.5), ((0, 0, 0), None, 0.5), ((0, 0, 0), (1, 1, 1), 0.0), ((0, 0, 0), (1, 1, 1), -1.0),
                 ((0, 0, 0), (1, 1, 1), nan), ((0, 0, 0), (1, 1, 1), 0.5, 0.0), ((0, 0, 0), (1, 1, 1), 0.5, nan),
                 ((0, 0, 0), (1, -1, 1), 0.5), ((0, nan, 0), (1, 1, 1), 0.5), ((0, 0, 0), (1, 1, float("inf")), 0.5),
                 ((0, 0, 0), (2047, 1, 1), 1.0),                       # 2049 points
                 ((0, 0, 0), (1023, 1023, 1023), 1.0)]:                # 2^30 points
        assert call(*args) == abi.ERR_INVALID_ARG, args
    assert call((0, 0, 0), (1, 1, 1), 0.5, 1.0, None) == abi.ERR_INVALID_ARG


# ---- the generated table ---------------------------------------------------------------------------------------------
def test_tet_table_equals_the_rule_restated(abi):
    corners, ntri, edges = abi.mesh_tet_table()
    rc, rn, re = MR.tet_table()
    assert np.array_equal(corners, rc) and np.array_equal(ntri, rn) and np.array_equal(edges, re)
    assert corners.tolist() == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]
    L = abi.load_library()
    assert L.spz_amd_mesh_tet_table(None, ntri.ctypes.data, edges.ctypes.data) == abi.ERR_INVALID_ARG


def test_tets_partition_the_cube(abi):
    corners, _, _ = abi.mesh_tet_table()
    pos = lambda c: MR.corner_xyz(int(c)).astype(np.float64)
    vols = []
    for t in range(6):
        p = np.array([pos(c) for c in corners[t]])
        vols.append(abs(np.linalg.det(p[1:] - p[0])) / 6.0)
    assert np.allclose(vols, 1.0 / 6.0, rtol=0, atol=1e-15)
    # every point of a grid of interior samples lies in exactly one tet (strictly inside: off the shared faces)
    rng = np.random.default_rng(3)
    for x in rng.uniform(0.01, 0.99, size=(500, 3)):
        inside = 0
        for t in range(6):
            p = np.array([pos(c) for c in corners[t]])
            bary = np.linalg.solve(np.vstack([p.T, np.ones(4)]), np.append(x, 1.0))
            inside += bool((bary > 1e-9).all())
        on_a_face = min(abs(x[0] - x[1]), abs(x[1] - x[2]), abs(x[0] - x[2])) < 1e-6
        assert inside == 1 or on_a_face


def test_face_diagonals_of_neighbouring_cubes_coincide(abi):
    corners, _, _ = abi.mesh_tet_table()
    # the tet edges of one cube that lie in a face, as point pairs of that face
    edges = set()
    for t in range(6):
        for a, b in MR.TET_EDGES:
            edges.add((int(corners[t][a]), int(corners[t][b])))
    for axis in range(3):
        bit = 1 << axis
        low = {(a, b) for a, b in edges if not a & bit and not b & bit}            # in the face x_axis = 0
        high = {(a & ~bit, b & ~bit) for a, b in edges if a & bit and b & bit}     # in the face x_axis = 1, moved down
        assert low == high, axis
        others = [1 << k for k in range(3) if k != axis]
        assert (0, others[0] | others[1]) in low and (others[0], others[1]) not in low   # the diagonal from the corner


def test_orientation_and_quads_for_all_masks(abi):
    corners, ntri, edges = abi.mesh_tet_table()
    assert not ntri[:, 0].any() and not ntri[:, 15].any()
    for t, m in itertools.product(range(6), range(1, 15)):
        pos = np.array([MR.corner_xyz(int(c)) for c in corners[t]], np.float64)
        mid = [(pos[a] + pos[b]) / 2 for a, b in MR.TET_EDGES]
        inside = [v for v in range(4) if (m >> v) & 1]
        outside = [v for v in range(4) if not (m >> v) & 1]
        n = int(ntri[t, m])
        assert n == (2 if len(inside) == 2 else 1)
        want = pos[outside].mean(axis=0) - pos[inside].mean(axis=0)
        normals = []
        for r in range(n):
            tri = [int(q) for q in edges[t, m, 3 * r: 3 * r + 3]]
            # only edges that cross the surface
            assert all((MR.TET_EDGES[q][0] in inside) != (MR.TET_EDGES[q][1] in inside) for q in tri)
            a, b, c = (mid[q] for q in tri)
            nrm = np.cross(b - a, c - a)
            assert np.dot(nrm, want) > 0, (t, m, r)
            normals.append(nrm / np.linalg.norm(nrm))
        if n == 2:
            t0 = [int(q) for q in edges[t, m, 0:3]]
            t1 = [int(q) for q in edges[t, m, 3:6]]
            assert sorted(set(t0) | set(t1)) == sorted(q for q, (a, b) in enumerate(MR.TET_EDGES)
                                                       if (a in inside) != (b in inside))
            shared = set(t0) & set(t1)
            assert len(shared) == 2                        # the quad's diagonal,
            d0 = [(t0[k], t0[(k + 1) % 3]) for k in range(3)]
            d1 = [(t1[k], t1[(k + 1) % 3]) for k in range(3)]
            assert len([e for e in d0 if (e[1], e[0]) in d1]) == 1      # walked in opposite directions,
            assert np.allclose(normals[0], normals[1])     # and with midpoints the four corners are coplanar


# ---- argument checks of the device entry points ------------------------------------------------------------------------
def good_params(abi):
    m = np.concatenate([np.eye(3), [[0.0], [0.0], [3.0]]], axis=1)
    return abi.render_params(m, 60.0, 60.0, 32.0, 24.0, 64, 48, coord=abi.RUB)


def test_device_entry_points_check_their_arguments_first(abi):
    import torch
    L = abi.load_library()
    v = vol_of(abi, (4, 4, 4))
    bad_v = vol_of(abi, (1, 4, 4))
    p = good_params(abi)
    bad_p = abi.RenderParams.from_buffer_copy(p)
    bad_p.fx = -1.0
    buf = np.zeros(1 << 16, np.uint8).ctypes.data     # never read: no device work is reached with a bad argument
    last = abi.OK if torch.cuda.is_available() else abi.ERR_NO_DEVICE

    def integrate(vol=v, grid=buf, params=p, depth=buf, image=buf, kind=abi.MESH_DEPTH_MEDIAN, min_alpha=0.5):
        return L.spz_amd_tsdf_integrate_device(C.byref(vol) if vol is not None else None, grid,
                                               C.byref(params) if params is not None else None, depth, image, kind,
                                               min_alpha, None)
    for kw in [dict(vol=None), dict(vol=bad_v), dict(grid=None), dict(params=None), dict(params=bad_p), dict(depth=None),
               dict(image=None), dict(kind=2), dict(kind=-1), dict(min_alpha=float("nan")), dict(min_alpha=-0.1),
               dict(min_alpha=1.5)]:
        assert integrate(**kw) == abi.ERR_INVALID_ARG, kw

    def count(vol=v, grid=buf, min_weight=1.0, counts=buf, ws=buf):
        return L.spz_amd_mesh_count_device(C.byref(vol) if vol is not None else None, grid, min_weight, counts, ws, None)
    for kw in [dict(vol=None), dict(vol=bad_v), dict(grid=None), dict(counts=None), dict(ws=None), dict(min_weight=0.0),
               dict(min_weight=-1.0), dict(min_weight=float("nan")), dict(min_weight=float("inf"))]:
        assert count(**kw) == abi.ERR_INVALID_ARG, kw

    def emit(vol=v, grid=buf, nv=3, nt=1, cap_v=3, cap_t=1, pos=buf, col=buf, tri=buf, ws=buf):
        return L.spz_amd_mesh_emit_device(C.byref(vol) if vol is not None else None, grid, nv, nt, cap_v, cap_t, pos, col,
                                          tri, ws, None)
    for kw in [dict(vol=None), dict(vol=bad_v), dict(grid=None), dict(ws=None), dict(pos=None), dict(col=None),
               dict(tri=None), dict(nv=7 * 64 + 1), dict(nt=12 * 64 + 1)]:
        assert emit(**kw) == abi.ERR_INVALID_ARG, kw
    assert emit(cap_v=2) == abi.ERR_CAPACITY and emit(cap_t=0) == abi.ERR_CAPACITY
    if last == abi.ERR_NO_DEVICE:
        assert integrate() == last and count() == last and emit() == last      # the device: last of all


def test_mesh_open_checks_options_views_and_input_before_the_device(abi):
    import torch
    L = abi.load_library()
    h = abi.Header()
    h.num_points, h.sh_degree, h.version, h.fractional_bits = 10, 0, 3, 12
    buf = (C.c_uint8 * 4096)()
    good = good_params(abi)

    def call(views, opts=None, stream=buf, hdr=h, counts=True):
        o = opts if opts is not None else abi.mesh_options()
        arr = (abi.RenderParams * max(1, len(views)))(*views)
        ctx, bad, n = C.c_void_p(), C.c_int32(7), (C.c_uint64 * 2)()
        rc = L.spz_amd_mesh_open(stream, 4096, C.byref(hdr), arr, len(views), C.byref(o), 0, C.byref(ctx),
                                 n if counts else None, None, None, C.byref(bad))
        assert not ctx.value
        return rc, bad.value

    assert call([]) == (abi.ERR_INVALID_ARG, -1)
    assert call([good] * 1025) == (abi.ERR_INVALID_ARG, -1)
    worse = abi.RenderParams.from_buffer_copy(good)
    worse.fx = -1.0
    assert call([good, good, worse]) == (abi.ERR_INVALID_ARG, 2)
    other = abi.RenderParams.from_buffer_copy(good)
    other.coord = abi.RDF
    assert call([good, other]) == (abi.ERR_INVALID_ARG, 1)
    assert call([good], stream=None) == (abi.ERR_INVALID_ARG, -1)
    assert call([good], counts=False) == (abi.ERR_INVALID_ARG, -1)
    for field, value in [("resolution", 0), ("resolution", 2047), ("voxel_size", -1.0), ("voxel_size", float("nan")),
                         ("truncation", -1.0), ("depth_kind", 2), ("min_alpha", 2.0), ("min_weight", 0.0)]:
        o = abi.mesh_options()
        if field == "voxel_size":
            o.resolution = 0
        setattr(o, field, value)
        assert call([good], opts=o) == (abi.ERR_INVALID_ARG, -1), (field, value)
    both = abi.mesh_options()
    both.voxel_size = 0.1                                              # with the default resolution: not exactly one
    assert call([good], opts=both) == (abi.ERR_INVALID_ARG, -1)
    box = abi.mesh_options(box=(0, 0, 0, 1, 1, 1))
    box.box[3] = 0.0
    assert call([good], opts=box) == (abi.ERR_INVALID_ARG, -1)
    big = abi.Header.from_buffer_copy(h)
    big.num_points = 0x80000000
    assert call([good], hdr=big)[0] == abi.ERR_TOO_MANY_POINTS
    big.version = 4
    assert call([good], hdr=big)[0] == abi.ERR_VERSION
    if not torch.cuda.is_available():
        assert call([good]) == (abi.ERR_NO_DEVICE, -1)
    assert L.spz_amd_mesh_fetch(None, None, None, None) == abi.ERR_INVALID_ARG
    L.spz_amd_mesh_close(None)


def test_mesh_options_helper(abi):
    o = abi.mesh_options()
    assert o.resolution == 256 and o.voxel_size == 0.0 and o.depth_kind == abi.MESH_DEPTH_MEDIAN
    assert o.min_alpha == 0.5 and o.min_weight == 1.0 and not o.has_box and o.truncation == 0.0
    o = abi.mesh_options(voxel_size=0.25, depth="expected", box=(0, 0, 0, 1, 2, 3), truncation=0.5)
    assert o.resolution == 0 and o.voxel_size == 0.25 and o.depth_kind == abi.MESH_DEPTH_EXPECTED and o.has_box
    assert list(o.box) == [0, 0, 0, 1, 2, 3] and o.truncation == 0.5
    for kw, msg in [(dict(voxel_size=0.1, resolution=8), "exclude each other"), (dict(resolution=0), "1..2046"),
                    (dict(resolution=True), "1..2046"), (dict(depth="mean"), "'median' or 'expected'"),
                    (dict(box=(0, 0, 0, 1, 1)), "box must be"), (dict(box=(0, 0, 0, 1, 1, 0)), "refused options"),
                    (dict(min_alpha=1.5), "refused options"), (dict(min_weight=0), "refused options"),
                    (dict(voxel_size=-1), "refused options"), (dict(voxels=3), "unknown option")]:
        with pytest.raises(ValueError, match=msg):
            abi.mesh_options(**kw)


# ---- spz.mesh_spz and spz.save_mesh_ply: (call, type, whole message) ---------------------------------------------------
IN = "/nonexistent/in.spz"
EYE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
VIEW = dict(world_to_camera=EYE, fx=1.0, fy=1.0, cx=1.0, cy=1.0, width=2, height=2)
V3 = np.zeros((3, 3), np.float32)
T1 = np.array([[0, 1, 2]], np.uint32)
BOX = "box must be six finite numbers x0, y0, z0, x1, y1, z1 with x1 > x0, y1 > y0, z1 > z0"
BAD_CAMERA = ("bad camera: world_to_camera must be [R | t] with R a rotation (to 1e-4), fx, fy > 0, width and height in "
              "1..16384, near_plane > 0, values finite")

ROWS = [
    ("mesh_spz(IN, [VIEW], voxel_size=0.1, resolution=8)", ValueError, "give voxel_size or resolution, not both"),
    ("mesh_spz(IN, [VIEW], voxel_size=0)", ValueError, "voxel_size must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], voxel_size=-1.0)", ValueError, "voxel_size must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], voxel_size=inf)", ValueError, "voxel_size must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], voxel_size=True)", ValueError, "voxel_size must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], voxel_size='1')", ValueError, "voxel_size must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], resolution=0)", ValueError, "resolution must be an int in 1..2046"),
    ("mesh_spz(IN, [VIEW], resolution=2047)", ValueError, "resolution must be an int in 1..2046"),
    ("mesh_spz(IN, [VIEW], resolution=8.0)", ValueError, "resolution must be an int in 1..2046"),
    ("mesh_spz(IN, [VIEW], resolution=True)", ValueError, "resolution must be an int in 1..2046"),
    ("mesh_spz(IN, [VIEW], truncation=0)", ValueError, "truncation must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], truncation=nan)", ValueError, "truncation must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], truncation=True)", ValueError, "truncation must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], depth='mean')", ValueError, "depth must be 'median' or 'expected'"),
    ("mesh_spz(IN, [VIEW], min_alpha=-0.1)", ValueError, "min_alpha must be a number in [0, 1]"),
    ("mesh_spz(IN, [VIEW], min_alpha=1.1)", ValueError, "min_alpha must be a number in [0, 1]"),
    ("mesh_spz(IN, [VIEW], min_alpha=True)", ValueError, "min_alpha must be a number in [0, 1]"),
    ("mesh_spz(IN, [VIEW], min_weight=0)", ValueError, "min_weight must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], min_weight=inf)", ValueError, "min_weight must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], min_weight=True)", ValueError, "min_weight must be a finite number > 0"),
    ("mesh_spz(IN, [VIEW], box=(0, 0, 0, 1, 1))", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], box=(0, 0, 0, 1, 1, 0))", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], box=(0, 0, 0, 1, 1, nan))", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], box='abcdef')", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], box=(0, 0, 0, 1, 1, True))", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], box=7)", ValueError, BOX),
    ("mesh_spz(IN, [VIEW], near=0.0)", ValueError, "near must be > 0"),
    ("mesh_spz(IN, [VIEW], near=nan)", ValueError, "near must be > 0"),
    ("mesh_spz(IN, VIEW)", ValueError, "views must be a sequence of view dicts (orbit_views, load_3dgs_cameras)"),
    ("mesh_spz(IN, [])", ValueError, "give 1..1024 views, got 0"),
    ("mesh_spz(IN, [VIEW] * 1025)", ValueError, "give 1..1024 views, got 1025"),
    ("mesh_spz(IN, [VIEW, dict(VIEW, fx=0.0)])", ValueError, "view 1: " + BAD_CAMERA),
    ("mesh_spz(IN, [VIEW, 3])", ValueError, "view 1: must be a dict (world_to_camera, fx, fy, cx, cy, width, height)"),
    ("mesh_spz(IN, [dict(VIEW, coord=RDF)])", ValueError,
     "view 0: its coord differs from the prune's coord (every view is in one frame)"),
    ("mesh_spz(IN, [VIEW])", RuntimeError, "mesh_spz failed (see the [SPZ ERROR] line)"),
    ("mesh_spz(b'not a file', [VIEW])", RuntimeError, "mesh_spz failed (see the [SPZ ERROR] line)"),
    ("save_mesh_ply(OUT, [[0, 0, 0]], V3, T1)", ValueError, "vertices must be a numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, np.zeros(9, np.float32), V3, T1)", ValueError, "vertices must be a numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, V3, np.zeros((3, 4), np.float32), T1)", ValueError,
     "colors must be a numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, V3, np.zeros((2, 3), np.float32), T1)", ValueError, "colors must have one row per vertex"),
    ("save_mesh_ply(OUT, V3, V3, np.zeros((1, 3), np.float32))", ValueError,
     "triangles must be an integer numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, V3, V3, np.zeros(3, np.uint32))", ValueError,
     "triangles must be an integer numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, V3, V3, [[0, 1, 2]])", ValueError, "triangles must be an integer numpy array of shape (n, 3)"),
    ("save_mesh_ply(OUT, V3, V3, np.array([[0, 1, 3]]))", ValueError,
     "save_mesh_ply: refused (see the [SPZ ERROR] line)"),
    ("save_mesh_ply(OUT, V3, V3, np.array([[0, 1, -1]]))", ValueError,
     "save_mesh_ply: refused (see the [SPZ ERROR] line)"),
]


@pytest.mark.parametrize("call,kind,message", ROWS, ids=[r[0] for r in ROWS])
def test_python_argument_errors(spz, tmp_path, call, kind, message):
    names = {k: getattr(spz, k) for k in dir(spz) if not k.startswith("_")}
    names.update(np=np, IN=IN, OUT=str(tmp_path / "out.ply"), VIEW=VIEW, V3=V3, T1=T1, inf=float("inf"), nan=float("nan"))
    with pytest.raises(kind) as e:
        eval(call, names)
    assert type(e.value) is kind and str(e.value) == message
    assert not os.path.exists(names["OUT"])


# ---- the PLY writer --------------------------------------------------------------------------------------------------
def read_mesh_ply(path):
    """(header text, vertices (n, 3) f32, rgb (n, 3) u8, triangles (m, 3) u32) of a PLY as save_mesh_ply writes it."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii")
    lines = head.split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nt = int([l for l in lines if l.startswith("element face")][0].split()[2])
    vt = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("n", "u1"), ("idx", "<u4", 3)])
    assert vt.itemsize == 15 and ft.itemsize == 13 and len(raw) == end + 15 * nv + 13 * nt
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nt, end + 15 * nv)
    assert (f["n"] == 3).all()
    return head, v["xyz"].copy(), v["rgb"].copy(), f["idx"].copy()


def test_save_mesh_ply_round_trip(spz, tmp_path):
    rng = np.random.default_rng(11)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    v[0] = [-0.0, 1e-40, 3.4e38]
    c = np.array([[0.0, 1.0, 0.5], [-0.2, 1.2, 0.25], [0.5 / 255, 1.5 / 255, 2.5 / 255], [0.999, 0.001, 0.498],
                  [float("nan"), float("inf"), -float("inf")], [254.5 / 255, 253.5 / 255, 0.7], [0.1, 0.2, 0.3]], np.float32)
    t = np.array([[0, 1, 2], [2, 1, 6], [6, 5, 4]], np.int64)
    path = str(tmp_path / "m.ply")
    assert spz.save_mesh_ply(path, v, c, t) is None
    head, gv, gc, gt = read_mesh_ply(path)
    assert head == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\n"
                    "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 3\n"
                    "property list uchar uint vertex_indices\nend_header\n")
    assert np.array_equal(gv.view(np.uint32), v.view(np.uint32))
    with np.errstate(invalid="ignore"):
        clamped = np.where(c >= 0, np.minimum(c, np.float32(1)), np.float32(0)).astype(np.float32)    # NaN -> 0
    want = np.rint(np.float32(255) * clamped).astype(np.uint8)          # rint: ties to even, in float32
    assert np.array_equal(gc, want)
    assert gc[2].tolist() == [0, 2, 2] and gc[4].tolist() == [0, 255, 0]
    assert np.array_equal(gt, t.astype(np.uint32))
    # an empty mesh is a header alone
    e = str(tmp_path / "e.ply")
    spz.save_mesh_ply(e, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    head, gv, gc, gt = read_mesh_ply(e)
    assert "element vertex 0\n" in head and "element face 0\n" in head and len(gv) == 0 and len(gt) == 0
    with pytest.raises(RuntimeError, match="save_mesh_ply: .* failed"):
        spz.save_mesh_ply(str(tmp_path / "no" / "dir" / "m.ply"), v, c, t)


# ---- the tool --------------------------------------------------------------------------------------------------------
def test_spz_mesh_usage_errors_and_a_missing_input(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_mesh")
    views = tmp_path / "v.txt"
    views.write_text("64 48 50 50 32 24 1 0 0 0 0 1 0 0 0 0 1 5\n")
    out = str(tmp_path / "out.ply")
    base = [str(tmp_path / "missing.spz"), out]
    vf = ["--views", str(views)]
    orbit = ["--orbit", "4", "--size", "64", "48", "--fov-y", "50", "--center", "0", "0", "0", "--radius", "1"]
    for args in [[], base[:1], base, base + vf + ["--voxel", "0.1", "--resolution", "64"], base + vf + ["--voxel", "0"],
                 base + vf + ["--voxel", "abc"], base + vf + ["--resolution", "0"], base + vf + ["--resolution", "2047"],
                 base + vf + ["--resolution", "64.0"], base + vf + ["--box", "0", "0", "0", "1", "1"],
                 base + vf + ["--box", "0", "0", "0", "1", "1", "0"], base + vf + ["--box", "0", "0", "0", "1", "1", "nan"],
                 base + vf + ["--truncation", "0"], base + vf + ["--depth", "mean"], base + vf + ["--min-alpha", "1.5"],
                 base + vf + ["--min-weight", "0"], base + vf + ["--near", "0"], base + vf + ["--coord", "XYZ"],
                 base + vf + ["--voxel", "0.1", "--voxel", "0.2"], base + vf + ["--keep", "3"],
                 base + vf + orbit, base + orbit[:2], base + ["--orbit", "4", "--size", "64", "48"],
                 ["--views", str(views), out], base + ["--views", str(tmp_path / "none.txt")]]:
        r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: spz_mesh <in.spz> <out.ply>" in r.stderr, (args, r.stdout, r.stderr)
        assert not os.path.exists(out)
    # a well-formed line whose input is missing fails, and is not a usage error
    for args in [base + vf, base + vf + ["--resolution", "32", "--depth", "expected", "--min-alpha", "0.3"],
                 base + orbit + ["--voxel", "0.05", "--box", "-1", "-1", "-1", "1", "1", "1", "--coord", "RUB"]]:
        r = subprocess.run([tool, *args], capture_output=True, text=True, timeout=60)
        said = r.stdout + r.stderr
        assert r.returncode == 1 and "Usage" not in said and "missing.spz" in said, (args, said)
        assert not os.path.exists(out)
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "spz_mesh" in r.stderr


# ---- mesh_ref itself on analytic fields --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analytic():
    return {name: MR.extract(g, vol) + (g, vol) for name, (g, vol) in MR.analytic_grids().items()}


def check_closed_and_oriented(v, t, euler):
    und, dire = MR.edge_counts(t)
    assert set(und.values()) == {2}, "every undirected edge in exactly two triangles"
    assert set(dire.values()) == {1}, "every directed edge once"
    assert MR.euler_characteristic(len(v), t) == euler
    assert np.array_equal(np.unique(t), np.arange(len(v))), "every vertex referenced"


def test_ref_sphere(analytic):
    v, c, t, _, _ = analytic["sphere"]
    assert (len(v), len(t)) == (2534, 5064)
    check_closed_and_oriented(v, t, 2)
    n = MR.triangle_normals(v, t)
    out = v[t].astype(np.float64).mean(axis=1) - np.array(MR.SPHERE_C)
    assert ((n * out).sum(axis=1) > 0).all(), "all normals point outward"
    r = np.linalg.norm(v.astype(np.float64) - np.array(MR.SPHERE_C), axis=1)
    assert np.abs(r - MR.SPHERE_R).max() < 0.1            # linear interpolation of a distance field on a unit lattice
    # the colour is the interpolated field x / 20, y / 18, z / 22: linear, so exact to rounding
    assert np.allclose(c, v / np.array(MR.FIELD_DIMS, np.float32), atol=1e-6)
    assert v.dtype == np.float32 and c.dtype == np.float32 and t.dtype == np.uint32


def test_ref_torus(analytic):
    v, _, t, _, _ = analytic["torus"]
    check_closed_and_oriented(v, t, 0)


def test_ref_half_valid_sphere(analytic):
    v, _, t, g, vol = analytic["half_sphere"]
    und, dire = MR.edge_counts(t)
    assert set(und.values()) == {1, 2} and set(dire.values()) == {1}
    assert MR.euler_characteristic(len(v), t) == 1
    assert np.array_equal(np.unique(t), np.arange(len(v))), "no unreferenced vertex"
    assert v[:, 0].max() <= 9.0, "no triangle in a cube with an invalid corner"
    boundary = np.array([e for e, k in und.items() if k == 1])
    assert (v[boundary.reshape(-1), 0] == 9.0).all(), "boundary edges only where the valid half ends"


def test_ref_plane_through_lattice_points(analytic):
    v, _, t, _, _ = analytic["plane"]
    assert t.max() < len(v) and np.array_equal(np.unique(t), np.arange(len(v)))
    assert (v[:, 0] == 7.0).all()
    area = 0.5 * np.linalg.norm(MR.triangle_normals(v, t), axis=1)
    assert area.sum() == 17 * 21
    assert (area == 0).any(), "zero-area triangles are present, and kept"
    n = MR.triangle_normals(v, t)
    assert (n[area > 0][:, 0] > 0).all()                   # f = x - 7: inside is x < 7, the normal points to +x
    assert MR.euler_characteristic(len(v), t) == 1


@pytest.mark.parametrize("name", ["sphere", "torus", "half_sphere", "plane"])
def test_ref_extract_ids_reproduce_the_mesh(analytic, name):
    v, c, t, g, vol = analytic[name]
    got = MR.extract(g, vol, return_ids=True)
    assert len(got) == 5 and all(np.array_equal(a, b) for a, b in zip(got[:3], (v, c, t))), "the mesh itself is unchanged"
    used, cubes = got[3], got[4]
    nx, ny, nz = vol["dims"]
    # a vertex per edge id, ascending; the vertex from the id alone: a = id // 7, the direction id % 7 + 1
    assert used.shape == (len(v),) and (np.diff(used) > 0).all() and used.min() >= 0 and used.max() < 7 * nx * ny * nz
    a, code = used // 7, used % 7 + 1
    delta = np.stack([code & 1, (code >> 1) & 1, (code >> 2) & 1], axis=1)
    b = a + delta[:, 0] + delta[:, 1] * nx + delta[:, 2] * nx * ny
    with np.errstate(all="ignore"):
        f = (g[1].reshape(-1) / g[0].reshape(-1)).astype(np.float32).astype(np.float64)
    assert ((f[a] < 0) != (f[b] < 0)).all(), "an edge of the list does not cross the surface"
    s = f[a] / (f[a] - f[b])
    at = np.stack([a % nx, (a // nx) % ny, a // (nx * ny)], axis=1)
    assert np.array_equal(v, (at + s[:, None] * delta).astype(np.float32))          # lo = 0, unit spacing
    # a cube per triangle, ascending; its three edges join corners of that cube
    assert cubes.shape == (len(t),) and (np.diff(cubes) >= 0).all()
    corner = lambda p: np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], axis=-1)   # noqa: E731
    for end in (a, b):
        off = corner(end[t.astype(np.int64)]) - corner(cubes)[:, None, :]
        assert ((off == 0) | (off == 1)).all()
    inside = f.reshape(nz, ny, nx) < 0
    ok = (g[0] >= 1).reshape(nz, ny, nx)
    some, every, valid = (np.zeros((nz - 1, ny - 1, nx - 1), bool), np.ones((nz - 1, ny - 1, nx - 1), bool),
                          np.ones((nz - 1, ny - 1, nx - 1), bool))
    for dz, dy, dx in itertools.product(range(2), repeat=3):
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        some, every, valid = some | inside[sl], every & inside[sl], valid & ok[sl]
    k, j, i = np.nonzero(valid & some & ~every)
    assert np.array_equal(np.unique(cubes), (k * ny + j) * nx + i), "the cubes the surface crosses, each with a triangle"


@pytest.mark.parametrize("name", ["sphere", "torus", "half_sphere", "plane"])
def test_ref_edge_multiplicity_equals_edge_counts(analytic, name):
    _, _, t, _, _ = analytic[name]
    und, dire = MR.edge_counts(t)
    edges, per_edge, per_directed = MR.edge_multiplicity(t)
    assert {(int(a), int(b)): int(k) for (a, b), k in zip(edges, per_edge)} == und
    assert sorted(per_directed.tolist()) == sorted(dire.values())
    assert len(edges) == len(t) + (t.max() + 1) - MR.euler_characteristic(t.max() + 1, t)
    e, u, d = MR.edge_multiplicity(np.zeros((0, 3), np.uint32))
    assert e.shape == (0, 2) and len(u) == 0 and len(d) == 0


def test_ref_scan_chunks_and_field_color():
    assert (MR.SCAN_TILE, MR.SCAN_CHUNK) == (2048, 256)
    assert [MR.scan_blocks(n) for n in (1, 2048, 2049, 524288, 524289, 7 * 524288, 638685, 7 * 638685)] == \
        [1, 1, 2, 256, 257, 1792, 312, 2184]
    assert MR.scan_chunk_counts([0, 524287, 524288, 638684], 638685).tolist() == [2, 2]
    assert MR.scan_chunk_counts([524287], 524288).tolist() == [1]
    assert MR.scan_chunk_counts([], 7 * 638685).tolist() == [0] * 9
    assert MR.scan_chunk_counts([8 * 524288], 7 * 638685).tolist() == [0] * 8 + [1]
    for bad in ([-1], [524288]):
        with pytest.raises(AssertionError):
            MR.scan_chunk_counts(bad, 524288)
    x, y, z = MR.field_coords()
    assert np.array_equal(MR.field_color(), np.stack([x / 20.0, y / 18.0, z / 22.0]).astype(np.float32))
    assert MR.field_color((5, 3, 2)).shape == (3, 2, 3, 5) and MR.field_color((5, 3, 2)).max() == np.float32(0.8)


def test_ref_integrate_on_a_wall():
    """One view looking down +z at a wall at depth 2: W counts the views, S / W is the truncated signed distance along
    z, and occluded, out-of-frustum and near-clipped points are not written."""
    vol = MR.volume((-0.05, -0.05, 0.05), (2, 2, 40), 0.1, 0.4)      # narrow: every point projects into the image
    g = np.zeros((5, 40, 2, 2), np.float32)
    view = {"world_to_camera": np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), "fx": 60.0, "fy": 60.0, "cx": 32.0,
            "cy": 24.0, "width": 64, "height": 48, "near": 0.2}
    depth = np.full((48, 64, 2), 2.0, np.float32)
    image = np.full((48, 64, 4), 0.25, np.float32)
    image[..., 3] = 1.0
    depth[..., 0] = 2.0
    ok = MR.integrate(g, vol, view, depth, image, MR.MEDIAN)
    z = MR.lattice_points(vol)[..., 2]
    assert not ok[z <= 0.2].any() and not ok[z > 2.4 + 1e-9].any() and ok[(z > 0.2) & (z < 2.4 - 1e-9)].all()
    assert np.array_equal(g[0], ok.astype(np.float32))
    want = np.minimum(1.0, (2.0 - z) / np.float64(np.float32(0.4)))
    assert np.allclose(g[1][ok], want[ok], atol=1e-6) and np.array_equal(g[2][ok], np.full(ok.sum(), 0.25, np.float32))
    before = g.copy()
    MR.integrate(g, vol, view, depth, image, MR.EXPECTED, min_alpha=0.5)
    assert np.array_equal(g[0], 2 * before[0]) and np.array_equal(g[1], 2 * before[1])
    image[..., 3] = 0.4
    kept = g.copy()
    assert not MR.integrate(g, vol, view, depth, image, MR.EXPECTED, min_alpha=0.5).any() and np.array_equal(g, kept)
    v, c, t = MR.extract(g, vol)
    assert len(t) > 0 and np.allclose(v[:, 2], 2.0, atol=1e-5) and np.allclose(c, 0.25)
