"""The host-only parts of the plane contract (include/spz_amd.h "plane", DESIGN §8 "Level") against the restatement of
tests/plane_ref.py: the option check, the threshold, the seeded hypotheses, the solve, the levelling placement in every
coordinate system, and spz_level's argument errors.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import plane_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from spz_amd import abi
    return abi.load_library()


def options(lib, **kw):
    from spz_amd import abi
    o = abi.PlaneOptions()
    assert lib.spz_amd_plane_default_options(C.byref(o)) == abi.OK
    o.threshold = 0.01
    for k, v in kw.items():
        if k in ("axis", "up_hint"):
            getattr(o, k)[:] = v
        else:
            setattr(o, k, v)
    return o


def test_default_options(lib):
    from spz_amd import abi
    o = abi.PlaneOptions()
    assert lib.spz_amd_plane_default_options(C.byref(o)) == abi.OK
    assert (o.hypotheses, o.refine, o.max_planes, o.stride, o.seed, o.min_inliers) == (4096, 3, 1, 1, 0, 0)
    assert (o.has_axis, o.has_up_hint, o.coord, o.no_translate) == (0, 0, 0, 0)
    assert math.isnan(o.threshold), "tau has no default"
    assert lib.spz_amd_plane_check(C.byref(o)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_default_options(None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_check(None) == abi.ERR_INVALID_ARG


@pytest.mark.parametrize("kw, ok", [
    ({}, True), ({"threshold": 0.0}, True), ({"threshold": -1e-9}, False), ({"threshold": math.inf}, False),
    ({"threshold": math.nan}, False),
    ({"hypotheses": 1}, True), ({"hypotheses": 65536}, True), ({"hypotheses": 0}, False), ({"hypotheses": 65537}, False),
    ({"refine": 0}, True), ({"refine": 16}, True), ({"refine": 17}, False),
    ({"max_planes": 255}, True), ({"max_planes": 0}, False), ({"max_planes": 256}, False),
    ({"stride": 0}, False), ({"stride": 0xFFFFFFFF}, True),
    ({"has_axis": 1, "axis": (0.0, 2.0, 0.0), "max_tilt": 10.0}, True), ({"has_axis": 1, "axis": (0.0, 0.0, 0.0)}, False),
    ({"has_axis": 1, "axis": (0.0, math.nan, 1.0)}, False), ({"has_axis": 0, "axis": (0.0, 0.0, 0.0)}, True),
    ({"has_up_hint": 1, "up_hint": (0.0, 0.0, 0.0)}, False), ({"has_up_hint": 1, "up_hint": (math.inf, 0.0, 0.0)}, False),
    ({"has_up_hint": 1, "up_hint": (0.0, -1.0, 0.0)}, True),
    ({"max_tilt": 0.0}, True), ({"max_tilt": 90.0}, True), ({"max_tilt": 90.5}, False), ({"max_tilt": -1.0}, False),
    ({"max_tilt": math.nan}, False),
    ({"coord": 8}, True), ({"coord": 9}, False), ({"coord": -1}, False),
])
def test_plane_check_rows(lib, kw, ok):
    from spz_amd import abi
    assert lib.spz_amd_plane_check(C.byref(options(lib, **kw))) == (abi.OK if ok else abi.ERR_INVALID_ARG)


def test_threshold_edges(lib):
    from spz_amd import abi
    T = C.c_uint64(77)

    def call(tau, f):
        rc = lib.spz_amd_plane_threshold(tau, f, C.byref(T))
        return T.value if rc == abi.OK else None

    assert call(0.0, 12) == 0
    assert call(2.0 ** -29, 12) == 0 and call(2.0 ** -28, 12) == 1            # one unit of 2^-(f+16)
    assert call(256.0, 12) == 1 << 36                                          # T = 2^36 exactly
    assert call(math.nextafter(256.0, 0.0), 12) == (1 << 36) - 1
    assert call(256.0 + 2.0 ** -28, 12) is None                                # one above
    assert call(2.0 ** 20, 0) == 1 << 36 and call(2.0 ** 20 + 1.0, 0) is None
    assert call(2.0 ** -4, 24) == 1 << 36
    assert call(0.05, 12) == math.floor(0.05 * 2.0 ** 28) == R.threshold(0.05, 12)
    for tau in (-0.0, 1e-300):
        assert call(tau, 12) == 0
    for tau in (-1e-12, math.nan, math.inf):
        assert call(tau, 12) is None and R.threshold(tau, 12) is None
    assert call(0.1, 25) is None and call(0.1, -1) is None
    assert lib.spz_amd_plane_threshold(0.1, 12, None) == abi.ERR_INVALID_ARG


def test_mix64_is_splitmix64s_finaliser():
    # the first outputs of splitmix64 seeded with 0: mix64 of the running sum of the golden gamma
    gamma = 0x9E3779B97F4A7C15
    assert [R.mix64(gamma * k) for k in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def lib_hypotheses(lib, seed, r, H, m, points=None, axis=None, max_tilt=0.0):
    from spz_amd import abi
    idx = np.zeros(3 * H, np.uint32)
    planes = (abi.Plane * H)()
    pts = None if points is None else np.ascontiguousarray(points, np.int32)
    ax = None if axis is None else (C.c_double * 3)(*axis)
    rc = lib.spz_amd_plane_hypotheses(seed, r, H, m, None if pts is None else pts.ctypes.data, ax, max_tilt,
                                      idx.ctypes.data, planes if pts is not None else None)
    assert rc == abi.OK
    return idx.reshape(H, 3).tolist(), [(p.a, p.b, p.c, p.e) for p in planes]


@pytest.mark.parametrize("seed, r, m", [(0, 0, 1000), (1, 0, 3), (12345678901234567890, 2, 9_999_999),
                                        ((1 << 64) - 1, 254, 7), (42, 1, 1)])
def test_hypothesis_indices(lib, seed, r, m):
    got, _ = lib_hypotheses(lib, seed, r, 257, m)
    assert got == R.sample_indices(seed, r, 257, m)
    assert all(0 <= i < m for t in got for i in t)


CORNER = 1 << 23
# recorded triples: (what, P0, P1, P2); the answers are the restatement's, compared exactly
TRIPLES = [
    ("axis plane", (0, 5, 0), (100, 5, 0), (0, 5, 100)),
    ("tilted", (10, 20, 30), (1010, 25, 33), (12, 21, 1030)),
    ("collinear", (0, 0, 0), (10, 10, 10), (-30, -30, -30)),
    ("repeated point", (7, 7, 7), (7, 7, 7), (1, 2, 3)),
    ("cube corners", (-CORNER, -CORNER, -CORNER), (CORNER - 1, -CORNER, CORNER - 1), (-CORNER, CORNER - 1, CORNER - 1)),
    ("cube corners 2", (CORNER - 1, CORNER - 1, -CORNER), (-CORNER, CORNER - 1, CORNER - 1), (CORNER - 1, -CORNER, CORNER - 1)),
    ("tiny", (0, 0, 0), (1, 0, 0), (0, 0, 1)),
    ("ties in rint", (0, 0, 0), (3, 0, 0), (0, 4, 0)),
    ("needle", (0, 0, 0), (CORNER, 1, 0), (CORNER, 0, 1)),
]


def test_hypotheses_on_recorded_triples(lib):
    H, m = len(TRIPLES), 1000
    pts = np.array([p for t in TRIPLES for p in t[1:]], np.int64)
    idx, got = lib_hypotheses(lib, 5, 0, H, m, pts)
    assert all(len(set(t)) == 3 for t in idx), "distinct indices: the planes depend on the points alone"
    for h, (what, *P) in enumerate(TRIPLES):
        want = R.hypothesis(idx[h], *P)
        assert got[h] == want, what
        if what in ("collinear", "repeated point"):
            assert want == (0, 0, 0, 0), what
        else:
            assert R.valid(want) and max(abs(v) for v in want[:3]) <= 65536 and abs(want[3]) < 1 << 42
    N = np.cross(np.array(TRIPLES[4][2], np.int64) - np.array(TRIPLES[4][1], np.int64),
                 np.array(TRIPLES[4][3], np.int64) - np.array(TRIPLES[4][1], np.int64))
    assert max(abs(int(v)) for v in N) > 1 << 47, "the cube's corners: components near 2^48 .. 2^52"
    assert got[0][:3] in ((0, 65536, 0), (0, -65536, 0)) and abs(got[0][3]) == 5 * 65536


def test_hypotheses_with_equal_indices(lib):
    # m = 2: every triple repeats an index, whatever the points
    pts = np.tile(np.array([(0, 0, 0), (9, 0, 0), (0, 0, 9)], np.int64), (64, 1))
    idx, got = lib_hypotheses(lib, 3, 0, 64, 2, pts)
    assert all(len(set(t)) < 3 for t in idx) and all(p == (0, 0, 0, 0) for p in got)
    # m = 4: some repeat, some do not; the planes follow the indices
    idx, got = lib_hypotheses(lib, 3, 0, 64, 4, pts)
    kinds = {len(set(t)) == 3 for t in idx}
    assert kinds == {True, False}
    for t, p in zip(idx, got):
        assert p == R.hypothesis(t, *pts[:3])
        assert R.valid(p) == (len(set(t)) == 3)


def test_hypotheses_axis_constraint_just_inside_and_outside(lib):
    # a plane tilted by atan(1/10) = 5.7106 degrees against +Y; b rounds to 65211 from 65210.76, and 0.01 degrees move
    # the limit 65536 cos(max_tilt) by 1.1, so the two tilts fall on either side of the rounded normal too
    P = [(0, 0, 0), (1000, 100, 0), (0, 0, 1000)]
    pts = np.array(P, np.int64)
    tilt = math.degrees(math.atan(0.1))
    for axis in ((0.0, 1.0, 0.0), (0.0, -3.0, 0.0)):
        for max_tilt, keep in ((tilt + 0.01, True), (tilt - 0.01, False), (90.0, True), (0.0, False)):
            idx, got = lib_hypotheses(lib, 0, 0, 1, 1000, pts, axis, max_tilt)
            want = R.hypothesis(idx[0], *P, axis=axis, max_tilt=max_tilt)
            assert got[0] == want
            assert R.valid(want) == keep, (axis, max_tilt)
    # max_tilt = 0 keeps only the axis itself
    flat = np.array([(0, 3, 0), (50, 3, 0), (0, 3, 50)], np.int64)
    _, got = lib_hypotheses(lib, 0, 0, 1, 1000, flat, (0.0, 1.0, 0.0), 0.0)
    assert got[0][:3] in ((0, 65536, 0), (0, -65536, 0))


def test_hypotheses_rejects_bad_arguments(lib):
    from spz_amd import abi
    idx = np.zeros(3, np.uint32)
    pts = np.zeros((3, 3), np.int32)
    plane = (abi.Plane * 1)()
    assert lib.spz_amd_plane_hypotheses(0, 0, 0, 10, None, None, 0.0, idx.ctypes.data, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_hypotheses(0, 0, 65537, 10, None, None, 0.0, None, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_hypotheses(0, 0, 1, 0, None, None, 0.0, idx.ctypes.data, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_hypotheses(0, 0, 1, 10, pts.ctypes.data, None, 0.0, None, None) == abi.ERR_INVALID_ARG
    zero = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.spz_amd_plane_hypotheses(0, 0, 1, 10, pts.ctypes.data, zero, 5.0, None, plane) == abi.ERR_INVALID_ARG
    up = (C.c_double * 3)(0.0, 1.0, 0.0)
    assert lib.spz_amd_plane_hypotheses(0, 0, 1, 10, pts.ctypes.data, up, 91.0, None, plane) == abi.ERR_INVALID_ARG


# ---- solve -----------------------------------------------------------------------------------------------------------
def moments_struct(mo):
    from spz_amd import abi
    s = abi.PlaneMoments()
    s.count, s.sum_abs, s.above, s.below, s.points = mo["count"], mo["sum_abs"], mo["above"], mo["below"], mo["points"]
    s.sum_p[:] = mo["sum_p"]
    for k, v in enumerate(mo["sum_pp"]):
        s.sum_pp_lo[k] = v & R.MASK64
        s.sum_pp_hi[k] = v >> 64
    return s


def lib_solve(lib, mo):
    from spz_amd import abi
    out = abi.Plane(9, 9, 9, 0, 9)
    n, lam = (C.c_double * 3)(), (C.c_double * 3)()
    deg = C.c_int(-1)
    assert lib.spz_amd_plane_solve(C.byref(moments_struct(mo)), C.byref(out), n, lam, C.byref(deg)) == abi.OK
    assert deg.value in (0, 1)
    if deg.value:
        assert (out.a, out.b, out.c, out.e) == (9, 9, 9, 9), "untouched when degenerate"
        return None
    return (out.a, out.b, out.c, out.e), list(n), list(lam)


def all_inliers(P):
    return R.moments(np.asarray(P, np.int64), (0, 65536, 0, 0), 1 << 62)


def planar_points(normal, e, n, seed, span=4000):
    """Integer points exactly on a X + b Y + c Z = e for a small integer normal with c = +-1."""
    a, b, c = normal
    assert abs(c) == 1
    rng = np.random.default_rng(seed)
    xy = rng.integers(-span, span, (n, 2))
    z = (e - a * xy[:, 0] - b * xy[:, 1]) * c
    return np.stack([xy[:, 0], xy[:, 1], z], axis=1).astype(np.int64)


@pytest.mark.parametrize("normal, e", [((0, 0, 1), 0), ((0, 0, 1), -77), ((3, 4, 1), 1000), ((-2, 7, -1), 12345),
                                       ((1, 1, 1), -5), ((100, -3, 1), 999)])
def test_solve_on_exactly_planar_points(lib, normal, e):
    P = planar_points(normal, e, 500, seed=abs(e) + 1)
    mo = all_inliers(P)
    got = lib_solve(lib, mo)
    want = R.solve(mo)
    assert got is not None and want is not None
    assert got[0] == want[0], "the integers of the restatement"
    # and the answer is the plane itself: the rounded unit normal, up to sign, and the offset it implies
    L = math.sqrt(sum(v * v for v in normal))
    unit = tuple(int(np.rint(65536.0 * v / L)) for v in normal)
    a, b, c, ee = got[0]
    assert (a, b, c) in (unit, tuple(-v for v in unit))
    d = R.distances(P, got[0])
    # d_i = delta . (P_i - mean) + the rounding of e, delta the rounding of the normal (at most 1/2 per component)
    assert np.abs(d).max() <= 0.5 * float((P.max(axis=0) - P.min(axis=0)).sum()) + 1.0
    assert got[2][2] <= 1e-12 * got[2][0], "no variance along the normal"


def test_solve_at_the_cube_corners_has_no_overflow(lib):
    # a plane through the far corners: sum P P^T near 2^57 per point, M near 2^70 for a handful of points
    c = (1 << 23) - 1
    P = np.array([(c, c, 100), (-c, c, 100), (c, -c, 100), (-c, -c, 100), (0, 0, 100), (c, 0, 100)], np.int64)
    mo = all_inliers(P)
    got, want = lib_solve(lib, mo), R.solve(mo)
    assert got[0] == want[0] and got[0][:3] in ((0, 0, 65536), (0, 0, -65536)) and abs(got[0][3]) == 100 * 65536


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_solve_on_noisy_points_residual(lib, seed):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    flat = np.stack([rng.uniform(-20000, 20000, 3000), rng.uniform(-20000, 20000, 3000), rng.normal(0, 3, 3000)], axis=1)
    P = np.rint(flat @ q.T + rng.uniform(-1000, 1000, 3)).astype(np.int64)
    mo = all_inliers(P)
    got, want = lib_solve(lib, mo), R.solve(mo)
    assert got[0] == want[0]
    assert got[1] == want[1] and got[2] == want[2], "the same Jacobi, operation for operation"
    M = np.array(R.moment_matrix(mo), np.float64)
    n, lam = np.array(got[1]), got[2]
    assert lam[0] >= lam[1] >= lam[2] >= 0
    assert abs(np.linalg.norm(n) - 1.0) <= 1e-14
    assert np.linalg.norm(M @ n - lam[2] * n) <= 1e-12 * np.linalg.norm(M), "|M n - lambda n| <= 1e-12 |M|"
    assert abs(abs(n @ q[:, 2]) - 1.0) < 1e-4, "the normal of the slab"
    w = np.linalg.eigvalsh(M)
    assert np.allclose(sorted(lam), w, rtol=1e-10, atol=1e-12 * w[-1])


def test_solve_degenerate_flags(lib):
    from spz_amd import abi
    line = np.array([(k, 2 * k, -3 * k) for k in range(-50, 50)], np.int64)
    assert lib_solve(lib, all_inliers(line)) is None and R.solve(all_inliers(line)) is None
    point = np.tile(np.array([(5, 6, 7)], np.int64), (10, 1))
    assert lib_solve(lib, all_inliers(point)) is None and R.solve(all_inliers(point)) is None
    two = np.array([(0, 0, 0), (1, 2, 3)], np.int64)
    assert lib_solve(lib, all_inliers(two)) is None and R.solve(all_inliers(two)) is None        # K < 3
    three = np.array([(0, 0, 0), (10, 0, 0), (0, 0, 10)], np.int64)
    assert lib_solve(lib, all_inliers(three))[0] == R.solve(all_inliers(three))[0]
    # nearly a line: the middle eigenvalue just above and just below 1e-12 of the largest
    for width, ok in ((10, True), (1, False), (0, False)):
        P = np.array([(k * 40000, (k % 2) * width, 0) for k in range(-100, 100)], np.int64)
        mo = all_inliers(P)
        assert (lib_solve(lib, mo) is not None) == ok == (R.solve(mo) is not None)
    deg = C.c_int(0)
    assert lib.spz_amd_plane_solve(None, C.byref(abi.Plane()), None, None, C.byref(deg)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_solve(C.byref(abi.PlaneMoments()), None, None, None, C.byref(deg)) == abi.ERR_INVALID_ARG


def test_div_round_ties_to_even():
    assert [R.div_round(n, 4) for n in (-6, -5, -2, 2, 5, 6, 10, 14)] == [-2, -1, 0, 0, 1, 2, 2, 4]


# ---- the placement ---------------------------------------------------------------------------------------------------
def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


PLANES = [(0, 65536, 0, 65536 * 4096), (0, -65536, 0, 12345678), (46341, 46341, 0, -999), (12345, -23456, 59952, 4000000),
          (-65536, 0, 0, 77), (1, -65536, 2, 0), (0, 0, -65536, -(1 << 40)), (37837, 37837, 37837, 1 << 41)]


@pytest.mark.parametrize("coord", range(0, 9))
@pytest.mark.parametrize("plane", PLANES)
def test_placement_levels_the_plane_in_every_coord(lib, coord, plane):
    from spz_amd import abi
    f = 12
    res = abi.PlaneResult()
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(plane[0], plane[1], plane[2], 0, plane[3])), f, coord, 0,
                                       C.byref(res)) == abi.OK
    normal, offset, rot, tr = R.placement(plane, f, coord)
    assert list(res.normal) == normal and res.offset == offset and list(res.rotation) == rot
    assert list(res.translation) == tr and res.scale == 1.0
    fl = np.array(R.flips(coord))
    up = np.array([0.0, fl[1], 0.0])             # +-Y by the U / D letter
    n, q, t = np.array(res.normal), np.array(res.rotation), np.array(res.translation)
    assert abs(np.linalg.norm(n) - 1.0) <= 4e-16 and abs(np.linalg.norm(q) - 1.0) <= 4e-16 and q[3] >= 0.0
    # the placed plane: n' = R n, offset' = offset + n' . t
    n2 = quat_matrix(q) @ n
    assert np.abs(n2 - up).max() <= 4e-15, "normal = up"
    assert abs(res.offset + n2 @ t) <= 4e-15 * max(1.0, abs(res.offset)), "offset 0"
    # ... and through spz_amd_transform_params, in the stored frame, where up is +Y whatever coord is (f32 block)
    xf = abi.Transform()
    assert lib.spz_amd_transform_params(res.rotation, res.translation, 1.0, coord, C.byref(xf)) == abi.OK
    M = np.array(list(xf.m), np.float64).reshape(3, 3)
    n_rub = np.array(plane[:3], np.float64) / math.sqrt(sum(float(v) ** 2 for v in plane[:3]))
    assert np.abs(M @ n_rub - np.array([0.0, 1.0, 0.0])).max() <= 3e-7
    assert np.allclose(list(xf.t), [0.0, -res.offset, 0.0], rtol=1e-7, atol=0.0)
    # without the translation
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(plane[0], plane[1], plane[2], 0, plane[3])), f, coord, 1,
                                       C.byref(res)) == abi.OK
    assert list(res.translation) == [0.0, 0.0, 0.0] and list(res.rotation) == rot


def test_placement_of_the_opposite_normal_is_a_half_turn_about_stored_x(lib):
    from spz_amd import abi
    for coord in range(9):
        res = abi.PlaneResult()
        assert lib.spz_amd_plane_placement(C.byref(abi.Plane(0, -65536, 0, 0, 65536 * 2048)), 11, coord, 0,
                                           C.byref(res)) == abi.OK
        assert [abs(v) for v in res.rotation] == [1.0, 0.0, 0.0, 0.0]
        assert res.offset == 1.0
        fl = R.flips(coord)
        n2 = quat_matrix(res.rotation) @ np.array(res.normal)
        assert list(n2) == [0.0, fl[1], 0.0]
        assert res.offset + n2 @ np.array(res.translation) == 0.0
    bad = abi.PlaneResult()
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(0, 0, 0, 0, 5)), 12, 0, 0, C.byref(bad)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(0, 65537, 0, 0, 5)), 12, 0, 0, C.byref(bad)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(0, 1, 0, 0, 5)), 12, 9, 0, C.byref(bad)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_placement(C.byref(abi.Plane(0, 1, 0, 0, 5)), 25, 0, 0, C.byref(bad)) == abi.ERR_INVALID_ARG


def test_device_forms_check_their_arguments_before_the_device(lib):
    from spz_amd import abi
    hdr = abi.Header(3, 8, 0, 12, 0, 0)
    m = C.c_uint64(5)
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    prepare = lambda h, stride=1, ws=p, size=buf.size: lib.spz_amd_plane_prepare_device(
        p, size, C.byref(h), stride, None, ws, C.byref(m), None)
    assert prepare(abi.Header(1, 8, 0, 12, 0, 0)) == abi.ERR_UNSUPPORTED and m.value == 0
    assert prepare(abi.Header(3, 10_000_001, 0, 12, 0, 0), size=1 << 40) == abi.ERR_TOO_MANY_POINTS
    assert prepare(hdr, size=100) == abi.ERR_SHORT_STREAM
    assert prepare(hdr, stride=0) == abi.ERR_INVALID_ARG
    assert prepare(hdr, ws=None) == abi.ERR_INVALID_ARG
    assert prepare(abi.Header(3, 8, 0, 25, 0, 0)) == abi.ERR_INVALID_ARG
    plane, zero = abi.Plane(0, 65536, 0, 0, 0), abi.Plane(0, 0, 0, 0, 7)
    assert lib.spz_amd_plane_score_device(p, 8, 8, p, 0, 5, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_score_device(p, 8, 9, p, 1, 5, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_score_device(p, 8, 8, p, 1, (1 << 36) + 1, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_score_device(None, 8, 8, p, 1, 5, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_moments_device(p, 8, 8, C.byref(zero), 5, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_moments_device(p, 8, 8, C.byref(plane), 5, None, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_mark_device(p, 8, 8, C.byref(zero), 5, 1, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_mark_device(p, 8, 8, C.byref(plane), 5, 1, None, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_gather_device(p, 8, 0, p, 3, p, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_plane_gather_device(p, 8, 8, p, 0, p, None) == abi.OK                     # nothing to do
    found = C.c_uint32(9)
    res = (abi.PlaneResult * 2)()
    o = options(lib, max_planes=2)
    host = lambda h, opt=o, cap=2: lib.spz_amd_plane_host(p, buf.size, C.byref(h), C.byref(opt), 0, res, cap,
                                                          C.byref(found), None, None)
    assert host(abi.Header(1, 8, 0, 12, 0, 0)) == abi.ERR_UNSUPPORTED and found.value == 0
    assert host(hdr, cap=1) == abi.ERR_INVALID_ARG
    assert host(hdr, opt=options(lib, threshold=math.nan)) == abi.ERR_INVALID_ARG
    assert host(hdr, opt=options(lib, threshold=257.0)) == abi.ERR_INVALID_ARG                   # T > 2^36 at f = 12
    assert lib.spz_amd_plane_workspace_bytes(0) > 0
    assert lib.spz_amd_plane_workspace_bytes(10_000_000) < 1 << 30


# ---- spz_level's arguments -------------------------------------------------------------------------------------------
USAGE = ("Usage: spz_level <in.spz> [out.spz] --threshold TAU [--hypotheses H] [--seed S] [--stride K] [--refine R] "
         "[--planes K] [--min-inliers N|FRACTION] [--axis X Y Z --max-tilt DEG] [--up-hint X Y Z] "
         "[--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED] [--no-translate] "
         "[--select plane|off-plane|above|below] [--fractional-bits n]")


@pytest.mark.parametrize("argv", [
    ["spz_level"], ["spz_level", "--threshold", "0.1"], ["spz_tool", "spz_level"], ["spz_level", "a.spz"],
    ["spz_level", "a.spz", "b.spz"], ["spz_level", "a.spz", "--threshold"], ["spz_level", "a.spz", "--threshold", "x"],
    ["spz_level", "a.spz", "--threshold", "nan"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--hypotheses", "0"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--hypotheses", "65537"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--refine", "17"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--planes", "0"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--planes", "256"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--stride", "0"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--seed", "-1"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--min-inliers", "1.5"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--min-inliers", "-3"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--min-inliers", "half"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--axis", "0", "1"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--axis", "0", "1", "0"],            # no --max-tilt
    ["spz_level", "a.spz", "--threshold", "0.1", "--max-tilt", "5"],                   # no --axis
    ["spz_level", "a.spz", "--threshold", "0.1", "--up-hint", "0", "1", "z"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--coord", "XYZ"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--select", "plane"],                 # no output file
    ["spz_level", "a.spz", "b.spz", "--threshold", "0.1", "--select", "floor"],
    ["spz_level", "a.spz", "b.spz", "--threshold", "0.1", "--fractional-bits", "25"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--threshold", "0.2"],
    ["spz_level", "a.spz", "--threshold", "0.1", "--bogus"],
])
def test_cli_usage(argv, tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith(USAGE)
    assert r.stdout == ""


@pytest.mark.parametrize("extra", [["--threshold", "-1"], ["--threshold", "inf"],
                                   ["--threshold", "0.1", "--axis", "0", "0", "0", "--max-tilt", "5"],
                                   ["--threshold", "0.1", "--axis", "0", "1", "0", "--max-tilt", "95"],
                                   ["--threshold", "0.1", "--up-hint", "0", "0", "0"]])
def test_cli_bad_values_exit_1_with_one_error_line(tmp_path, extra):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_level")
    r = subprocess.run([exe, "a.spz", "c.spz"] + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert (r.stdout + r.stderr).count("[SPZ ERROR] levelSpz:") == 1
    assert not (tmp_path / "c.spz").exists()


def test_cli_unreadable_input_exits_1_without_output(tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_level")
    for args in (["missing.spz", "--threshold", "0.1"], ["missing.spz", "c.spz", "--threshold", "0.1"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
        assert r.returncode == 1 and "--rotate" not in r.stdout
        assert not (tmp_path / "c.spz").exists()


def test_python_level_spz_refuses_bad_arguments(tmp_path):
    import spz_amd.spz as spz
    f = str(tmp_path / "a.spz")
    with pytest.raises(TypeError):
        spz.level_spz(f)                                          # threshold has no default
    for kw in ({"threshold": -1.0}, {"threshold": math.nan}, {"threshold": "x"}, {"threshold": 0.1, "hypotheses": 0},
               {"threshold": 0.1, "hypotheses": 65537}, {"threshold": 0.1, "refine": 17}, {"threshold": 0.1, "planes": 0},
               {"threshold": 0.1, "stride": 0}, {"threshold": 0.1, "seed": -1}, {"threshold": 0.1, "min_inliers": 1.5},
               {"threshold": 0.1, "min_inliers": -1}, {"threshold": 0.1, "axis": (0, 1, 0)},
               {"threshold": 0.1, "max_tilt": 5.0}, {"threshold": 0.1, "axis": (0, 1), "max_tilt": 5.0},
               {"threshold": 0.1, "axis": (0, 1, 0), "max_tilt": 91.0}, {"threshold": 0.1, "select": "plane"},
               {"threshold": 0.1, "up_hint": (1, 2)}, {"threshold": 0.1, "fractional_bits": 25}):
        with pytest.raises(ValueError):
            spz.level_spz(f, **kw)
    with pytest.raises(ValueError):
        spz.level_spz(f, str(tmp_path / "b.spz"), threshold=0.1, select="floor")
    with pytest.raises(ValueError):
        spz.level_spz(b"1234", str(tmp_path / "b.spz"), threshold=0.1)
    with pytest.raises(ValueError, match="refused"):
        spz.level_spz(f, threshold=0.1, up_hint=(0.0, 0.0, 0.0))   # the library's own check
    assert not (tmp_path / "b.spz").exists()
