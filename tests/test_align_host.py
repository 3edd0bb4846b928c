"""The host side of the alignment (DESIGN §8 "Align"; include/spz_amd.h "align"), no GPU: tests/align_ref.py's nearest
neighbour against an independent O(n^2) loop, the library's argument checks and workspace size, spz_amd_align_solve
against the numpy SVD solution, the entry points without a device, and the CLI's argument handling."""
import ctypes as C
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import align_ref as R
from conftest import ROOT
from test_filter_host import MAGIC


@pytest.fixture(scope="module")
def lib():
    from spz_amd import abi
    return abi.load_library()


# ---- the restatement's nearest neighbour ---------------------------------------------------------------------------
def loop_nearest(Q, T):
    idx, d2 = [], []
    for q in Q.tolist():
        best, at = None, -1
        for j, t in enumerate(T.tolist()):
            d = sum((a - b) ** 2 for a, b in zip(q, t))
            if best is None or d < best:
                best, at = d, j
        idx.append(at)
        d2.append(best)
    return np.array(idx, np.int64), np.array(d2, np.int64)


@pytest.mark.parametrize("method", ["brute", "tree"])
def test_reference_nearest_matches_a_plain_loop(method):
    if method == "tree":
        pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(3)
    T = rng.integers(-40, 40, (300, 3))
    T[50:60] = T[7]                                    # duplicates: the smallest index wins
    T = np.concatenate([T, [[100, 0, 0], [102, 0, 0], [101, 1, 0], [101, -1, 0], [101, 0, 1], [101, 0, -1]]])
    Q = np.concatenate([rng.integers(-60, 60, (200, 3)), T[7:8], [[101, 0, 0]],   # six targets at distance 1
                        [[1 << 26, -(1 << 26), 1 << 26]]]).astype(np.int64)
    T = T.astype(np.int64)
    want_i, want_d = loop_nearest(Q, T)
    got_i, got_d = R.nearest(Q, T, method=method)
    assert np.array_equal(got_d, want_d)
    assert np.array_equal(got_i, want_i)
    assert got_i[200] == 7 and got_d[200] == 0
    assert got_i[201] == 300 and got_d[201] == 1
    lim_i, lim_d = R.nearest(Q, T, limit=4, method=method)
    far = want_d > 4
    assert np.all(lim_i[far] == R.NONE) and np.all(lim_d[far] == R.NONE)
    assert np.array_equal(lim_i[~far], want_i[~far])


def test_reference_queries_round_to_even_and_saturate():
    P = np.array([[1, 0, 0], [3, 0, 0], [5, 0, 0], [1 << 22, 0, 0]], np.int64)
    m = list(R.IDENTITY)
    Q, valid = R.queries(P, 1, 0, m)                  # x = P / 2: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert Q[:3, 0].tolist() == [0, 2, 2] and valid.all()
    m[0] = 1e6
    Q, valid = R.queries(P, 0, 12, m)
    assert Q[3, 0] == 1 << 26 and valid.all()
    m[9] = math.inf
    Q, valid = R.queries(P, 0, 12, m)
    assert not valid.any()
    Q, valid = R.queries(P, 0, 0, R.IDENTITY, stride=3)
    assert valid.tolist() == [True, False, False, True]


# ---- argument checks and sizes -------------------------------------------------------------------------------------
def defaults(lib):
    from spz_amd import abi
    o = abi.AlignOptions()
    assert lib.spz_amd_align_default_options(C.byref(o)) == abi.OK
    return o


def test_align_check_accepts_the_defaults_and_refuses_each_bad_argument(lib):
    from spz_amd import abi
    o = defaults(lib)
    assert lib.spz_amd_align_check(C.byref(o)) == abi.OK
    assert (o.stride, o.max_iterations, o.overlap, o.has_max_distance) == (1, 30, 1.0, 0)
    assert (o.relative_fitness, o.relative_rmse, o.scale, tuple(o.rotation)) == (1e-6, 1e-6, 1.0, (0.0, 0.0, 0.0, 1.0))
    assert lib.spz_amd_align_check(None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_align_default_options(None) == abi.ERR_INVALID_ARG

    def bad(**kw):
        o = defaults(lib)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[:] = v
            else:
                setattr(o, k, v)
        return lib.spz_amd_align_check(C.byref(o))

    good = [dict(overlap=0.5), dict(has_max_distance=1, max_distance=0.25), dict(max_iterations=1000), dict(stride=7),
            dict(relative_fitness=0.0, relative_rmse=0.0), dict(rotation=(0.0, 3.0, 0.0, 0.0)), dict(coord=8),
            dict(max_distance=-1.0)]                   # not read without has_max_distance
    for kw in good:
        assert bad(**kw) == abi.OK, kw
    refused = [dict(stride=0), dict(overlap=0.0), dict(overlap=-0.1), dict(overlap=1.0000001), dict(overlap=math.nan),
               dict(has_max_distance=1, max_distance=0.0), dict(has_max_distance=1, max_distance=-1.0),
               dict(has_max_distance=1, max_distance=math.inf), dict(has_max_distance=1, max_distance=math.nan),
               dict(max_iterations=0), dict(max_iterations=1001), dict(relative_fitness=-1e-9),
               dict(relative_fitness=math.nan), dict(relative_rmse=math.inf), dict(relative_rmse=-1.0),
               dict(rotation=(0.0, 0.0, 0.0, 0.0)), dict(rotation=(math.nan, 0.0, 0.0, 1.0)),
               dict(rotation=(math.inf, 0.0, 0.0, 1.0)), dict(translation=(0.0, math.inf, 0.0)),
               dict(translation=(math.nan, 0.0, 0.0)), dict(scale=0.0), dict(scale=-2.0), dict(scale=math.inf),
               dict(scale=math.nan), dict(coord=9), dict(coord=-1)]
    for kw in refused:
        assert bad(**kw) == abi.ERR_INVALID_ARG, kw


def test_align_workspace_bytes_is_monotone(lib):
    f = lib.spz_amd_align_workspace_bytes
    sizes = [0, 1, 2048, 2049, 100_000, 1_000_000, 10_000_000]
    for a, b in zip(sizes, sizes[1:]):
        for other in (1, 5000, 10_000_000):
            assert f(a, other) <= f(b, other)
            assert f(other, a) <= f(other, b)
    assert f(0, 1) > 0
    # the sorted positions (16 B), index, d2 and inlier byte per source point at least
    assert f(1_000_000, 1) - f(0, 1) >= 1_000_000 * (16 + 4 + 8 + 1)


def stream(n, version=3, fb=12):
    return struct.pack("<IIIBBBB", MAGIC, version, n, 0, fb, 0, 0) + bytes(n * (9 + 1 + 3 + 3 + (3 if version == 2 else 4)))


def test_device_entry_points_check_before_they_launch_and_fail_loudly_without_a_gpu(lib):
    import torch
    from spz_amd import abi
    raw = np.frombuffer(stream(8), np.uint8)
    cloud = lambda n=8, version=3, size=None: abi.AlignCloud(raw.ctypes.data, raw.size if size is None else size,
                                                              abi.Header(version, n, 0, 12, 0, 0))
    ok, v1, empty, short = cloud(), cloud(version=1), cloud(n=0), cloud(size=raw.size - 1)
    big = abi.AlignCloud(raw.ctypes.data, 1 << 40, abi.Header(3, 10_000_001, 0, 12, 0, 0))
    m = (C.c_double * 12)(*R.IDENTITY)
    nan_map = (C.c_double * 12)(*([math.nan] * 12))
    d = raw.ctypes.data                                # never dereferenced: every call below returns before a launch
    prep, near, step = lib.spz_amd_align_prepare_device, lib.spz_amd_nearest_device, lib.spz_amd_align_step_device
    for s, t, want in ((v1, ok, abi.ERR_UNSUPPORTED), (ok, v1, abi.ERR_UNSUPPORTED), (ok, empty, abi.ERR_INVALID_ARG),
                       (short, ok, abi.ERR_SHORT_STREAM), (big, ok, abi.ERR_TOO_MANY_POINTS),
                       (ok, big, abi.ERR_TOO_MANY_POINTS)):
        assert prep(C.byref(s), C.byref(t), d, None) == want
        assert near(C.byref(s), C.byref(t), 1, m, abi.NO_LIMIT_R2, d, d, d, None) == want
        assert step(C.byref(s), C.byref(t), 1, m, abi.NO_LIMIT_R2, 1.0, d, d, d, d, d, None) == want
    assert prep(None, C.byref(ok), d, None) == abi.ERR_INVALID_ARG
    assert prep(C.byref(ok), C.byref(ok), None, None) == abi.ERR_INVALID_ARG
    assert near(C.byref(ok), C.byref(ok), 0, m, abi.NO_LIMIT_R2, d, d, d, None) == abi.ERR_INVALID_ARG
    assert near(C.byref(ok), C.byref(ok), 1, nan_map, abi.NO_LIMIT_R2, d, d, d, None) == abi.ERR_INVALID_ARG
    assert near(C.byref(ok), C.byref(ok), 1, m, abi.NO_LIMIT_R2, None, d, d, None) == abi.ERR_INVALID_ARG
    for overlap in (0.0, 1.5, math.nan):
        assert step(C.byref(ok), C.byref(ok), 1, m, abi.NO_LIMIT_R2, overlap, d, d, d, d, d, None) == abi.ERR_INVALID_ARG
    assert step(C.byref(ok), C.byref(ok), 1, m, abi.NO_LIMIT_R2, 1.0, d, d, d, None, d, None) == abi.ERR_INVALID_ARG
    res, o = abi.AlignResult(), defaults(lib)
    host = lib.spz_amd_align_host
    assert host(C.byref(ok), C.byref(ok), C.byref(o), 0, None, None, 0, None) == abi.ERR_INVALID_ARG
    assert host(C.byref(v1), C.byref(ok), C.byref(o), 0, C.byref(res), None, 0, None) == abi.ERR_UNSUPPORTED
    assert host(C.byref(ok), C.byref(empty), C.byref(o), 0, C.byref(res), None, 0, None) == abi.ERR_INVALID_ARG
    o.stride = 0
    assert host(C.byref(ok), C.byref(ok), C.byref(o), 0, C.byref(res), None, 0, None) == abi.ERR_INVALID_ARG
    if torch.cuda.is_available():
        return
    o = defaults(lib)
    assert prep(C.byref(ok), C.byref(ok), d, None) == abi.ERR_NO_DEVICE
    assert near(C.byref(ok), C.byref(ok), 1, m, abi.NO_LIMIT_R2, d, d, d, None) == abi.ERR_NO_DEVICE
    assert step(C.byref(ok), C.byref(ok), 1, m, abi.NO_LIMIT_R2, 1.0, d, d, d, d, d, None) == abi.ERR_NO_DEVICE
    assert host(C.byref(ok), C.byref(ok), C.byref(o), 0, C.byref(res), None, 0, None) == abi.ERR_NO_DEVICE
    assert res.iterations == 0


# ---- the solve -------------------------------------------------------------------------------------------------------
def moments_of(a, b):
    from spz_amd import abi
    t = np.empty((a.shape[0], 9))
    for r in range(3):
        for c in range(3):
            t[:, 3 * r + c] = a[:, r] * b[:, c]
    mom = dict(count=a.shape[0], taking_part=a.shape[0], sum_a=a.sum(0), sum_b=b.sum(0), sum_ab=t.sum(0),
               sum_aa=float((a * a).sum()), sum_bb=float((b * b).sum()), sum_d2=0)
    m = abi.AlignMoments()
    m.count = m.taking_part = m.candidates = a.shape[0]
    m.sum_a[:] = mom["sum_a"]
    m.sum_b[:] = mom["sum_b"]
    m.sum_ab[:] = mom["sum_ab"]
    m.sum_aa, m.sum_bb = mom["sum_aa"], mom["sum_bb"]
    return mom, m


def lib_solve(lib, m, estimate_scale, scale_in=1.0):
    from spz_amd import abi
    out, s, deg = (C.c_double * 12)(*([7.0] * 12)), C.c_double(-1.0), C.c_int(-1)
    assert lib.spz_amd_align_solve(C.byref(m), int(estimate_scale), scale_in, out, C.byref(s), C.byref(deg)) == abi.OK
    return np.array(out[:]), s.value, deg.value


def residual(mp, a, b):
    y = a @ mp[:9].reshape(3, 3).T + mp[9:]
    return float(((y - b) ** 2).sum())


def random_rotation(rng):
    q = rng.normal(size=4)
    return R.quat_to_matrix(q)


@pytest.mark.parametrize("estimate_scale", [False, True])
@pytest.mark.parametrize("case", ["rigid", "scaled", "reflection", "planar", "offset"])
def test_solve_matches_the_numpy_svd_solution(lib, case, estimate_scale):
    rng = np.random.default_rng(2 * ["rigid", "scaled", "reflection", "planar", "offset"].index(case) + int(estimate_scale))
    n = 500
    a = rng.normal(size=(n, 3)) * np.array([3.0, 1.0, 0.5])
    if case == "planar":
        a[:, 2] = 0.0
    if case == "offset":
        a += np.array([40.0, -25.0, 10.0])
    Rt, t, s = random_rotation(rng), rng.normal(size=3) * 2, (1.3 if case == "scaled" else 1.0)
    b = s * a @ Rt.T + t + rng.normal(size=(n, 3)) * 0.05
    if case == "reflection":                           # the best orthogonal fit is a reflection: det U det V < 0
        b = a * np.array([1.0, 1.0, -1.0]) @ Rt.T + t + rng.normal(size=(n, 3)) * 0.01
    mom, m = moments_of(a, b)
    got, gs, deg = lib_solve(lib, m, estimate_scale, 1.0)
    want = R.solve(mom, estimate_scale, 1.0)
    assert deg == 0 and want is not None
    if case == "reflection":
        H = np.asarray(mom["sum_ab"]).reshape(3, 3).T / n - np.outer(mom["sum_b"] / n, mom["sum_a"] / n)
        U, _, Vt = np.linalg.svd(H)
        assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    Rg = got[:9].reshape(3, 3) / gs
    assert np.abs(Rg.T @ Rg - np.eye(3)).max() <= 1e-14
    assert abs(np.linalg.det(Rg) - 1.0) <= 1e-14
    if not estimate_scale:
        assert gs == 1.0
    rg, rw = residual(got, a, b), residual(want[0], a, b)
    assert abs(rg - rw) <= 1e-12 * rw, (rg, rw)
    assert abs(gs - want[1]) <= 1e-12 * want[1]


def test_solve_reports_the_degenerate_cases(lib):
    from spz_amd import abi
    rng = np.random.default_rng(5)
    b = rng.normal(size=(50, 3))
    line = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5]) + 3.0
    point = np.tile([[1.0, 2.0, 3.0]], (50, 1))
    for a, bb in ((b[:2], b[:2]), (point, b), (line, b), (b, point), (line, line)):
        mom, m = moments_of(a, bb)
        got, gs, deg = lib_solve(lib, m, True)
        assert deg == 1 and np.all(got == 7.0) and gs == -1.0, "a degenerate solve leaves its outputs alone"
        assert R.solve(mom, True, 1.0) is None
    mom, m = moments_of(b, b)
    assert lib_solve(lib, m, True)[2] == 0
    out, deg = (C.c_double * 12)(), C.c_int()
    assert lib.spz_amd_align_solve(None, 0, 1.0, out, None, C.byref(deg)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_align_solve(C.byref(m), 0, 0.0, out, None, C.byref(deg)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_align_solve(C.byref(m), 0, 1.0, out, None, None) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_align_solve(C.byref(m), 0, 1.0, out, None, C.byref(deg)) == abi.OK and deg.value == 0


# ---- the Python layers -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


@pytest.mark.parametrize("kw", [
    dict(stride=0), dict(stride=2.0), dict(stride=True), dict(overlap=0.0), dict(overlap=1.5), dict(overlap=math.nan),
    dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=math.inf), dict(max_iterations=0),
    dict(max_iterations=1001), dict(relative_fitness=-1.0), dict(relative_rmse=math.nan),
    dict(rotation=(0, 0, 0, 0)), dict(rotation=(0, 0, 1)), dict(translation=(0, math.inf, 0)), dict(translation=(1, 2)),
    dict(scale=0.0), dict(scale=math.nan),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()))
def test_align_spz_refuses_bad_arguments_before_device_work(spz, tmp_path, kw):
    p = tmp_path / "in.spz"
    p.write_bytes(b"not read: the arguments are checked first")
    with pytest.raises(ValueError):
        spz.align_spz(str(p), str(p), **kw)
    with pytest.raises(ValueError):
        spz.align_spz(str(p), b"bytes and a path")


def test_align_spz_fails_loudly_without_a_gpu(spz, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = tmp_path / "in.spz"
    p.write_bytes(gz(stream(8)))
    with pytest.raises(RuntimeError):
        spz.align_spz(str(p), str(p))
    with pytest.raises(RuntimeError):
        spz.align_spz(p.read_bytes(), p.read_bytes())


def test_device_align_functions_check_their_arguments():
    torch = pytest.importorskip("torch")
    from spz_amd import abi, device as D
    hdr = D.make_header(10, 0)
    st = torch.zeros(16, dtype=torch.uint8)
    for f in (D.nearest_packed, D.align_step_packed, D.align_packed):
        with pytest.raises(ValueError):
            f(st, hdr, st, hdr)                                # not CUDA tensors
    # the helpers behind them, which need no tensor
    assert list(D._align_map(None)) == list(R.IDENTITY)
    for bad in ([1.0] * 11, [math.nan] + [0.0] * 11, [math.inf] * 12):
        with pytest.raises(ValueError):
            D._align_map(bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            D._align_stride(bad)
    assert D._align_stride(3) == 3
    assert D._align_r2(None, 12) == abi.NO_LIMIT_R2
    assert D._align_r2(0.05, 12) == R.radius_r2(0.05, 12)
    for bad in (0.0, -1.0, math.nan, math.inf, True, "1"):
        with pytest.raises(ValueError):
            D._align_r2(bad, 12)


# ---- the CLI -----------------------------------------------------------------------------------------------------
USAGE = ("Usage: spz_align <source.spz> <target.spz> [--output aligned.spz] [--scale] [--overlap F] [--max-distance D] "
         "[--stride K] [--iterations N] [--init-centroids] [--rotate x y z w] [--translate x y z] [--init-scale S] "
         "[--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED] [--fractional-bits n]")


@pytest.mark.parametrize("argv", [
    ["spz_align"], ["spz_align", "a.spz"], ["spz_tool", "spz_align", "a.spz"], ["spz_align", "--scale", "a.spz", "b.spz"],
    ["spz_align", "a.spz", "b.spz", "--overlap"], ["spz_align", "a.spz", "b.spz", "--overlap", "x"],
    ["spz_align", "a.spz", "b.spz", "--stride", "0"], ["spz_align", "a.spz", "b.spz", "--stride", "2.5"],
    ["spz_align", "a.spz", "b.spz", "--iterations", "0"], ["spz_align", "a.spz", "b.spz", "--iterations", "1001"],
    ["spz_align", "a.spz", "b.spz", "--rotate", "0", "0", "1"], ["spz_align", "a.spz", "b.spz", "--translate", "1", "2"],
    ["spz_align", "a.spz", "b.spz", "--coord", "XYZ"], ["spz_align", "a.spz", "b.spz", "--fractional-bits", "25"],
    ["spz_align", "a.spz", "b.spz", "--scale", "--scale"], ["spz_align", "a.spz", "b.spz", "--bogus"],
    ["spz_align", "a.spz", "b.spz", "--output"], ["spz_align", "a.spz", "b.spz", "--max-distance", "1e"],
])
def test_cli_usage(argv, tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith(USAGE)
    assert r.stdout == ""


@pytest.mark.parametrize("extra", [["--overlap", "0"], ["--overlap", "1.5"], ["--max-distance", "-1"],
                                   ["--init-scale", "0"], ["--rotate", "0", "0", "0", "0"]])
def test_cli_bad_values_exit_1_with_one_error_line(tmp_path, extra):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_align")
    r = subprocess.run([exe, "a.spz", "b.spz", "--output", "c.spz"] + extra, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert (r.stdout + r.stderr).count("[SPZ ERROR] alignSpz:") == 1
    assert not (tmp_path / "c.spz").exists()


def test_cli_unreadable_input_exits_1_without_output(tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_align")
    r = subprocess.run([exe, "missing.spz", "b.spz", "--output", "c.spz"], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1 and "--rotate" not in r.stdout
    assert not (tmp_path / "c.spz").exists()
