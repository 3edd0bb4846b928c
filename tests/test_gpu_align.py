"""spz.align_spz / spz_align / spz_amd_align_host / spz_amd.device.nearest_packed + align_step_packed + align_packed
(DESIGN §8 "Align") on the GPU, against the numpy restatement of tests/align_ref.py: the nearest neighbour index for
index and d2 for d2, the inlier set exactly, the moments within the bound of their summation tree, runs that recover a
known placement, and two runs equal bit for bit."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

import align_ref as R
from clean_ref import stored_positions
from conftest import ROOT
from test_gpu_clean import clustered_scene, gz, on_device, stream_of

pytestmark = pytest.mark.gpu

BIAS = 1 << 23


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


@pytest.fixture(scope="module")
def D(cuda):
    from spz_amd import device
    return device


def fields_of(P):
    """The stored 24-bit fields (two's complement) of signed integer positions."""
    return np.asarray(P, np.int64) & 0xFFFFFF


def u_stream(u, **kw):
    """A stream from biased coordinates u = P + 2^23 in [0, 2^24): the cube as the Morton key sees it."""
    return stream_of(np.asarray(u, np.int64) ^ BIAS, **kw)


def check_nearest(D, src_raw, tgt_raw, m=None, stride=1, max_distance=None, method=None):
    """nearest_packed against the restatement, exactly; returns the reference's (index, d2)."""
    (st, sh), (tt, th) = on_device(src_raw), on_device(tgt_raw)
    idx, d2 = D.nearest_packed(st, sh, tt, th, map=m, stride=stride, max_distance=max_distance)
    Ps, fs = R.positions_of(src_raw)
    Pt, ft = R.positions_of(tgt_raw)
    Q, valid = R.queries(Ps, fs, ft, R.IDENTITY if m is None else m, stride)
    limit = None if max_distance is None else R.radius_r2(max_distance, ft)
    want_i, want_d = R.nearest(Q, Pt, valid, limit, method)
    got_i, got_d = idx.cpu().numpy(), d2.cpu().numpy()
    assert got_i.shape == (Ps.shape[0],) and got_d.shape == (Ps.shape[0],)
    assert np.array_equal(got_d, want_d), "d2 for d2"
    assert np.array_equal(got_i, want_i), "index for index"
    return want_i, want_d


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097])
def test_nearest_random_pairs(D, n):
    rng = np.random.default_rng(n)
    src = u_stream(rng.integers(0x7e0000, 0x820000, (n + 3, 3)), seed=1)
    tgt = u_stream(rng.integers(0x7e0000, 0x820000, (n, 3)), seed=2)
    check_nearest(D, src, tgt)
    check_nearest(D, tgt, src, m=(0.9, 0.1, 0.0, -0.1, 0.9, 0.0, 0.0, 0.0, 1.1, 0.5, -0.25, 3.0))
    check_nearest(D, src, u_stream(rng.integers(0, 1 << 24, (n, 3)), seed=3))      # all of the cube


def test_nearest_different_fractional_bits(D):
    rng = np.random.default_rng(8)
    src = u_stream(rng.integers(BIAS - 2000, BIAS + 2000, (3000, 3)), fb=8, seed=1)     # +-7.8 units
    tgt = u_stream(rng.integers(BIAS - 120_000, BIAS + 120_000, (5000, 3)), fb=14, seed=2)  # +-7.3 units
    check_nearest(D, src, tgt)
    check_nearest(D, tgt, src)          # 14 -> 8: many queries round to one place, and ties to even


def test_nearest_target_of_many_duplicates(D):
    rng = np.random.default_rng(9)
    places = rng.integers(BIAS - 500, BIAS + 500, (40, 3))
    tgt = u_stream(places[rng.integers(0, 40, 6000)], seed=1)         # 150 copies of each place, shuffled
    src = u_stream(np.concatenate([places, rng.integers(BIAS - 600, BIAS + 600, (2000, 3))]), seed=2)
    want_i, want_d = check_nearest(D, src, tgt)
    assert np.all(want_d[:40] == 0)


def test_nearest_source_outside_the_targets_cube(D):
    rng = np.random.default_rng(10)
    src = u_stream(rng.integers(BIAS - 4000, BIAS + 4000, (1500, 3)), seed=1)
    tgt = u_stream(rng.integers(0, 1 << 24, (3000, 3)), seed=2)
    far = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 30000.0, -30000.0, 2100.0)   # beyond +-2^26 quanta: saturates
    want_i, want_d = check_nearest(D, src, tgt, m=far)
    assert want_d.min() > (1 << 50)
    check_nearest(D, src, tgt, m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 2047.0, 0.0, -2049.0))   # the faces
    nowhere = list(far)
    nowhere[9] = 1e308
    nowhere[0] = 1e308
    idx, d2 = D.nearest_packed(*on_device(src), *on_device(tgt), map=nowhere)
    Q, valid = R.queries(R.positions_of(src)[0], 12, 12, nowhere)
    assert np.array_equal(idx.cpu().numpy() == R.NONE, ~valid) and not valid.all()


def test_nearest_stride_and_max_distance(D):
    rng = np.random.default_rng(11)
    src = u_stream(rng.integers(BIAS - 30_000, BIAS + 30_000, (5000, 3)), seed=1)
    tgt = u_stream(rng.integers(BIAS - 30_000, BIAS + 30_000, (4000, 3)), seed=2)
    want_i, _ = check_nearest(D, src, tgt, stride=3)
    assert np.all(want_i[np.arange(5000) % 3 != 0] == R.NONE) and np.all(want_i[::3] != R.NONE)
    want_i, _ = check_nearest(D, src, tgt, max_distance=0.3)           # 1229 quanta: most queries find nothing
    assert 0.5 < np.mean(want_i == R.NONE) < 1.0
    check_nearest(D, src, tgt, stride=3, max_distance=0.6)
    check_nearest(D, src, tgt, max_distance=1e-4)                      # below one quantum: R2 = 0
    check_nearest(D, src, tgt, max_distance=1e6)


def test_nearest_clustered_200k_against_300k(D):
    pytest.importorskip("scipy.spatial")
    fields, _, _ = clustered_scene()
    src = u_stream(fields[:200_000], seed=1)
    tgt = u_stream(fields[300_000:600_000], seed=2)
    check_nearest(D, src, tgt, m=(0.999, 0.02, 0.0, -0.02, 0.999, 0.0, 0.0, 0.0, 1.0, 0.5, 0.25, -0.125), method="tree")


# ---- one step ------------------------------------------------------------------------------------------------------
def blobs(n, seed, centres=20, spread=2.0, sigma=0.15):
    """A clustered cloud in world units, inside a few units of the origin."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (centres, 3))
    return c[rng.integers(0, centres, n)] + rng.normal(0, sigma, (n, 3))


def patches(n, seed, k=10, spread=2.0, size=1.0, thick=0.01):
    """A cloud of k thin planar patches (surfaces, as a capture has them) in world units.  Point-to-point ICP settles in
    a few tens of steps on surfaces; inside volumetric blobs it creeps, the nearest point of a shifted blob lying in
    no particular direction."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (k, 3))
    Q = np.linalg.qr(rng.normal(size=(k, 3, 3)))[0]
    which = rng.integers(0, k, n)
    local = rng.normal(0, 1, (n, 3)) * np.array([size, size, thick])
    return c[which] + np.einsum("nij,nj->ni", Q[which], local)


def cloud_stream(x, fb=12, seed=0):
    return stream_of(fields_of(np.rint(np.asarray(x) * 2.0 ** fb)), fb=fb, seed=seed)


@pytest.mark.parametrize("kw", [dict(overlap=0.7), dict(max_distance=0.05), dict(overlap=0.5, max_distance=0.08, stride=2)],
                         ids=["overlap", "max_distance", "both_strided"])
def test_one_step_inliers_and_moments(D, kw):
    x = blobs(20_000, 4)
    src, tgt = cloud_stream(x, seed=1), cloud_stream(x[::-1] * 1.01 + np.array([0.02, -0.01, 0.015]), seed=2)
    m = (1.0, 0.01, 0.0, -0.01, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
    idx, d2, inlier, mom = D.align_step_packed(*on_device(src), *on_device(tgt), map=m, **kw)
    Ps, fs = R.positions_of(src)
    Pt, ft = R.positions_of(tgt)
    want = R.step(Ps, fs, Pt, ft, m, terms=True, method="tree", **kw)
    assert np.array_equal(idx.cpu().numpy(), want["index"]) and np.array_equal(d2.cpu().numpy(), want["d2"])
    assert np.array_equal(inlier.cpu().numpy(), want["inlier"]), "the inlier set, exactly"
    assert (mom.count, mom.taking_part, mom.candidates) == (want["count"], want["taking_part"], want["candidates"])
    assert 0 < mom.count < mom.taking_part
    assert (mom.sum_d2_hi << 64) + mom.sum_d2_lo == want["sum_d2"]
    # a fixed summation tree of depth ceil(log2 n_s) + 2 at most: |error| <= depth * 2^-53 * sum |term|
    got = np.array(list(mom.sum_a) + list(mom.sum_b) + list(mom.sum_ab) + [mom.sum_aa, mom.sum_bb])
    depth = math.ceil(math.log2(Ps.shape[0])) + 2
    for k in range(17):
        exact = math.fsum(want["terms"][:, k])
        bound = depth * 2.0 ** -53 * math.fsum(np.abs(want["terms"][:, k]))
        print(f"moment {k}: got {got[k]!r} exact {exact!r} bound {bound:.3e}")
        assert abs(got[k] - exact) <= bound, k


# ---- the run -----------------------------------------------------------------------------------------------------
def placed_target(D, src_raw, q, t, s, seed, replace_tail=0.0):
    """transform_packed(source, known) with its points permuted; optionally the last part replaced by an unrelated
    cluster 6 units away."""
    st, sh = on_device(src_raw)
    out, bad = D.transform_packed(st, sh, rotation=q, translation=t, scale=s)
    assert int(bad.item()) == 0
    P = stored_positions(out.cpu().numpy().tobytes())
    rng = np.random.default_rng(seed)
    P = P[rng.permutation(P.shape[0])]
    if replace_tail:
        k = int(P.shape[0] * replace_tail)
        other = patches(k, seed + 1, k=5, spread=0.7, size=0.3) + np.array([6.0, 0.0, 0.0])
        P[-k:] = np.rint(other * 4096.0).astype(np.int64)
    return stream_of(fields_of(P), seed=seed)


# rigid and scaled run at the default 30 steps.  The trimmed case needs 41 on this cloud, and volumetric blobs (the
# nearest point of a shifted blob lies in no particular direction, so point-to-point ICP creeps) need 37: a cap of 200.
KNOWN = {
    "rigid": dict(cloud=patches, angle=0.15, t=(0.3, -0.2, 0.25), s=1.0, opts=dict()),
    "scaled": dict(cloud=patches, angle=0.25, t=(0.3, -0.2, 0.25), s=1.07, opts=dict(estimate_scale=True)),
    "partial": dict(cloud=patches, angle=0.15, t=(0.3, -0.2, 0.25), s=1.05,
                    opts=dict(estimate_scale=True, overlap=0.7, max_iterations=200), tail=0.3),
    "blobs": dict(cloud=blobs, angle=0.15, t=(0.3, -0.2, 0.25), s=1.0, opts=dict(max_iterations=200)),
}


@pytest.mark.parametrize("case", sorted(KNOWN))
def test_run_recovers_a_known_placement(D, case):
    pytest.importorskip("scipy.spatial")
    k = KNOWN[case]
    q = R.axis_angle_quat((1, 2, 3), k["angle"])
    src = cloud_stream(k["cloud"](20_000, 7), seed=1)
    tgt = placed_target(D, src, q, k["t"], k["s"], seed=7, replace_tail=k.get("tail", 0.0))
    got = D.align_packed(*on_device(src), *on_device(tgt), **k["opts"])
    Ps, fs = R.positions_of(src)
    Pt, ft = R.positions_of(tgt)
    want = R.run(Ps, fs, Pt, ft, method="tree", **k["opts"])
    Rt = R.quat_to_matrix(q)
    e_dev = R.map_errors(got["map"], got["scale"], Rt, k["t"], k["s"])
    e_ref = R.map_errors(want["map"], want["scale"], Rt, k["t"], k["s"])
    print(f"{case}: device {e_dev} in {got['iterations']} steps, reference {e_ref} in {want['iterations']} steps")
    assert got["converged"] and want["converged"] and not got["degenerate"]
    quantum = 2.0 ** -ft
    for d, r, what in zip(e_dev, e_ref, ("rotation", "translation", "scale")):
        assert d < quantum, what
        assert d <= 10.0 * r, what
    assert abs(got["iterations"] - want["iterations"]) <= 1
    assert len(got["history"]) == got["iterations"] and got["history"][-1] == (got["fitness"], got["inlier_rmse"], got["inliers"])
    # the quaternion, translation and scale say what the map says (coord UNSPECIFIED: the stored frame)
    m = np.concatenate([(got["scale"] * R.quat_to_matrix(got["rotation"])).reshape(-1), got["translation"]])
    assert np.abs(m - np.array(got["map"])).max() <= 1e-12


def test_initial_placement_in_a_coord_and_the_centroid_start(D):
    """One step from an initial rotation, translation and scale stated in RDF, and from the centroid start: the map the
    run used (reported after one step) is the restatement's to rounding, and the step's numbers are the restatement's
    at the device's map."""
    from spz_amd import abi
    q = R.axis_angle_quat((1, 2, 3), 0.15)
    src = cloud_stream(patches(20_000, 7), seed=1)
    tgt = placed_target(D, src, q, (0.3, -0.2, 0.25), 1.05, seed=7)
    Ps, fs = R.positions_of(src)
    Pt, ft = R.positions_of(tgt)
    init = dict(rotation=(0.02, -0.11, 0.05, 0.9), translation=(0.25, 0.3, -0.2), scale=1.04, coord=abi.RDF)
    for centroids in (False, True):
        got = D.align_packed(*on_device(src), *on_device(tgt), max_iterations=1, stride=3, init_centroids=centroids, **init)
        want = R.initial_map(**init)
        if centroids:
            want = R.centroid_map(Ps, fs, Pt, ft, want, stride=3)
        assert np.abs(np.array(got["map"]) - want).max() <= 1e-13, centroids
        assert got["iterations"] == 1 and not got["converged"]
        step = R.step(Ps, fs, Pt, ft, got["map"], stride=3, method="tree")
        assert got["inliers"] == step["count"] == step["taking_part"]
        assert got["history"] == [R.fitness_rmse(step, ft) + (step["count"],)]
        # the reported rotation, translation and scale are the initial ones, still stated in RDF
        qn = np.array(init["rotation"]) / np.linalg.norm(init["rotation"])
        assert np.abs(np.array(got["rotation"]) - qn).max() <= 1e-14 and got["scale"] == 1.04
        if not centroids:
            assert np.abs(np.array(got["translation"]) - np.array(init["translation"])).max() <= 1e-15
    assert abs(np.linalg.norm(want[9:] - R.initial_map(**init)[9:])) > 0.1, "the centroid start moved the translation"


def test_result_in_rdf_places_the_source_on_the_target(D, spz, tmp_path):
    from spz_amd import abi
    q = R.axis_angle_quat((1, 2, 3), 0.15)
    src = cloud_stream(patches(20_000, 7), seed=1)
    tgt = placed_target(D, src, q, (0.3, -0.2, 0.25), 1.0, seed=7)
    got = D.align_packed(*on_device(src), *on_device(tgt), coord=abi.RDF, max_iterations=200)
    assert got["converged"]
    st, sh = on_device(src)
    out, bad = D.transform_packed(st, sh, rotation=got["rotation"], translation=got["translation"], scale=got["scale"],
                                  coord=abi.RDF)
    assert int(bad.item()) == 0
    tt, th = on_device(tgt)
    oh = abi.peek_header(out.cpu().numpy().tobytes())[1]
    idx, d2 = D.nearest_packed(out, oh, tt, th)
    rmse = math.sqrt(float(d2.cpu().numpy().astype(np.float64).sum()) / sh.num_points) * 2.0 ** -12
    print(f"reported {got['inlier_rmse']!r}, placed {rmse!r}")
    assert abs(rmse - got["inlier_rmse"]) <= 2.0 ** -12


def test_runs_repeat_their_bits_and_the_file_form_agrees(D, spz):
    q = R.axis_angle_quat((3, -1, 2), 0.2)
    src = cloud_stream(blobs(30_000, 12), seed=1)
    tgt = placed_target(D, src, q, (0.1, 0.2, -0.3), 1.04, seed=3, replace_tail=0.2)
    opts = dict(estimate_scale=True, overlap=0.8, max_distance=1.5, stride=2, init_centroids=True)
    a = D.align_packed(*on_device(src), *on_device(tgt), **opts)
    b = D.align_packed(*on_device(src), *on_device(tgt), **opts)
    a.pop("ms"), b.pop("ms")
    assert a == b
    m = a["map"]
    one = D.align_step_packed(*on_device(src), *on_device(tgt), map=m, stride=2, max_distance=1.5, overlap=0.8)
    two = D.align_step_packed(*on_device(src), *on_device(tgt), map=m, stride=2, max_distance=1.5, overlap=0.8)
    for x, y in zip(one[:3], two[:3]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert bytes(one[3]) == bytes(two[3])
    assert one[3].count == a["inliers"]
    f = spz.align_spz(gz(src), gz(tgt), **opts)
    for key in ("rotation", "translation", "scale", "fitness", "inlier_rmse", "inliers", "iterations", "converged",
                "degenerate"):
        assert f[key] == a[key], key
    assert [tuple(h) for h in f["history"]] == a["history"]


def test_degenerate_and_refused_inputs(D, spz, tmp_path):
    line = np.outer(np.arange(-250, 250) * 8, [1, 2, -1])      # stored integers exactly on one line
    src, tgt = stream_of(fields_of(line), seed=1), cloud_stream(blobs(2000, 5), seed=2)
    got = D.align_packed(*on_device(src), *on_device(tgt))
    assert got["degenerate"] and not got["converged"] and got["iterations"] == 1
    assert got["map"] == R.IDENTITY
    (tmp_path / "line.spz").write_bytes(gz(src))
    (tmp_path / "t.spz").write_bytes(gz(tgt))
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_align")
    r = subprocess.run([exe, "line.spz", "t.spz", "--output", "c.spz"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=120)
    assert r.returncode == 2 and not (tmp_path / "c.spz").exists()
    v1 = stream_of(np.zeros((4, 3), np.int64), version=2)
    v1 = v1[:4] + (1).to_bytes(4, "little") + v1[8:]           # the version field: 1
    empty = stream_of(np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError):
        spz.align_spz(gz(src), gz(empty))
    with pytest.raises(ValueError):
        D.align_packed(*on_device(src), *on_device(empty))
    with pytest.raises(ValueError):
        D.nearest_packed(*on_device(v1), *on_device(tgt))
    v1_file = gz(v1[:16] + bytes(4 * 16))                      # a version 1 point is 16 bytes at degree 0
    for a, b in ((v1_file, gz(tgt)), (gz(tgt), v1_file)):
        with pytest.raises(ValueError):
            spz.align_spz(a, b)
    got = D.align_packed(*on_device(empty), *on_device(tgt))   # an empty source: nothing to fit
    assert got["degenerate"] and got["inliers"] == 0 and got["fitness"] == 0.0


def test_cli_round_trip(D, tmp_path):
    q = R.axis_angle_quat((1, 2, 3), 0.15)
    src = cloud_stream(patches(20_000, 7), seed=1)
    tgt = placed_target(D, src, q, (0.3, -0.2, 0.25), 1.05, seed=7)
    (tmp_path / "a.spz").write_bytes(gz(src))
    (tmp_path / "b.spz").write_bytes(gz(tgt))
    bindir = os.path.join(ROOT, "spz_amd", "bin")
    r = subprocess.run([os.path.join(bindir, "spz_align"), "a.spz", "b.spz", "--output", "c.spz", "--scale",
                        "--iterations", "200"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("--rotate ") and lines[1].startswith("fitness ")
    assert abs(float(lines[0].split()[lines[0].split().index("--scale") + 1]) - 1.05) < 1e-4
    r2 = subprocess.run([os.path.join(bindir, "spz_transform"), "a.spz", "d.spz"] + lines[0].split(),
                        capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert (tmp_path / "c.spz").read_bytes() == (tmp_path / "d.spz").read_bytes()


def test_one_million_against_one_million(D):
    """The device's last step against the restatement's single step at the device's reported map, exactly.  The time
    limit is a guard against a walk that degrades to a scan, not a measured figure: ten queries of a million points."""
    pytest.importorskip("scipy.spatial")
    fields, _, _ = clustered_scene()
    src = u_stream(fields, seed=1)
    q = R.axis_angle_quat((1, 2, 3), 0.02)
    P = stored_positions(src).astype(np.float64)               # the scene fills the cube: placed in numpy and clipped
    P = np.rint(P @ R.quat_to_matrix(q).T + np.array([0.5, -0.25, 0.125]) * 4096.0).astype(np.int64)
    P = np.clip(P, -BIAS, BIAS - 1)[np.random.default_rng(9).permutation(P.shape[0])]
    tgt = stream_of(fields_of(P), seed=9)
    st, sh = on_device(src)
    tt, th = on_device(tgt)
    t0 = time.perf_counter()
    got = D.align_packed(st, sh, tt, th, max_iterations=10)
    wall = time.perf_counter() - t0
    print(f"1 M against 1 M, {got['iterations']} steps: {wall:.2f} s, ms {got['ms']}")
    assert wall < 120.0
    Ps, fs = R.positions_of(src)
    Pt, ft = R.positions_of(tgt)
    want = R.step(Ps, fs, Pt, ft, got["map"], method="tree")
    _, _, _, mom = D.align_step_packed(st, sh, tt, th, map=got["map"])
    assert mom.count == want["count"] == got["inliers"]
    assert (mom.sum_d2_hi << 64) + mom.sum_d2_lo == want["sum_d2"]
    assert got["inlier_rmse"] == R.fitness_rmse(want, ft)[1]
