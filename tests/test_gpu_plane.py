"""spz.level_spz / spz_level / spz_amd_plane_* / spz_amd.device.plane_score + plane_moments + plane_mark +
detect_planes_packed (DESIGN §8 "Level") on the GPU, against the restatement of tests/plane_ref.py: the scores, the
moments and the labels count for count, a run on a synthetic room equal to the restatement's run, two runs equal bit for
bit, and the file forms.  The shapes are the smallest at which the kernels take another path: partial waves and plane
groups (63, 64, 65 planes), the score's chunk edge and the moments' tile edge (2047, 2049, 4097 points)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import plane_ref as R
from clean_ref import stored_positions
from conftest import ROOT
from test_filter_host import MAGIC
from test_gpu_clean import gz, on_device, stream_of

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 63, 64, 65, 2047, 2049, 4097]
HS = [1, 63, 64, 65, 1025]
CORNER = 1 << 23


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


def random_points(n, seed, span=20000):
    rng = np.random.default_rng(seed)
    return rng.integers(-span, span, (n, 3))


def random_planes(P, H, seed):
    """H planes through random triples of P (as the hypotheses make them), so that each has inliers of its own."""
    rng = np.random.default_rng(seed)
    n = P.shape[0]
    out = []
    for h in range(H):
        i, j, k = rng.integers(0, n, 3)
        p = R.hypothesis((0, 1, 2), P[i], P[j], P[k])          # repeated points give N = 0: an invalid plane
        if not R.valid(p) and h % 2:
            a, b, c = (int(v) for v in rng.integers(-65536, 65537, 3))
            p = (a, b, c, int(rng.integers(-(1 << 30), 1 << 30)))
        out.append(p)
    return out


def check_score(D, raw, planes, T, stride=1, labels=None):
    import torch
    t, h = on_device(raw)
    lab = None if labels is None else torch.from_numpy(np.asarray(labels, np.uint8)).to("cuda")
    K, S, cost = D.plane_score(t, h, planes, T=T, stride=stride, labels=lab)
    Q, _ = R.prepare(stored_positions(raw), stride, labels)
    want = R.score(Q, planes, T)
    got = list(zip(K.cpu().tolist(), S.cpu().tolist(), [c & R.MASK64 for c in cost.cpu().tolist()]))
    assert got == want
    return want


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_score_against_the_restatement(D, n, H):
    P = random_points(n, 100 * n + H)
    planes = random_planes(P, H, n + H)
    check_score(D, stream_of(fields_of(P), seed=n), planes, T=R.threshold(0.01, 12))


def test_score_at_the_threshold_and_at_zero(D):
    # d = Y - 7 for the plane (0, 1, 0, 7): points at |d| = T and T + 1 on both sides, and on the plane
    T = 100
    ys = [7 + T, 7 + T + 1, 7 - T, 7 - T - 1, 7, 7, 8, 6]
    P = np.array([(k * 11, y, -k) for k, y in enumerate(ys)], np.int64)
    raw = stream_of(fields_of(P))
    planes = [(0, 1, 0, 7), (0, -1, 0, -7), (0, 65536, 0, 7 * 65536)]
    want = check_score(D, raw, planes, T=T)
    assert want[0] == (6, 2 * T + 2, 2 * T + 2 + 2 * T) and want[1] == want[0]
    assert want[2][0] == 2                                     # d = 65536 (Y - 7): only the points on the plane
    want = check_score(D, raw, planes, T=0)
    assert [w[0] for w in want] == [2, 2, 2] and all(w[1] == 0 and w[2] == 0 for w in want)
    want = check_score(D, raw, planes, T=1 << 36)
    assert all(w[0] == 8 for w in want)


def test_score_with_invalid_planes_among_valid_ones(D):
    P = random_points(500, 1)
    planes = random_planes(P, 130, 2)
    for h in (0, 63, 64, 129):
        planes[h] = (0, 0, 0, 12345)
    planes[5] = (0, 65537, 0, 0)                               # out of range: invalid too
    planes[6] = (0, 65536, 0, (1 << 42) + 1)
    want = check_score(D, stream_of(fields_of(P)), planes, T=50000)
    for h in (0, 5, 6, 63, 64, 129):
        assert want[h] == (0, 0, R.MASK64)
    assert sum(c != R.MASK64 for _, _, c in want) >= 100


def test_score_at_the_cube_corners_has_no_overflow(D):
    lo, hi = -CORNER, CORNER - 1
    P = np.array([(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.int64)
    raw = stream_of(fields_of(P))
    planes = []
    for sa in (-65536, 65536):
        for sb in (-65536, 65536):
            for sc in (-65536, 65536):
                for e in (3 << 39, -(3 << 39), 1 << 42, -(1 << 42), 0):
                    planes.append((sa, sb, sc, e))
    d = np.array([[abs(int(a) * int(p[0]) + int(b) * int(p[1]) + int(c) * int(p[2]) - e) for p in P]
                  for a, b, c, e in planes], object)
    assert int(d.max()) > 1 << 42 and int(d.max()) < 1 << 43
    for T in (1 << 36, 0, 65536 * 3):
        want = check_score(D, raw, planes, T=T)
    assert any(K > 0 for K, _, _ in want), "the planes through the corners themselves"


def test_score_with_stride_and_labels(D):
    P = random_points(3001, 7)
    raw = stream_of(fields_of(P))
    planes = random_planes(P, 70, 8)
    T = R.threshold(0.02, 12)
    check_score(D, raw, planes, T, stride=3)
    labels = (np.random.default_rng(9).random(3001) < 0.4).astype(np.uint8) * 2
    check_score(D, raw, planes, T, labels=labels)
    check_score(D, raw, planes, T, stride=3, labels=labels)
    check_score(D, raw, planes, T, stride=5000)                # one point takes part
    everything = np.ones(3001, np.uint8)
    import torch
    t, h = on_device(raw)
    ws, m = D.plane_prepare(t, h, labels=torch.from_numpy(everything).to("cuda"))
    assert m == 0
    K, S, cost = D.plane_score(t, h, planes[:3], T=T, prepared=(ws, m))
    assert K.tolist() == [0, 0, 0] and S.tolist() == [0, 0, 0]


def test_prepare_and_gather(D):
    import torch
    P = random_points(2500, 11, span=CORNER)
    raw = stream_of(fields_of(P), deg=1, seed=3)
    t, h = on_device(raw)
    labels = (np.arange(2500) % 7 == 0).astype(np.uint8)
    prep = D.plane_prepare(t, h, stride=2, labels=torch.from_numpy(labels).to("cuda"))
    Q, _ = R.prepare(stored_positions(raw), 2, labels)
    assert prep[1] == Q.shape[0]
    idx = np.random.default_rng(1).integers(0, Q.shape[0], 777)
    got = D.plane_gather(prep, h, idx).cpu().numpy()
    assert np.array_equal(got, Q[idx])
    with pytest.raises(ValueError):
        D.plane_gather(prep, h, [Q.shape[0]])


def check_moments(D, raw, plane, T, **kw):
    t, h = on_device(raw)
    got = D.plane_moments(t, h, plane, T=T, **kw)
    Q, _ = R.prepare(stored_positions(raw), kw.get("stride", 1))
    want = R.moments(Q, plane, T)
    for k in ("count", "sum_abs", "above", "below", "points", "sum_p", "sum_pp"):
        assert got[k] == want[k], k
    return got


@pytest.mark.parametrize("n", NS)
def test_moments_against_python_ints(D, n):
    P = random_points(n, 50 + n, span=CORNER)               # all of the cube: products near 2^46
    raw = stream_of(fields_of(P), seed=n)
    plane = (20000, -50000, 37000, 123456789)
    got = check_moments(D, raw, plane, T=1 << 36)
    check_moments(D, raw, plane, T=0)
    check_moments(D, raw, (0, 65536, 0, 0), T=1 << 36, stride=2)
    if n >= 2047:
        assert 0 < got["count"] < n and got["above"] and got["below"]


def test_moments_carry_past_2_64(D):
    n = (1 << 18) + 1
    P = np.tile(np.array([(-CORNER, -CORNER, CORNER - 1)], np.int64), (n, 1))
    raw = stream_of(fields_of(P))
    got = check_moments(D, raw, (0, 65536, 0, -CORNER * 65536), T=0)
    assert got["count"] == n and got["sum_pp"][0] == n << 46 and got["sum_pp"][0] > 1 << 64
    assert got["sum_pp"][2] < -(1 << 63), "a negative 128-bit sum"
    assert got["struct"].sum_pp_hi[0] == 1 and got["struct"].sum_pp_hi[2] < 0
    got = check_moments(D, raw, (0, 65536, 0, -CORNER * 65536 + 1), T=0)
    assert got["count"] == 0 and got["below"] == n and got["sum_pp"] == [0] * 6


def test_mark(D):
    import torch
    P = random_points(4097, 21)
    raw = stream_of(fields_of(P))
    t, h = on_device(raw)
    plane, T = (3000, 65000, -7000, 40000), R.threshold(0.5, 12)
    before = np.random.default_rng(2).integers(0, 2, 4097).astype(np.uint8) * 9
    labels = torch.from_numpy(before.copy()).to("cuda")
    # the points whose label is 0 and whose index is even take part; their inliers get 5
    out = D.plane_mark(t, h, plane, 5, labels, T=T, stride=2, labels=labels.clone())
    assert out is labels
    Q, index = R.prepare(stored_positions(raw), 2, before)
    inl = np.abs(R.distances(Q, plane)) <= T
    want = before.copy()
    want[index[inl]] = 5
    assert 50 < inl.sum() < Q.shape[0]
    assert np.array_equal(labels.cpu().numpy(), want), "inliers marked, every other point keeps its value"


# ---- the run ---------------------------------------------------------------------------------------------------------
TAU = 0.001
EXTENT = 4.0


def room(seed=5):
    """About 6 000 points at 12 fractional bits: 3 000 on a floor 4 units square with +-2 grid steps of noise, 1 500 on a
    wall, 1 500 of clutter above the floor, turned by a known rotation and shuffled.  Returns (raw stream, kind per
    point: 0 floor, 1 wall, 2 clutter, the floor's true normal, the rotation)."""
    rng = np.random.default_rng(seed)
    step = 2.0 ** -12
    half = EXTENT / 2
    floor = np.stack([rng.uniform(-half, half, 3000), rng.integers(-2, 3, 3000) * step, rng.uniform(-half, half, 3000)], 1)
    wall = np.stack([-half + rng.integers(-2, 3, 1500) * step, rng.uniform(0.0, 2.5, 1500), rng.uniform(-half, half, 1500)], 1)
    clutter = np.stack([rng.uniform(-half, half, 1500), rng.uniform(0.05, 2.5, 1500), rng.uniform(-half, half, 1500)], 1)
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    ang = 0.6
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * Kx @ Kx
    pts = np.concatenate([floor, wall, clutter]) @ Rm.T + np.array([0.3, -0.2, 0.5])
    kind = np.concatenate([np.zeros(3000, int), np.ones(1500, int), np.full(1500, 2)])
    perm = rng.permutation(6000)
    P = np.rint(pts[perm] * 4096.0).astype(np.int64)
    assert np.abs(P).max() < CORNER
    return stream_of(fields_of(P), deg=1, fb=12, seed=seed), kind[perm], Rm @ np.array([0.0, 1.0, 0.0]), Rm


@pytest.fixture(scope="module")
def scene():
    raw, kind, normal, Rm = room()
    want, labels = R.run_stream(raw, TAU, hypotheses_count=256)
    return dict(raw=raw, kind=kind, normal=normal, Rm=Rm, want=want, labels=labels)


def same_plane(got, want):
    assert tuple(got["integers"]) == tuple(want["plane"])
    for k in ("inliers", "sum_abs", "points", "above", "below", "best_hypothesis", "refinements"):
        assert got[k] == want[k], k
    assert got["fitness"] == want["fitness"] and got["mean_distance"] == want["mean_distance"]
    assert list(got["normal"]) == want["normal"] and got["offset"] == want["offset"]
    assert list(got["rotation"]) == want["rotation"] and list(got["translation"]) == want["translation"]


def test_run_on_a_synthetic_room(D, scene):
    want = scene["want"]
    # a fair input: the restatement's winning triple lies on the floor (with half the points there a miss in 256 draws
    # has probability about 1e-15)
    assert len(want) == 1 and all(scene["kind"][i] == 0 for i in want[0]["triple"])
    t, h = on_device(scene["raw"])
    got = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256)
    assert len(got["planes"]) == 1 and got["threshold"] == R.threshold(TAU, 12)
    same_plane(got["planes"][0], want[0])
    assert np.array_equal(got["labels"].cpu().numpy(), scene["labels"]), "the labels"
    p = got["planes"][0]
    assert p["inliers"] >= 2900 and p["above"] > p["below"]
    # the recovered normal: within atan(2 tau / L) of the true one, the most a plane holding those inliers can tilt
    n = np.array(p["normal"])
    angle = math.acos(min(1.0, abs(float(n @ scene["normal"]))))
    assert angle <= math.atan(2 * TAU / EXTENT)
    assert float(n @ scene["normal"]) > 0, "the scene lies on the positive side of its floor"
    # two runs are equal bit for bit
    again = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256)
    assert again["planes"] == got["planes"] and np.array_equal(again["labels"].cpu().numpy(), scene["labels"])


def test_run_finds_floor_then_wall_then_stops(D, scene):
    kw = dict(seed=3, stride=1, refine=2, min_inliers=800)
    want, labels = R.run_stream(scene["raw"], TAU, hypotheses_count=256, max_planes=3, **kw)
    assert len(want) == 2
    t, h = on_device(scene["raw"])
    got = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256, planes=3, **kw)
    assert len(got["planes"]) == 2
    for g, w in zip(got["planes"], want):
        same_plane(g, w)
    assert np.array_equal(got["labels"].cpu().numpy(), labels)
    lab = got["labels"].cpu().numpy()
    kind = scene["kind"]
    assert (lab[kind == 0] == 1).mean() > 0.95 and (lab[kind == 1] == 2).mean() > 0.95
    assert got["planes"][1]["points"] == 6000 - got["planes"][0]["inliers"]
    wall_normal = scene["Rm"] @ np.array([1.0, 0.0, 0.0])
    assert abs(float(np.array(got["planes"][1]["normal"]) @ wall_normal)) > 0.999
    # a fraction of the points taking part is the same floor
    frac = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256, planes=3, seed=3, refine=2, min_inliers=800 / 6000)
    assert frac["planes"] == got["planes"]
    # an axis the floor is far from, an up hint that turns it over, a frame with Y down
    hint = tuple(-scene["normal"])
    flipped = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256, up_hint=hint)
    w2, _ = R.run_stream(scene["raw"], TAU, hypotheses_count=256, up_hint=hint)
    same_plane(flipped["planes"][0], w2[0])
    assert tuple(flipped["planes"][0]["integers"]) == tuple(-v for v in scene["want"][0]["plane"])
    fl = np.array(R.flips(7))
    wall_axis = tuple(fl * wall_normal)                        # stated in LUF
    constrained = D.detect_planes_packed(t, h, threshold=TAU, hypotheses=256, axis=wall_axis, max_tilt=10.0, coord=7)
    w3, _ = R.run_stream(scene["raw"], TAU, hypotheses_count=256, axis=wall_axis, max_tilt=10.0, coord=7)
    same_plane(constrained["planes"][0], w3[0])
    assert abs(float(np.array(constrained["planes"][0]["normal"]) @ np.array(wall_axis))) > 0.999, "the wall, not the floor"


# ---- the file forms --------------------------------------------------------------------------------------------------
def test_level_spz_file_to_file(spz, scene, tmp_path):
    src, dst = tmp_path / "in.spz", tmp_path / "level.spz"
    src.write_bytes(gz(scene["raw"]))
    r = spz.level_spz(str(src), str(dst), threshold=TAU, hypotheses=256)
    assert len(r["planes"]) == 1 and r["kept"] is None
    same_plane(r["planes"][0], scene["want"][0])
    assert np.array_equal(r["labels"], scene["labels"])
    assert r["rotation"] == r["planes"][0]["rotation"] and r["scale"] == 1.0
    # the file is transform_spz's with that placement
    ref = tmp_path / "ref.spz"
    spz.transform_spz(str(src), str(ref), rotation=r["rotation"], translation=r["translation"])
    assert dst.read_bytes() == ref.read_bytes()
    # the levelled file's floor points decode within tau of height 0
    cloud = spz.load_spz(str(dst))
    y = np.asarray(cloud.positions, np.float64).reshape(-1, 3)[:, 1]
    assert y.shape[0] == 6000
    assert np.abs(y[scene["kind"] == 0]).max() <= TAU
    assert (y[scene["kind"] == 2] > 0).mean() > 0.99, "the clutter stands on the floor"
    # no output: the planes alone; bytes in
    only = spz.level_spz(src.read_bytes(), threshold=TAU, hypotheses=256)
    assert only["planes"] == r["planes"]
    # no plane reaches the floor of inliers: nothing is written
    none = spz.level_spz(str(src), str(tmp_path / "none.spz"), threshold=TAU, hypotheses=256, min_inliers=5000)
    assert none["planes"] == [] and none["rotation"] is None and not (tmp_path / "none.spz").exists()


def test_spz_level_select_off_plane_is_the_filters_mask(spz, scene, tmp_path):
    src, dst, ref = tmp_path / "in.spz", tmp_path / "off.spz", tmp_path / "ref.spz"
    src.write_bytes(gz(scene["raw"]))
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_level")
    r = subprocess.run([exe, str(src), str(dst), "--threshold", repr(TAU), "--hypotheses", "256", "--select", "off-plane"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plane = scene["want"][0]["plane"]
    d = R.distances(stored_positions(scene["raw"]), plane)
    T = R.threshold(TAU, 12)
    spz.filter_spz(str(src), str(ref), mask=np.abs(d) > T)
    assert dst.read_bytes() == ref.read_bytes(), "byte for byte filter_spz with the restatement's mask"
    lines = r.stdout.splitlines()
    assert lines[0].startswith("plane 1 normal ") and lines[0].endswith("integers %d %d %d %d" % plane)
    assert lines[1].startswith("--rotate ") and " --translate " in lines[1] and lines[1].endswith(" --scale 1 --coord UNSPECIFIED")
    assert lines[2] == "kept %d" % int((np.abs(d) > T).sum())
    want = scene["want"][0]
    assert [float(v) for v in lines[1].split()[1:5]] == want["rotation"]
    # above: what stands on the floor, without the floor
    for select, mask in (("above", d > T), ("below", d < -T), ("plane", np.abs(d) <= T)):
        out = tmp_path / (select + ".spz")
        got = spz.level_spz(str(src), str(out), threshold=TAU, hypotheses=256, select=select)
        assert got["kept"] == int(mask.sum())
        spz.filter_spz(str(src), str(ref), mask=mask)
        assert out.read_bytes() == ref.read_bytes(), select
    # exit status 2 when no plane reaches --min-inliers
    r = subprocess.run([exe, str(src), str(tmp_path / "none.spz"), "--threshold", repr(TAU), "--hypotheses", "256",
                        "--min-inliers", "0.9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "" and not (tmp_path / "none.spz").exists()


def test_version_1_is_unsupported(spz, D, tmp_path):
    import ctypes as C
    from spz_amd import abi
    n = 50
    raw = struct.pack("<IIIBBBB", MAGIC, 1, n, 0, 12, 0, 0) + bytes(n * (6 + 1 + 3 + 3 + 3))
    t, h = on_device(raw)
    assert h.version == 1
    o = abi.PlaneOptions()
    L = abi.load_library()
    assert L.spz_amd_plane_default_options(C.byref(o)) == abi.OK
    o.threshold = 0.1
    res, found = (abi.PlaneResult * 1)(), C.c_uint32(7)
    assert L.spz_amd_plane_host(t.data_ptr(), t.numel(), C.byref(h), C.byref(o), 0, res, 1, C.byref(found), None,
                                None) == abi.ERR_UNSUPPORTED
    assert found.value == 0
    with pytest.raises(ValueError, match="version 1"):
        D.detect_planes_packed(t, h, threshold=0.1)
    src = tmp_path / "v1.spz"
    src.write_bytes(gz(raw))
    with pytest.raises(ValueError, match="refused"):
        spz.level_spz(str(src), threshold=0.1)
    with pytest.raises(ValueError, match="refused"):
        spz.level_spz(str(src), str(tmp_path / "out.spz"), threshold=0.1)
    assert not (tmp_path / "out.spz").exists()
