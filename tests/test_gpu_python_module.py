"""Behaviour of the Python module `spz_amd.spz` (pybind11 over the C++ drop-in layer over the C ABI)
on a GPU.  The cases restate what the reference's own suite pins for this path
(/root/reference/tests/python/load_spz_test.py; line numbers cited per test) with the same inputs
and tolerances, and add byte-level checks the reference's suite does not have: the .spz file
bytes must equal the bytes the reference's saveSpz produced (golden vectors)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import FIELDS, assert_bits_equal, load_golden

pytestmark = pytest.mark.gpu

SH_4BIT_EPSILON = 2.0 / 32.0 + 0.5 / 255.0   # load_spz_test.py:106
SH_5BIT_EPSILON = 2.0 / 64.0 + 0.5 / 255.0   # load_spz_test.py:107


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def two_point_cloud(spz, with_sh):
    """make_test_gaussian_cloud, load_spz_test.py:72-100."""
    c = spz.GaussianCloud()
    c.antialiased = True
    c.positions = np.array([0, 0.1, -0.2, 0.3, 0.4, 0.5])
    c.scales = np.array([-3, -2, -1.5, -1, 0, 0.1])
    c.rotations = np.array([-0.5, 0.2, 1, -0.2, 0.1, -0.4, -0.3, 0.5])
    c.alphas = np.array([-1.0, 1.0])
    c.colors = np.array([-1, 0, 1, -0.5, 0.5, 0.1])
    if with_sh:
        c.sh_degree = 3
        c.sh = np.array([i / 45.0 - 1.0 for i in range(90)])
    else:
        c.sh_degree = 0
        c.sh = np.array([], dtype=np.float32)
    return c


def rotate(q_xyzw, v):
    x, y, z, w = q_xyzw
    u = np.array([x, y, z])
    return v + 2 * np.cross(u, np.cross(u, v) + w * v)


def test_file_bytes_equal_reference_save_spz(spz, tmp_path):
    """.spz bytes (gzip container included) == the reference's for the same cloud."""
    g = load_golden("kat_small.npz")
    for with_sh, key in ((True, "two_gz_from0"), (False, "two_sh0_gz")):
        f = str(tmp_path / f"two_{with_sh}.spz")
        assert spz.save_spz(two_point_cloud(spz, with_sh), spz.PackOptions(), f) is True
        assert open(f, "rb").read() == g[key].tobytes()
        assert spz._save_spz_bytes(two_point_cloud(spz, with_sh), spz.PackOptions()) == g[key].tobytes()
    f = str(tmp_path / "empty.spz")
    assert spz.save_spz(spz.GaussianCloud(), spz.PackOptions(), f) is True
    assert open(f, "rb").read() == g["empty_gz"].tobytes()
    raw = spz._pack_to_stream(two_point_cloud(spz, True), spz.PackOptions())
    assert raw == g["two_stream_from0"].tobytes()
    # and the reference's own file decodes to the reference's own floats
    for to in range(9):
        o = spz.UnpackOptions()
        o.to_coord = spz.CoordinateSystem(to)
        c = spz._load_spz_bytes(g["two_gz_from0"].tobytes(), o)
        for k in FIELDS:
            assert_bits_equal(getattr(c, k), g[f"two_dec_to{to}_{k}"], f"to={to} {k}")


def test_save_load_round_trip_tolerances(spz, tmp_path):
    """load_spz_test.py:113-150."""
    src = two_point_cloud(spz, True)
    f = str(tmp_path / "rt.spz")
    assert spz.save_spz(src, spz.PackOptions(), f) is True
    dst = spz.load_spz(f, spz.UnpackOptions())
    assert (dst.num_points, dst.sh_degree, dst.antialiased) == (2, 3, True)
    np.testing.assert_allclose(dst.positions, src.positions, atol=1 / 2048.0)
    np.testing.assert_allclose(dst.scales, src.scales, atol=1 / 32.0)
    for i in range(2):
        q = dst.rotations[4 * i:4 * i + 4].astype(float)
        q0 = src.rotations[4 * i:4 * i + 4].astype(float)
        q0 /= np.linalg.norm(q0)
        assert abs(np.linalg.norm(q) - 1.0) < 1e-6
        for v in (np.array([3.0, -2.0, 0.2]), np.array([-1.0, 0.5, -3.0])):
            a, b = rotate(q, v), rotate(q0, v)
            assert abs(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) - 1.0) < 1e-4
    np.testing.assert_allclose(dst.alphas, src.alphas, atol=0.01)
    np.testing.assert_allclose(dst.sh, src.sh, atol=SH_4BIT_EPSILON)
    np.testing.assert_allclose(dst.sh[0:9], src.sh[0:9], atol=SH_5BIT_EPSILON)
    np.testing.assert_allclose(dst.sh[45:54], src.sh[45:54], atol=SH_5BIT_EPSILON)


def test_large_splat_round_trip(spz, tmp_path):
    """load_spz_test.py:152-178: 50 k points, SH3, default_rng(1), documented draw order."""
    n = 50000
    src = spz.GaussianCloud()
    src.sh_degree = 3
    rng = np.random.default_rng(1)
    src.positions = (rng.uniform(0.0, 1.0, size=(n, 3)) * 2.0 - 1.0).flatten()
    src.scales = (rng.uniform(0.0, 1.0, size=(n, 3)) - 1.0).flatten()
    src.rotations = (rng.uniform(0.0, 1.0, size=(n, 4)) * 2.0 - 1.0).flatten()
    src.colors = rng.uniform(0.0, 1.0, size=(n, 3)).flatten()
    src.alphas = rng.uniform(0.0, 1.0, size=n)
    src.sh = (rng.uniform(0.0, 1.0, size=(n, 45)) - 0.5).flatten()
    f = str(tmp_path / "large.spz")
    assert spz.save_spz(src, spz.PackOptions(), f) is True
    dst = spz.load_spz(f, spz.UnpackOptions())
    assert dst.num_points == n and dst.sh_degree == 3
    np.testing.assert_allclose(dst.positions, src.positions, atol=1 / 2048.0)
    np.testing.assert_allclose(dst.scales, src.scales, atol=1 / 16.0)
    assert len(dst.rotations) == len(src.rotations)
    np.testing.assert_allclose(dst.alphas, src.alphas, atol=0.01)
    np.testing.assert_allclose(dst.sh, src.sh, atol=2.0 / 32.0 + 1.0 / 255.0)


def test_sh_zero_and_edge_values(spz, tmp_path):
    """load_spz_test.py:180-207 (exact known answers)."""
    src = spz.GaussianCloud()
    src.sh_degree = 1
    src.positions = np.zeros(3)
    src.scales = np.zeros(3)
    src.rotations = np.array([0, 0, 0, 1.0])
    src.alphas = np.array([0.0])
    src.colors = np.zeros(3)
    src.sh = np.array([-0.01, 0.0, 0.01, -1.0, -0.99, -0.95, 0.95, 0.99, 1.0])
    f = str(tmp_path / "edges.spz")
    assert spz.save_spz(src, spz.PackOptions(), f) is True
    dst = spz.load_spz(f, spz.UnpackOptions())
    assert dst.num_points == 1 and dst.sh_degree == 1
    np.testing.assert_allclose(dst.sh, [0.0, 0.0, 0.0, -1.0, -1.0, -0.9375, 0.9375, 0.9922, 0.9922], atol=2e-5)


@pytest.mark.parametrize("with_sh", [False, True])
def test_ply_round_trip_is_exact(spz, tmp_path, with_sh):
    """load_spz_test.py:209-231 and :889-906."""
    src = two_point_cloud(spz, with_sh)
    f = str(tmp_path / "rt.ply")
    assert spz.save_splat_to_ply(src, spz.PackOptions(), f) is True
    assert open(f, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\n")
    dst = spz.load_splat_from_ply(f, spz.UnpackOptions())
    assert dst.num_points == 2 and dst.sh_degree == (3 if with_sh else 0)
    for k in FIELDS:
        assert np.array_equal(getattr(dst, k), getattr(src, k)), k


def test_coordinate_conversion_through_files(spz, tmp_path):
    """load_spz_test.py:444-512."""
    c = spz.GaussianCloud()
    c.sh_degree = 1
    c.positions = np.array([1.0, 2.0, 3.0], np.float32)
    c.scales = np.array([0.1, 0.2, 0.3], np.float32)
    c.rotations = np.array([0.1, 0.2, 0.3, 0.9], np.float32)
    c.alphas = np.array([0.5], np.float32)
    c.colors = np.array([0.1, 0.2, 0.3], np.float32)
    c.sh = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], np.float32)
    po, uo = spz.PackOptions(), spz.UnpackOptions()
    po.from_coord, uo.to_coord = spz.RUB, spz.RDF
    f = str(tmp_path / "c1.spz")
    assert spz.save_spz(c, po, f) is True
    d = spz.load_spz(f, uo)
    np.testing.assert_allclose(d.positions, [1.0, -2.0, -3.0], atol=1 / 2048.0)
    want = np.array([0.1, -0.2, -0.3, 0.9])
    np.testing.assert_allclose(d.rotations / np.linalg.norm(d.rotations), want / np.linalg.norm(want), atol=1e-3)
    c.sh_degree = 0
    c.sh = np.array([], np.float32)
    po.from_coord, uo.to_coord = spz.RDF, spz.LUF
    f = str(tmp_path / "c2.spz")
    assert spz.save_spz(c, po, f) is True
    np.testing.assert_allclose(spz.load_spz(f, uo).positions, [-1.0, -2.0, 3.0], atol=1 / 2048.0)


def test_sh_flip_is_consistent_across_round_trips(spz, tmp_path):
    """load_spz_test.py:550-602."""
    c = spz.GaussianCloud()
    c.sh_degree = 1
    c.positions = np.array([1.0, 2.0, 3.0])
    c.scales = np.array([0.1, 0.2, 0.3])
    c.rotations = np.array([0.0, 0.0, 0.0, 1.0])
    c.alphas = np.array([0.5])
    c.colors = np.array([0.1, 0.2, 0.3])
    sh0 = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0], np.float32)
    c.sh = sh0
    po, uo = spz.PackOptions(), spz.UnpackOptions()
    po.from_coord, uo.to_coord = spz.RUB, spz.RDF
    f = str(tmp_path / "s1.spz")
    assert spz.save_spz(c, po, f) is True
    a = spz.load_spz(f, uo)
    assert len(a.sh) == 9 and not np.array_equal(a.sh, sh0)
    po.from_coord = spz.RDF
    f2 = str(tmp_path / "s2.spz")
    assert spz.save_spz(a, po, f2) is True
    b = spz.load_spz(f2, uo)
    np.testing.assert_array_almost_equal(a.sh, b.sh, decimal=4)


def test_quaternions_are_normalised_by_packing(spz, tmp_path):
    """load_spz_test.py:605-656."""
    c = spz.GaussianCloud()
    c.positions = np.arange(1.0, 7.0)
    c.scales = np.arange(1, 7) / 10.0
    c.alphas = np.array([0.5, 0.7])
    c.colors = np.arange(1, 7) / 10.0
    q = np.array([2.0, 3.0, 4.0, 5.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    c.rotations = q
    f = str(tmp_path / "q.spz")
    assert spz.save_spz(c, spz.PackOptions(), f) is True
    d = spz.load_spz(f, spz.UnpackOptions())
    for i in range(2):
        got = d.rotations[4 * i:4 * i + 4]
        want = q[4 * i:4 * i + 4] / np.linalg.norm(q[4 * i:4 * i + 4])
        assert abs(np.linalg.norm(got) - 1.0) < 1e-4
        assert np.allclose(got, want, atol=1e-2) or np.allclose(got, -want, atol=1e-2)


def test_in_place_coordinate_methods(spz):
    """load_spz_test.py:375-400, :659-675, :753-761."""
    c = spz.GaussianCloud()
    c.positions = np.array([1.0, 2.0, 3.0], np.float32)
    c.rotations = np.array([0.1, 0.2, 0.3, 0.9], np.float32)
    c.rotate_180_deg_about_x()
    np.testing.assert_array_equal(c.positions, np.float32([1.0, -2.0, -3.0]))
    np.testing.assert_array_equal(c.rotations, np.float32([0.1, -0.2, -0.3, 0.9]))
    c.convert_coordinates(spz.RDF, spz.RUB)
    np.testing.assert_array_equal(c.positions, np.float32([1.0, 2.0, 3.0]))
    np.testing.assert_array_equal(c.rotations, np.float32([0.1, 0.2, 0.3, 0.9]))
    e = spz.GaussianCloud()
    e.rotate_180_deg_about_x()  # empty cloud: no-op, no crash
    np.testing.assert_almost_equal(e.median_volume(), 0.01, decimal=5)


def test_compression_precision(spz, tmp_path):
    """load_spz_test.py:698-750."""
    c = spz.GaussianCloud()
    c.sh_degree = 1
    c.positions = np.array([1.0, -1.0, 0.5])
    c.scales = np.array([1.0, -1.0, 0.5])
    c.rotations = np.array([0.1, 0.2, 0.3, 0.9])
    c.alphas = np.array([0.5])
    c.colors = np.array([0.5, -0.5, 0.25])
    c.sh = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9])
    f = str(tmp_path / "p.spz")
    assert spz.save_spz(c, spz.PackOptions(), f) is True
    d = spz.load_spz(f, spz.UnpackOptions())
    np.testing.assert_allclose(d.positions, c.positions, atol=1 / 2048.0)
    np.testing.assert_allclose(d.scales, c.scales, atol=1 / 32.0)
    assert abs(np.linalg.norm(d.rotations) - 1.0) < 1e-4
    np.testing.assert_allclose(d.alphas, c.alphas, atol=0.01)
    np.testing.assert_allclose(d.colors, c.colors, atol=0.01)
    np.testing.assert_allclose(d.sh[0:9], c.sh[0:9], atol=SH_5BIT_EPSILON)


def test_error_conventions_for_files(spz, tmp_path):
    """load_spz_test.py:842-863: bad path -> False; missing / garbage file -> empty cloud."""
    c = two_point_cloud(spz, False)
    assert spz.save_spz(c, spz.PackOptions(), "/invalid/path/that/does/not/exist/test.spz") is False
    d = spz.load_spz("non_existent_file.spz", spz.UnpackOptions())
    assert d.num_points == 0 and d.sh_degree == 0
    f = str(tmp_path / "garbage.spz")
    with open(f, "w") as fh:
        fh.write("This is not a valid SPZ file")
    d = spz.load_spz(f, spz.UnpackOptions())
    assert d.num_points == 0 and d.sh_degree == 0


def test_inconsistent_cloud_saves_a_zero_point_file(spz, tmp_path):
    """Quirk kept on purpose: packGaussians returns an empty PackedGaussians when checkSizes fails
    (load-spz.cc:258-260) and saveSpz still writes it and succeeds (:598-607)."""
    c = spz.GaussianCloud()
    c.positions = np.zeros(6, np.float32)  # 2 points, every other array left empty
    f = str(tmp_path / "quirk.spz")
    assert spz.save_spz(c, spz.PackOptions(), f) is True
    d = spz.load_spz(f, spz.UnpackOptions())
    assert d.num_points == 0


def test_save_load_cycles_are_stable(spz, tmp_path):
    """load_spz_test.py:866-886, strengthened: after the first cycle the file bytes are a fixed point."""
    cur = two_point_cloud(spz, True)
    f = str(tmp_path / "cycle.spz")
    prev = None
    for _ in range(3):
        assert spz.save_spz(cur, spz.PackOptions(), f) is True
        data = open(f, "rb").read()
        cur = spz.load_spz(f, spz.UnpackOptions())
        assert cur.num_points == 2 and cur.sh_degree == 3 and cur.antialiased is True
        if prev is not None:
            assert data == prev
        prev = data


def test_timing_bounds_of_the_reference_suite(spz, tmp_path):
    """load_spz_test.py:775-807: 10 k points SH2, save < 5 s and load < 5 s."""
    import time
    n = 10000
    c = spz.GaussianCloud()
    c.sh_degree = 2
    rng = np.random.default_rng(42)
    c.positions = rng.uniform(-1.0, 1.0, n * 3).astype(np.float32)
    c.scales = rng.uniform(-2.0, 2.0, n * 3).astype(np.float32)
    c.rotations = rng.uniform(-1.0, 1.0, n * 4).astype(np.float32)
    c.alphas = rng.uniform(0.0, 1.0, n).astype(np.float32)
    c.colors = rng.uniform(0.0, 1.0, n * 3).astype(np.float32)
    c.sh = rng.uniform(-0.5, 0.5, n * 24).astype(np.float32)
    f = str(tmp_path / "perf.spz")
    spz.save_spz(c, spz.PackOptions(), f)  # first call pays the one-time table upload
    t0 = time.time()
    assert spz.save_spz(c, spz.PackOptions(), f) is True
    assert time.time() - t0 < 5.0
    t0 = time.time()
    d = spz.load_spz(f, spz.UnpackOptions())
    assert time.time() - t0 < 5.0 and d.num_points == n


@pytest.mark.parametrize("order", ["module_first", "torch_first"])
def test_one_hip_runtime_whatever_the_import_order(spz, order):
    """PyTorch-ROCm bundles its own libamdhip64; a process that mapped the system copy first (through
    libspz_amd.so) and torch's second had two runtimes and the later one saw no device.  Both orders
    must work, in a fresh process each."""
    import subprocess
    import sys
    first, second = ("import spz_amd.spz as spz", "import torch") if order == "module_first" else \
                    ("import torch", "import spz_amd.spz as spz")
    code = "\n".join([
        first, second,
        "import numpy as np, os",
        "from spz_amd import abi",
        "assert torch.cuda.is_available()",
        "L = abi.load_library()",
        "assert L.spz_amd_device_count() >= 1, L.spz_amd_last_hip_error()",
        "x = torch.arange(8, device='cuda').sum().item(); assert x == 28",
        "c = spz.GaussianCloud(); c.positions = np.zeros(3); c.scales = np.zeros(3)",
        "c.rotations = np.array([0, 0, 0, 1.0]); c.alphas = np.zeros(1); c.colors = np.zeros(3)",
        "b = spz._save_spz_bytes(c, spz.PackOptions()); assert spz._load_spz_bytes(b, spz.UnpackOptions()).num_points == 1",
        "maps = {l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}",
        "assert len(maps) == 1, maps",
    ])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def _persplat_cases():
    g = load_golden("persplat.npz")
    cl, lg = load_golden("clouds.npz"), load_golden("legacy.npz")
    streams = {f"d{d}": cl[f"d{d}_stream_from0"] for d in range(4)}
    streams.update(v2=lg["v2_stream"], v1=lg["v1_stream"], fb0=lg["fb0_stream"], fb8=lg["fb8_stream"],
                   fb23=lg["fb23_stream"])
    return g, streams


def test_per_splat_at_and_unpack_match_the_reference(spz):
    """PackedGaussians::at(i) and ::unpack(i, converter) (load-spz.cc:383-463) of the C++ drop-in layer:
    the 65 packed bytes and the 59 floats equal what the reference returned (tests/golden/persplat.npz:
    v3 SH0..3 with edge values, v2 first-three, v1 float16, fractionalBits 0/8/23; six from->to
    converters), bit for bit.  Each unpack is a one-point decode on the GPU."""
    g, streams = _persplat_cases()
    for name, s in streams.items():
        idx = g[f"{name}_indices"]
        raw = s.tobytes()
        for frm, to in g["pairs"]:
            want_f = g[f"{name}_floats_{frm}_{to}"]
            step = 1 if (frm, to) == (4, 6) else 7        # every index for one converter, a sample for the others
            for k in range(0, idx.size, step):
                b, f = spz._packed_unpack(raw, int(idx[k]), spz.CoordinateSystem(int(frm)), spz.CoordinateSystem(int(to)),
                                          False)
                assert bytes(b) == g[f"{name}_bytes"][k].tobytes(), (name, int(idx[k]))
                assert_bits_equal(f, want_f[k], f"{name} i={int(idx[k])} {frm}->{to}")
    assert spz._packed_unpack(streams["d3"].tobytes(), 10**6, spz.RUB, spz.RUB, False) is None


def test_unpack_indices_matches_per_splat_goldens(spz):
    """unpackIndices (one gather launch over the packed cloud) returns, in cloud-array layout, the same
    floats the reference's per-splat unpack gave for those indices (converter RUB -> to)."""
    g, streams = _persplat_cases()
    for name, s in streams.items():
        idx = g[f"{name}_indices"]
        for to in (6, 1):
            o = spz.UnpackOptions()
            o.to_coord = spz.CoordinateSystem(to)
            c = spz._unpack_indices(s.tobytes(), [int(i) for i in idx], o, False)
            f = g[f"{name}_floats_4_{to}"]
            assert c.num_points == idx.size
            d = c.sh_degree
            shd = {0: 0, 1: 3, 2: 8, 3: 15}[d]
            assert_bits_equal(c.positions, f[:, 0:3].reshape(-1), f"{name} positions")
            assert_bits_equal(c.rotations, f[:, 3:7].reshape(-1), f"{name} rotations")
            assert_bits_equal(c.scales, f[:, 7:10].reshape(-1), f"{name} scales")
            assert_bits_equal(c.colors, f[:, 10:13].reshape(-1), f"{name} colors")
            assert_bits_equal(c.alphas, f[:, 13], f"{name} alphas")
            sh = np.stack([f[:, 14:14 + shd], f[:, 29:29 + shd], f[:, 44:44 + shd]], axis=2)   # [n][coeff][rgb]
            assert_bits_equal(c.sh, sh.reshape(-1), f"{name} sh")
    # repeated and out-of-order indices, gzip container, empty list
    o = spz.UnpackOptions()
    big = streams["d2"].tobytes()
    gz = spz._compress_gzipped(big)
    a = spz._unpack_indices(gz, [5, 5, 0, 511, 5], o)
    assert a.num_points == 5
    np.testing.assert_array_equal(a.positions[0:3], a.positions[3:6])
    np.testing.assert_array_equal(a.positions[0:3], a.positions[12:15])
    assert spz._unpack_indices(gz, [], o).num_points == 0


def test_median_volume_matches_the_reference(spz):
    """GaussianCloud.median_volume(): the device radix selection of the middle scale sum gives the
    reference's value to the bit (tests/golden/median.npz), plus the literals of load_spz_test.py:403-441."""
    import math
    g = load_golden("median.npz")
    for name in sorted(k[:-7] for k in g.files if k.endswith("_scales")):
        sc = g[f"{name}_scales"]
        c = spz.GaussianCloud()
        c.positions = np.zeros(sc.size, np.float32)
        c.scales = sc
        got = np.float32(c.median_volume())
        assert got.tobytes() == np.float32(g[f"{name}_volume"]).tobytes(), (name, got, g[f"{name}_volume"])
    c = spz.GaussianCloud()
    c.positions = np.zeros(9, np.float32)
    c.scales = np.array([-1, -1, -1, 0, 0, 0, 1, 1, 1], np.float32)
    assert abs(c.median_volume() - 4.0 / 3.0 * math.pi) < 1e-5
    c.positions = np.zeros(15, np.float32)
    c.scales = np.repeat(np.array([1, -2, 0, 2, -1], np.float32), 3)      # unsorted on purpose
    assert abs(c.median_volume() - 4.0 / 3.0 * math.pi) < 1e-5
    c.positions = np.zeros(12, np.float32)
    c.scales = np.repeat(np.array([0.5, -1, 0.25, -3], np.float32), 3)    # sums -9 -3 0.75 1.5 -> rank 2
    want = 4.0 / 3.0 * math.pi * math.exp(np.float32(0.75))
    assert abs(c.median_volume() - want) < 1e-4 * want


def test_median_scale_sum_device_entry_point_10m(cuda):
    """spz_amd_median_scale_sum_device on device-resident scales: 10 M points equal numpy's order statistic
    of the f32 sums, and the call is asynchronous on the given stream."""
    import torch
    from spz_amd import abi
    L = abi.load_library()
    n = 10_000_001
    gen = torch.Generator(device=cuda).manual_seed(5)
    sc = torch.empty(3 * n, dtype=torch.float32, device=cuda).uniform_(-8.0, 0.0, generator=gen)
    ws = torch.empty(abi.MEDIAN_WORKSPACE_BYTES, dtype=torch.uint8, device=cuda)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rc = L.spz_amd_median_scale_sum_device(sc.data_ptr(), n, ws.data_ptr(), out.data_ptr(), C.c_void_p(s.cuda_stream))
    assert rc == abi.OK
    s.synchronize()
    v = sc.view(n, 3)
    sums = (v[:, 0] + v[:, 1]) + v[:, 2]
    want = torch.sort(sums).values[n // 2]
    assert out.view(torch.int32).item() == want.view(torch.int32).item()
    small = sc[: 3 * 4097].cpu().numpy().reshape(-1, 3)
    rc = L.spz_amd_median_scale_sum_device(sc.data_ptr(), 4097, ws.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    want = np.sort((small[:, 0] + small[:, 1]) + small[:, 2])[4097 // 2]
    assert rc == abi.OK and np.float32(out.item()).tobytes() == np.float32(want).tobytes()


def test_whole_file_of_a_large_cloud_equals_the_reference_file(spz, reference_digests):
    """saveSpz of a 120 k-point SH3 cloud (7.8 MB stream: the GPU pack, then the multi-threaded exact gzip
    writer) is the reference's file byte for byte (the reference build's own saveSpz on the same arrays),
    and loadSpz of the reference's file (large enough for the parallel inflater on a many-core host) gives
    the reference's floats (both recorded, tests/golden/reference_digests.json)."""
    from conftest import digest, digest_cloud
    from spz_amd.synth import make_cloud_numpy
    ref = reference_digests
    n, deg = 120_000, 3
    c = make_cloud_numpy(n, deg, 77)
    assert digest_cloud(c) == ref["whole_file/input"], "the input generator changed"
    g = spz.GaussianCloud()
    g.sh_degree = deg
    g.antialiased = True
    for k in FIELDS:
        setattr(g, k, c[k])
    o = spz.PackOptions()
    o.from_coord = spz.RDF
    want = spz._save_spz_bytes(g, o)
    assert digest(want) == ref["whole_file/save"], ".spz bytes differ from the reference's saveSpz"
    # the same with the writer's opt-in checks switched on: SPZ_AMD_GZIP_VERIFY=1 inflates the finished member
    # and compares it with the stream, =2 also runs zlib over the whole stream and compares the two members
    for level in ("1", "2"):
        os.environ["SPZ_AMD_GZIP_VERIFY"] = level
        try:
            assert spz._save_spz_bytes(g, o) == want, f"SPZ_AMD_GZIP_VERIFY={level}"
        finally:
            del os.environ["SPZ_AMD_GZIP_VERIFY"]
    u = spz.UnpackOptions()
    u.to_coord = spz.LUF
    back = spz._load_spz_bytes(want, u)                # want is the reference's file (equal digests)
    assert back.num_points == ref["whole_file/load_to7/num_points"] == n and back.antialiased is True
    for k in FIELDS:
        assert digest(getattr(back, k)) == ref[f"whole_file/load_to7/{k}"], k


def test_file_name_overloads_of_a_file_above_16_mib(spz, tmp_path):
    """saveSpz(cloud, options, path) / loadSpz(path) of a 700 k-point SH3 cloud (a 28 MB file: above the size from which
    the file is read in pieces by several threads into a buffer that was never zero-filled, load-spz.cc:652-668 being one
    ifstream): the file is the vector overload's bytes, loading it by name gives what loading those bytes gives, and
    a directory as the target fails as the reference's ofstream does."""
    from spz_amd.synth import make_cloud_numpy
    n, deg = 700_000, 3
    c = make_cloud_numpy(n, deg, 78)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    o = spz.PackOptions()
    o.from_coord = spz.RUB
    want = spz._save_spz_bytes(g, o)
    assert len(want) > (16 << 20)
    path = str(tmp_path / "big.spz")
    with open(path, "wb") as f:
        f.write(b"x" * (len(want) + 12345))   # an older, longer file at that name: truncated, not overwritten in place
    assert spz.save_spz(g, o, path) is True
    with open(path, "rb") as f:
        assert f.read() == want
    u = spz.UnpackOptions()
    u.to_coord = spz.RDF
    a, b = spz.load_spz(path, u), spz._load_spz_bytes(want, u)
    assert a.num_points == n
    for k in FIELDS:
        assert_bits_equal(getattr(a, k), getattr(b, k), k)
    assert spz.save_spz(g, o, str(tmp_path)) is False
