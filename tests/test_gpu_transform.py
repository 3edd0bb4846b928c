"""spz.transform_spz / transform_cloud / spz_amd.device.transform + transform_packed / the spz_transform CLI (DESIGN
"Transform") on the GPU, each against the numpy restatement of tests/test_transform_host.py: the cloud kernel bit for
bit, every file byte for byte (zlib's level-6 gzip of Oracle.pack(T(Oracle.unpack(stream)))), the fused packed kernel
equal to decode -> transform -> encode at 10 M SH3 points, a half turn about X equal to convert_coordinates(RUB, RDF),
the identity equal to save_spz(load_spz(file)), and the refusal of positions that do not fit 24 bits."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import FIELDS, ROOT
from test_transform_host import apply_transform, expected_stream, golden_streams, params, quat_matrix, random_rotations

pytestmark = pytest.mark.gpu

TRANSFORMS = [
    dict(),
    dict(rotation=[1, 0, 0, 0]),
    dict(rotation=[0, 0, np.sqrt(0.5), np.sqrt(0.5)], translation=[0.5, -1.25, 2.0]),
    dict(rotation=list(random_rotations(1, 11)[0]), translation=[-3.0, 0.75, 1.5], scale=1.7),
    dict(rotation=list(random_rotations(1, 12)[0]), scale=0.35),
    dict(translation=[1.0, 2.0, -0.5]),
]


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def assert_floats_equal(got, want, what):
    """Bit for bit, except that any NaN equals any NaN."""
    g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert g.shape == w.shape, what
    gn, wn = np.isnan(g), np.isnan(w)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    gb, wb = g.view(np.uint32)[~gn], w.view(np.uint32)[~wn]
    if not np.array_equal(gb, wb):
        i = int(np.nonzero(gb != wb)[0][0])
        raise AssertionError(f"{what}: {(gb != wb).sum()} floats differ; first got {g[~gn][i]!r} want {w[~wn][i]!r}")


def specials(c, n):
    """+-0, infinities and NaNs in the first points of every field."""
    vals = np.float32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e-30])
    for k in ("positions", "scales", "rotations", "sh"):
        a = c[k]
        m = min(a.size, len(vals) * 3)
        if m:
            a[:m] = np.resize(vals, m)
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 4099])
def test_cloud_kernel_bit_for_bit(spz, n):
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_numpy
    for deg in range(4):
        c = specials(make_cloud_numpy(n, deg, 300 + n + deg), n) if n > 3 else make_cloud_numpy(n, deg, 300 + n + deg)
        for kw in TRANSFORMS:
            want = apply_transform(c, params(**kw), deg)
            t = D.to_device(c, torch.device("cuda:0"))
            D.transform(t, n, deg, **kw)
            torch.cuda.synchronize()
            for k in FIELDS:
                assert_floats_equal(t[k].cpu().numpy(), want[k], f"n={n} sh{deg} {kw} {k}")
    # the host form (spz.transform_cloud) gives the same floats
    g = spz.GaussianCloud()
    g.sh_degree = 3
    c = make_cloud_numpy(n, 3, 77)
    for k in FIELDS:
        setattr(g, k, c[k])
    spz.transform_cloud(g, **TRANSFORMS[3])
    want = apply_transform(c, params(**TRANSFORMS[3]), 3)
    for k in FIELDS:
        assert_floats_equal(np.asarray(getattr(g, k)), want[k], f"transform_cloud n={n} {k}")


def synth_stream(oracle, n=4099, deg=3, seed=5):
    """A stream of spz_amd.synth points (positions within +-10, far from the 24-bit limits)."""
    from spz_amd.synth import make_cloud_numpy
    return oracle.pack(make_cloud_numpy(n, deg, seed), n, deg, False, 0, 3).tobytes()


def run_file(spz, tmp_path, raw, **kw):
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    if dst.exists():
        dst.unlink()
    spz.transform_spz(str(src), str(dst), **kw)
    return dst.read_bytes()


def test_golden_streams_byte_for_byte(spz, tmp_path, oracle):
    from spz_amd import abi
    for name, raw in golden_streams().items():
        for i, kw in enumerate(TRANSFORMS):
            for coord in (abi.UNSPECIFIED, abi.RUB, abi.RDF, abi.LUF) if i in (2, 3) else (abi.UNSPECIFIED,):
                for fb in (8, 12, 16):
                    full = dict(kw, coord=spz.CoordinateSystem(coord), fractional_bits=fb)
                    want, bad = expected_stream(oracle, raw, params(**dict(kw, coord=coord)), fb)
                    what = f"{name} {kw} coord {coord} fb {fb}"
                    if bad:
                        with pytest.raises(ValueError):
                            run_file(spz, tmp_path, raw, **full)
                        assert not (tmp_path / "out.spz").exists(), what
                        continue
                    f = run_file(spz, tmp_path, raw, **full)
                    assert zlib.decompress(f, 31) == want, what
                    assert f == gz(want), f"{what}: the file is not zlib's member of the stream"


def test_device_packed_form_on_a_side_stream(spz, cuda, oracle):
    import torch
    from spz_amd import abi, device as D
    raw = golden_streams()["v2"]
    hdr = abi.peek_header(raw)[1]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
        out, bad = D.transform_packed(st, hdr, fractional_bits=10, stream=side, **TRANSFORMS[3])
    side.synchronize()
    want, nbad = expected_stream(oracle, raw, params(**TRANSFORMS[3]), 10)
    assert out.cpu().numpy().tobytes() == want and int(bad.item()) == nbad == 0


@pytest.fixture(scope="module")
def big(spz, tmp_path_factory):
    """10 M SH3 points from spz_amd.synth, written by save_spz."""
    from spz_amd.synth import make_cloud_numpy
    n, deg = 10_000_000, 3
    c = make_cloud_numpy(n, deg, 2025)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    del c
    path = str(tmp_path_factory.mktemp("big") / "big.spz")
    assert spz.save_spz(g, spz.PackOptions(), path)
    return path, g, n


def test_ten_million_fused_equals_unfused(spz, big, cuda):
    import torch
    from spz_amd import device as D
    path, g, n = big
    raw = spz._pack_to_stream(g, spz.PackOptions())
    hdr = D.make_header(n, 3)
    st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    kw = TRANSFORMS[3]
    fused, bad = D.transform_packed(st, hdr, **kw)
    cloud = D.decode(st, hdr)
    D.transform(cloud, n, 3, **kw)
    unfused = D.encode(cloud, n, 3)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert torch.equal(fused, unfused)


def test_ten_million_identity_is_save_of_load(spz, big, tmp_path):
    path, g, n = big
    out = str(tmp_path / "id.spz")
    spz.transform_spz(path, out)
    with open(out, "rb") as f:
        got = f.read()
    assert got == spz._save_spz_bytes(spz.load_spz(path, spz.UnpackOptions()), spz.PackOptions())


def test_half_turn_about_x_is_convert_coordinates(spz, cuda):
    import torch
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_numpy
    n = 4099
    c = make_cloud_numpy(n, 3, 9)
    a, b = D.to_device(c, cuda), D.to_device(c, cuda)
    D.transform(a, n, 3, rotation=[1, 0, 0, 0])
    D.convert_coordinates(b, n, 3, abi.RUB, abi.RDF)
    torch.cuda.synchronize()
    for k in ("positions", "sh", "scales", "alphas", "colors"):
        assert torch.equal(a[k], b[k]), k

    def covariance(cl):
        q = cl["rotations"].cpu().numpy().astype(np.float64).reshape(-1, 4)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        x, y, z, w = q.T
        r = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                      2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                      2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        s = np.exp(cl["scales"].cpu().numpy().astype(np.float64).reshape(-1, 3))
        return np.einsum("nij,nj,nkj->nik", r, s * s, r)

    assert np.allclose(covariance(a), covariance(b), rtol=1e-5, atol=1e-12)


def test_out_of_range_is_refused_and_fewer_bits_succeed(spz, tmp_path, capfd, oracle):
    raw = synth_stream(oracle, deg=1)
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    _, bad12 = expected_stream(oracle, raw, params(scale=1e4), 12)
    assert bad12 > 0
    with pytest.raises(ValueError):
        spz.transform_spz(str(src), str(dst), scale=1e4)
    assert f"{bad12} of " in capfd.readouterr().out
    assert not dst.exists()
    spz.transform_spz(str(src), str(dst), scale=1e4, fractional_bits=4)
    want, bad = expected_stream(oracle, raw, params(scale=1e4), 4)
    assert bad == 0 and zlib.decompress(dst.read_bytes(), 31) == want


def test_every_surface_writes_the_same_bytes(spz, tmp_path, cuda, oracle):
    import torch
    from spz_amd import abi, device as D
    raw = synth_stream(oracle)
    src = tmp_path / "in.spz"
    src.write_bytes(gz(raw))
    q, t, s = [0.2, -0.4, 0.1, 0.9], [1.0, -2.0, 0.5], 1.25
    spz.transform_spz(str(src), str(tmp_path / "py.spz"), rotation=q, translation=t, scale=s, coord=spz.RDF)
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_transform")
    r = subprocess.run([exe, str(src), str(tmp_path / "cli.spz"), "--rotate", *map(str, q), "--translate", *map(str, t),
                        "--scale", str(s), "--coord", "RDF"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    dev, _ = D.transform_packed(st, abi.peek_header(raw)[1], rotation=q, translation=t, scale=s, coord=abi.RDF)
    py = (tmp_path / "py.spz").read_bytes()
    assert py == (tmp_path / "cli.spz").read_bytes()
    assert py == gz(dev.cpu().numpy().tobytes())


def test_loose_round_trip(spz, tmp_path, oracle):
    """A transform followed by its inverse comes back within the quantisation steps."""
    raw = synth_stream(oracle, seed=6)
    q = np.array([0.3, -0.1, 0.5, 0.8])
    q /= np.linalg.norm(q)
    t, s = np.array([0.5, 1.0, -1.5]), 1.5
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    # p = s R p0 + t  ->  p0 = (1/s) R^T p - (1/s) R^T t
    ti = -(quat_matrix(qi) @ t) / s
    src, mid, back = tmp_path / "in.spz", tmp_path / "mid.spz", tmp_path / "back.spz"
    src.write_bytes(gz(raw))
    spz.transform_spz(str(src), str(mid), rotation=q, translation=t, scale=s)
    spz.transform_spz(str(mid), str(back), rotation=qi, translation=ti, scale=1.0 / s)
    rc, a = oracle.unpack(np.frombuffer(raw, np.uint8))
    rc, b = oracle.unpack(np.frombuffer(zlib.decompress(back.read_bytes(), 31), np.uint8))
    assert np.allclose(a["positions"], b["positions"], atol=3.0 / 4096)
    assert np.allclose(a["scales"], b["scales"], atol=2.0 / 16)
    assert np.array_equal(a["alphas"], b["alphas"]) and np.array_equal(a["colors"], b["colors"])
    qa, qb = a["rotations"].reshape(-1, 4), b["rotations"].reshape(-1, 4)
    assert np.all(np.abs(np.sum(qa * qb, axis=1)) > 0.99)
    assert np.allclose(a["sh"], b["sh"], atol=0.25)
    assert np.mean(np.abs(a["sh"] - b["sh"])) < 0.05
