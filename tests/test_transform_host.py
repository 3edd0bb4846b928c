"""spz.transform_spz / spz::transformSpz / spz_transform (DESIGN "Transform") without a GPU: the parameter block of
spz_amd_transform_params (orthogonal band matrices, exact signed permutations for axis-aligned turns, the rotated sh
function equal to the original one at the rotated direction, coord conjugation), the argument checks, which must raise
before any device work, the CLI's usage line, and a numpy float32 restatement of the per-point arithmetic.  The expected
file of every GPU test is zlib's level-6 gzip of Oracle.pack(T(Oracle.unpack(stream))) with T this restatement fed the
library's own parameter block (tests/test_gpu_transform.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}
BANDS = ((0, 3, "d1"), (3, 5, "d2"), (8, 7, "d3"))   # first coefficient, size, block field
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]


def params(rotation=None, translation=None, scale=1.0, coord=0):
    from spz_amd import abi
    return abi.transform_params(rotation, translation, scale, coord)


def block(xf):
    """The parameter block as float32 numpy arrays."""
    f = lambda v, *shape: np.array(v[:], np.float32).reshape(shape)  # noqa: E731
    return dict(m=f(xf.m, 3, 3), t=f(xf.t, 3), ln_s=np.float32(xf.ln_s), q=f(xf.q, 4), d1=f(xf.d1, 3, 3),
                d2=f(xf.d2, 5, 5), d3=f(xf.d3, 7, 7), pos=bool(xf.apply_positions), scl=bool(xf.apply_scales),
                rot=bool(xf.apply_rotation))


def sh_basis(d):
    """The 3DGS real-SH basis, bands 1..3, at unit vectors d (..., 3) -> (..., 15), float64."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([-C1 * y, C1 * z, -C1 * x,
                     C2[0] * x * y, C2[1] * y * z, C2[2] * (2 * zz - xx - yy), C2[3] * x * z, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * x * y * z, C3[2] * y * (4 * zz - xx - yy),
                     C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
                     C3[6] * x * (xx - 3 * yy)], axis=-1)


def quat_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def flip_sh(fx, fy, fz):
    """coordinateConverter's flipSh for the axis flips (fx, fy, fz) (1 = negated), as +-1 signs."""
    x, y, z = fx, fy, fz
    bits = [y, z, x, x ^ y, y ^ z, 0, x ^ z, 0, y, x ^ y ^ z, y, z, x, z, x]
    return np.array([-1.0 if b else 1.0 for b in bits], np.float32)


# ---- the restatement -----------------------------------------------------------------------------------------------
def apply_transform(cloud, xf, sh_degree):
    """T on a cloud of float32 arrays: every product and sum rounded on its own (numpy float32 element-wise ops)."""
    b = block(xf)
    out = {k: np.array(v, np.float32, copy=True) for k, v in cloud.items() if isinstance(v, np.ndarray)}
    with np.errstate(all="ignore"):
        if b["pos"]:
            p = out["positions"].reshape(-1, 3)
            m, t = b["m"], b["t"]
            out["positions"] = np.stack([((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + t[i]
                                         for i in range(3)], axis=1).reshape(-1)
        if b["scl"]:
            out["scales"] = out["scales"] + b["ln_s"]
        if b["rot"]:
            ax, ay, az, aw = b["q"]
            r = out["rotations"].reshape(-1, 4)
            bx, by, bz, bw = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
            out["rotations"] = np.stack([
                ((aw * bx + ax * bw) + ay * bz) - az * by,
                ((aw * by - ax * bz) + ay * bw) + az * bx,
                ((aw * bz + ax * by) - ay * bx) + az * bw,
                ((aw * bw - ax * bx) - ay * by) - az * bz], axis=1).reshape(-1)
            dim = SH_DIM[sh_degree]
            if dim:
                c = out["sh"].reshape(-1, dim, 3)
                new = np.empty_like(c)
                for k0, size, name in BANDS:
                    if k0 >= dim:
                        break
                    d = b[name]
                    for m_ in range(size):
                        acc = d[0, m_] * c[:, k0, :]
                        for k in range(1, size):
                            acc = acc + d[k, m_] * c[:, k0 + k, :]
                        new[:, k0 + m_, :] = acc
                out["sh"] = new.reshape(-1)
    return out


def round_half_away(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        t = np.trunc(x)
        return np.where(np.abs(x - t) >= np.float32(0.5), t + np.copysign(np.float32(1), x), t).astype(np.float32)


def encode_positions(p, fb):
    """24-bit positions at fb fractional bits (round half away, wrap to 24 bits) and the out-of-range count (points with
    a coordinate whose rounded value does not fit 24 bits, NaN included)."""
    with np.errstate(all="ignore"):
        r = round_half_away(np.asarray(p, np.float32) * np.float32(2.0 ** fb))
    ok = (r >= -8388608.0) & (r <= 8388607.0)
    bad = int(np.count_nonzero(~np.all(ok.reshape(-1, 3), axis=1)))
    # static_cast<int32_t> as x86 executes it: NaN and values outside int32 give 0x80000000, whose low 24 bits are 0
    v = np.where((r >= -2.0 ** 31) & (r < 2.0 ** 31), r, 0).astype(np.int64) & 0xFFFFFF
    b = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).reshape(-1)
    return b, bad


def expected_stream(oracle, raw, xf, fb=12):
    """(stream, out-of-range count) the transform of `raw` must produce: Oracle.pack(T(Oracle.unpack(raw))) as v3,
    positions at fb."""
    rc, c = oracle.unpack(np.frombuffer(bytes(raw), np.uint8))
    assert rc == 0
    n, deg = c["num_points"], c["sh_degree"]
    t = apply_transform(c, xf, deg)
    s = oracle.pack(t, n, deg, c["antialiased"], 0, 3).copy()
    pos, bad = encode_positions(t["positions"], fb)
    s[16:16 + 9 * n] = pos
    s[13] = fb
    return s.tobytes(), bad


def golden_streams():
    cl, lg = load_golden("clouds.npz"), load_golden("legacy.npz")
    out = {f"v3_sh{d}": cl[f"d{d}_stream_from0"].tobytes() for d in range(4)}
    out.update(v2=lg["v2_stream"].tobytes(), v1=lg["v1_stream"].tobytes(),
               fb0=lg["fb0_stream"].tobytes(), fb8=lg["fb8_stream"].tobytes(), fb23=lg["fb23_stream"].tobytes())
    return out


def random_rotations(k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(4) for _ in range(k)]


# ---- the parameter block --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", random_rotations(6, 1) + [[1, 0, 0, 0], [0, 0, 0.5, 0.5], [0.1, -0.2, 0.3, -0.9]])
def test_block_is_orthogonal_in_f32(q):
    b = block(params(q, [1, 2, 3], 2.5))
    r = b["m"].astype(np.float64) / 2.5
    assert np.allclose(r @ r.T, np.eye(3), atol=2e-7) and np.linalg.det(r) > 0
    assert np.allclose(r, quat_matrix(q), atol=2e-7)
    for name, size in (("d1", 3), ("d2", 5), ("d3", 7)):
        d = b[name].astype(np.float64)
        assert np.allclose(d @ d.T, np.eye(size), atol=1e-6), name
    assert b["ln_s"] == np.float32(np.log(2.5))
    assert np.isclose(np.linalg.norm(b["q"].astype(np.float64)), 1.0, atol=1e-7) and b["q"][3] >= 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_turns_are_exactly_flip_sh(axis):
    q = [0.0, 0.0, 0.0, 0.0]
    q[axis] = 1.0
    b = block(params(q))
    flips = [1, 1, 1]
    flips[axis] = 0          # a half turn about an axis negates the other two
    signs = flip_sh(*flips)
    want_m = np.diag([-1.0 if f else 1.0 for f in flips]).astype(np.float32)
    assert np.array_equal(b["m"], want_m)
    for k0, size, name in BANDS:
        assert np.array_equal(b[name], np.diag(signs[k0:k0 + size])), name


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_quarter_turns_are_signed_permutations(axis, sign):
    q = [0.0, 0.0, 0.0, np.sqrt(0.5)]
    q[axis] = sign * np.sqrt(0.5)
    b = block(params(q))
    # band 1 is the vector itself; the higher bands of the real basis are permuted only by turns about z (about x or y
    # the m = 0 functions mix with the others)
    for name in ("m", "d1", "d2", "d3") if axis == 2 else ("m", "d1"):
        d = b[name]
        assert set(np.unique(d).tolist()) <= {-1.0, 0.0, 1.0}, name
        assert np.all(np.count_nonzero(d, axis=0) == 1) and np.all(np.count_nonzero(d, axis=1) == 1), name


@pytest.mark.parametrize("q", random_rotations(5, 2))
def test_rotated_sh_function_is_the_original_at_the_rotated_direction(q):
    """f'(d) = f(R^T d) with c' = D^T c, in float64 with the block's (f32) matrices."""
    b = block(params(q))
    r = b["m"].astype(np.float64)
    rng = np.random.default_rng(7)
    c = rng.standard_normal(15)
    cp = np.empty(15)
    for k0, size, name in BANDS:
        cp[k0:k0 + size] = b[name].astype(np.float64).T @ c[k0:k0 + size]
    d = rng.standard_normal((64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.allclose(sh_basis(d) @ cp, sh_basis(d @ r) @ c, atol=2e-6)   # rows of d @ r are R^T d


@pytest.mark.parametrize("coord", [1, 2, 3, 5, 6, 7, 8])
def test_coord_is_conjugated_into_rub(coord):
    from spz_amd import abi
    q, t = [0.3, -0.5, 0.2, 0.7], [1.5, -2.0, 0.25]
    a, b = block(params(q, t, 1.5, abi.RUB)), block(params(q, t, 1.5, coord))
    # RUB = 4 = bits (x right, y up, z back); flip axis a where the bit differs
    f = np.array([-1.0 if ((coord - 1) >> k & 1) != ((4 - 1) >> k & 1) else 1.0 for k in range(3)], np.float32)
    assert np.array_equal(b["m"], (f[:, None] * a["m"] * f[None, :]).astype(np.float32))
    assert np.array_equal(b["t"], f * a["t"])
    assert np.array_equal(block(params(q, t, 1.5, 0))["m"], a["m"])  # UNSPECIFIED: no flips


def test_identity_block_runs_nothing():
    b = block(params())
    assert not (b["pos"] or b["scl"] or b["rot"])
    assert np.array_equal(b["q"], [0, 0, 0, 1]) and np.array_equal(b["m"], np.eye(3))
    assert not block(params([0, 0, 0, -3.0]))["rot"]               # -identity, any length
    b = block(params(translation=[0, 0, 1]))
    assert b["pos"] and not b["rot"] and not b["scl"]
    b = block(params(scale=2.0))
    assert b["pos"] and b["scl"] and not b["rot"]


@pytest.mark.parametrize("kw", [
    dict(rotation=[0, 0, 0, 0]), dict(rotation=[np.nan, 0, 0, 1]), dict(rotation=[np.inf, 0, 0, 1]),
    dict(translation=[0, np.inf, 0]), dict(translation=[np.nan, 0, 0]), dict(translation=[1e39, 0, 0]),
    dict(scale=0.0), dict(scale=-1.0), dict(scale=np.nan), dict(scale=np.inf), dict(scale=1e39), dict(scale=1e-50),
    dict(coord=9), dict(coord=-1),
], ids=lambda kw: ",".join(kw))
def test_c_abi_rejects_bad_parameters(kw):
    import ctypes as C

    from spz_amd import abi
    L = abi.load_library()
    q = (C.c_double * 4)(*kw.get("rotation", [0, 0, 0, 1]))
    t = (C.c_double * 3)(*kw.get("translation", [0, 0, 0]))
    out = abi.Transform()
    assert L.spz_amd_transform_params(q, t, float(kw.get("scale", 1.0)), int(kw.get("coord", 0)), C.byref(out)) == abi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        params(**kw)


def test_c_abi_null_means_identity():
    from spz_amd import abi
    L = abi.load_library()
    out = abi.Transform()
    assert L.spz_amd_transform_params(None, None, 1.0, 0, out) == abi.OK
    assert not (out.apply_positions or out.apply_scales or out.apply_rotation)
    assert L.spz_amd_transform_params(None, None, 1.0, 0, None) == abi.ERR_INVALID_ARG


# ---- argument checks: ValueError before any device work (no device here) -----------------------------------------
@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


@pytest.fixture()
def some_file(tmp_path):
    p = tmp_path / "in.spz"
    p.write_bytes(b"not read: the arguments are checked first")
    return str(p)


BAD = [
    dict(rotation=[0, 0, 0, 0]), dict(rotation=[0, 0, 1]), dict(rotation=[0, 0, 0, float("nan")]), dict(rotation="abcd"),
    dict(rotation=[[0, 0], [0, 1]]), dict(translation=[0, 0]), dict(translation=[0, float("inf"), 0]),
    dict(scale=0), dict(scale=-2.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale="1"), dict(scale=True),
    dict(scale=1e39), dict(fractional_bits=25), dict(fractional_bits=-1), dict(fractional_bits=12.0),
    dict(fractional_bits=True),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}" for k in kw))
def test_bad_arguments_raise_value_error_before_device_work(spz, some_file, tmp_path, kw):
    with pytest.raises(ValueError):
        spz.transform_spz(some_file, str(tmp_path / "out.spz"), **kw)
    assert not (tmp_path / "out.spz").exists()
    if "fractional_bits" not in kw:
        g = spz.GaussianCloud()
        with pytest.raises(ValueError):
            spz.transform_cloud(g, **kw)


def test_device_transform_checks_its_arguments():
    torch = pytest.importorskip("torch")
    from spz_amd import device as D
    hdr = D.make_header(10, 2)
    st = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        D.transform_packed(st, hdr, rotation=[0, 0, 0, 0])
    with pytest.raises(ValueError):
        D.transform_packed(st, hdr, fractional_bits=30)
    with pytest.raises(ValueError):
        D.transform_packed(st, hdr, scale=-1.0)
    with pytest.raises(ValueError):
        D.transform({"positions": torch.zeros(3)}, 1, 0, scale=float("nan"))
    with pytest.raises(ValueError):
        D.transform({"positions": torch.zeros(3)}, 1, 0, translation=[1, 2, 3])   # not a CUDA tensor


# ---- the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["spz_transform"], ["spz_transform", "in.spz"], ["spz_tool", "spz_transform"], ["spz_tool", "spz_transform", "in.spz"],
    ["spz_transform", "a.spz", "b.spz", "--rotate", "0", "0", "1"], ["spz_transform", "a.spz", "b.spz", "--scale"],
    ["spz_transform", "a.spz", "b.spz", "--scale", "x"], ["spz_transform", "a.spz", "b.spz", "--translate", "1", "2"],
    ["spz_transform", "a.spz", "b.spz", "--coord", "XYZ"], ["spz_transform", "a.spz", "b.spz", "--fractional-bits", "25"],
    ["spz_transform", "a.spz", "b.spz", "--bogus"],
    ["spz_transform", "a.spz", "b.spz", "--fractional-bits", ""], ["spz_transform", "a.spz", "b.spz", "--fractional-bits", "+2"],
    ["spz_transform", "a.spz", "b.spz", "--fractional-bits", " 2"], ["spz_transform", "a.spz", "b.spz", "--fractional-bits", "-0"],
    ["spz_transform", "a.spz", "b.spz", "--scale", "2", "--scale", "2"],
    ["spz_transform", "a.spz", "b.spz", "--coord", "RUB", "--coord", "RDF"],
    ["spz_transform", "-a.spz", "b.spz"], ["spz_transform", "a.spz", "-b.spz"],
])
def test_cli_usage(argv, tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith("Usage: spz_transform <input.spz> <output.spz>")
    assert not (tmp_path / "b.spz").exists()


def test_cli_bad_transform_exits_1_without_output(tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_transform")
    (tmp_path / "a.spz").write_bytes(b"never read")
    r = subprocess.run([exe, "a.spz", "b.spz", "--scale", "0"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1 and "[SPZ ERROR] transformSpz" in r.stdout
    assert not (tmp_path / "b.spz").exists()


# ---- the restatement against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(golden_streams()))
def test_restated_identity_is_pack_of_unpack(oracle, name):
    raw = golden_streams()[name]
    rc, c = oracle.unpack(np.frombuffer(raw, np.uint8))
    want = oracle.pack(c, c["num_points"], c["sh_degree"], c["antialiased"], 0, 3).tobytes()
    got, bad = expected_stream(oracle, raw, params(), 12)
    assert got == want   # out-of-range positions wrap as saveSpz's do; transformSpz refuses them instead
    # fb0 holds positions beyond +-2048, v1 infinities and NaNs: those do not fit 24 bits at 12 fractional bits
    assert (bad > 0) == (name in ("fb0", "v1"))


@pytest.mark.parametrize("q", random_rotations(3, 3) + [None])
def test_restated_position_encoder_is_the_oracles_at_12_bits(oracle, q):
    from spz_amd.synth import make_cloud_numpy
    n = 1000
    c = make_cloud_numpy(n, 1, 31)
    c["positions"][:6] = [0.5 / 4096, -0.5 / 4096, 1.5 / 4096, -2.5 / 4096, 0.0, -0.0]
    t = apply_transform(c, params(q, [0.25, -3.0, 7.0], 1.75), 1)
    want = oracle.pack(t, n, 1, False, 0, 3)[16:16 + 9 * n]
    got, bad = encode_positions(t["positions"], 12)
    assert bad == 0 and np.array_equal(got, want)
    assert encode_positions(np.float32([4096.0, 0, 0]), 11)[1] == 1 and encode_positions(np.float32([np.nan, 0, 0]), 12)[1] == 1
