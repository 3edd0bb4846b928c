"""spz.sort_spz / spz_sort / spz_amd_sort_open / spz_amd.device.morton_order + argsort + chunk_bounds (DESIGN §8 "sort")
on the GPU: every output is the numpy restatement of tests/test_sort_host.py byte for byte — the order is np.lexsort of
the 72-bit Morton key (or np.argsort(kind="stable") of the caller's keys), the stream is the filter's
expected_stream(raw, order), the file is zlib's level-6 gzip of it."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import FIELDS, ROOT
from test_filter_host import SH_DIM, expected_stream, golden_streams, parse_stream
from test_sort_host import PER, chunk_bounds, key_order, morton_order, sortable_goldens

pytestmark = pytest.mark.gpu

TILE = 2048  # points per radix tile (spz_sort.hip kSortTile)


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def reference():
    from oracle.pyoracle import REF_SO, Reference
    return Reference() if os.path.exists(REF_SO) else None


def run_sort(spz, tmp_path, raw, **kw):
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    if dst.exists():
        dst.unlink()
    order = spz.sort_spz(str(src), str(dst), **kw)
    return order, dst.read_bytes()


def on_device(raw):
    import torch
    from spz_amd import abi
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda"), abi.peek_header(raw)[1]


def with_positions(raw, fields):
    """`raw` with its stored position fields replaced by `fields` ((N, 3) 24-bit ints)."""
    s = bytearray(raw)
    f = np.asarray(fields, np.uint32).reshape(-1, 3)
    b = np.stack([(f >> s_) & 0xFF for s_ in (0, 8, 16)], axis=2).astype(np.uint8)   # (N, axis, byte)
    s[16:16 + 9 * f.shape[0]] = b.reshape(-1).tobytes()
    return bytes(s)


def test_golden_streams_both_directions(spz, tmp_path):
    ref = reference()
    for name, raw in sortable_goldens().items():
        h = parse_stream(raw)
        n, deg = h["num_points"], h["sh_degree"]
        for descending in (False, True):
            order, f = run_sort(spz, tmp_path, raw, descending=descending)
            want_order = morton_order(raw, descending)
            assert order.dtype == np.uint32 and np.array_equal(order, want_order), f"{name} {descending}: order"
            want = expected_stream(raw, want_order)
            assert zlib.decompress(f, 31) == want, f"{name} {descending}: stream"
            assert f == gz(want), f"{name} {descending}: the file is not zlib's member of the stream"
            if ref is not None:
                got = ref.load_spz(np.frombuffer(f, np.uint8), n, deg)
                full = ref.load_spz(np.frombuffer(gz(raw), np.uint8), n, deg)
                for k, w in PER.items():
                    assert np.array_equal(got[k].view(np.uint32),
                                          full[k].reshape(n, w)[order].reshape(-1).view(np.uint32)), f"{name} {k}"
                sh = full["sh"].reshape(n, SH_DIM[deg] * 3)[order].reshape(-1)
                assert np.array_equal(got["sh"].view(np.uint32), sh.view(np.uint32)), f"{name} sh"


def test_caller_keys_on_golden_streams(spz, tmp_path):
    """Keys work for every version (v1 included): the order is np.argsort(kind='stable'), NaN last."""
    rng = np.random.default_rng(4)
    for name, raw in golden_streams().items():
        n = parse_stream(raw)["num_points"]
        k = rng.choice(np.array([0.5, -0.0, 0.0, np.nan, np.inf, -np.inf, -2.0], np.float32), n)
        for descending in (False, True):
            order, f = run_sort(spz, tmp_path, raw, keys=k, descending=descending)
            want = key_order(k, descending)
            assert np.array_equal(order, want), f"{name} {descending}"
            assert zlib.decompress(f, 31) == expected_stream(raw, want)


def test_v1_and_wrong_key_count_are_refused(spz, tmp_path, capfd):
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(golden_streams()["v1"]))
    with pytest.raises(ValueError):
        spz.sort_spz(str(src), str(dst))
    assert "transformSpz with the identity" in capfd.readouterr().out
    assert not dst.exists()
    raw = sortable_goldens()["v3_sh2"]
    n = parse_stream(raw)["num_points"]
    src.write_bytes(gz(raw))
    for m in (n - 1, n + 1, 0):
        with pytest.raises(ValueError):
            spz.sort_spz(str(src), str(dst), keys=np.zeros(m, np.float32))
        assert not dst.exists()
    from spz_amd import device as D
    st, hdr = on_device(golden_streams()["v1"])
    with pytest.raises(ValueError):
        D.morton_order(st, hdr)
    with pytest.raises(ValueError):
        D.chunk_bounds(st, hdr)


def test_idempotent_and_filter_undoes_it(spz, tmp_path, oracle):
    from spz_amd.synth import make_cloud_clustered
    n = 3 * TILE + 77
    raw = oracle.pack(make_cloud_clustered(n, 3, 12, clusters=40), n, 3, True, 0).tobytes()
    src, once, twice, back = (tmp_path / s for s in ("in.spz", "once.spz", "twice.spz", "back.spz"))
    src.write_bytes(gz(raw))
    order = spz.sort_spz(str(src), str(once))
    order2 = spz.sort_spz(str(once), str(twice))
    assert twice.read_bytes() == once.read_bytes()
    assert np.array_equal(order2, np.arange(n))
    assert spz.filter_spz(str(once), str(back), indices=np.argsort(order).astype(np.uint32)) == n
    assert zlib.decompress(back.read_bytes(), 31) == raw


ODD_RUNS_N = 256 * TILE + 1   # 257 tiles for the 256 threads of the row scan: runs of two counts, the last owning thread
                              # holds one, half the block holds none


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, ODD_RUNS_N, (1 << 20) + 3, 10_000_000])
def test_device_argsort_equals_numpy(cuda, n):
    import torch
    from spz_amd import device as D
    if n == ODD_RUNS_N:
        tiles = -(-n // TILE)
        assert n == 524_289 and tiles % 2 == 1 and 256 < tiles < 2 * 256
    rng = np.random.default_rng(n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0], np.float32)
    cases = {"random": rng.standard_normal(n).astype(np.float32),
             "four": rng.choice(np.array([3.0, -1.0, 0.25, 7.0], np.float32), n)}
    if n <= (1 << 20) + 3:
        cases["special"] = rng.choice(special, n)
        cases["mixed"] = np.where(rng.random(n) < 0.2, rng.choice(special, n), rng.standard_normal(n)).astype(np.float32)
    for label, k in cases.items():
        kt = torch.from_numpy(k).to(cuda)
        for descending in (False, True):
            got = D.argsort(kt, descending=descending)
            torch.cuda.synchronize()
            assert got.dtype == torch.int32 and got.numel() == n
            assert np.array_equal(got.cpu().numpy(), key_order(k, descending)), f"n={n} {label} {descending}"


def morton_cases(n, seed):
    rng = np.random.default_rng(seed)
    return {
        "one_position": np.tile(np.array([[0x123456, 0xFEDCBA, 0x000001]], np.uint32), (n, 1)),
        "top_digit_only": (rng.integers(0, 4, (n, 3)) << 22).astype(np.uint32) | 0x155555,   # only key bits 64..71 vary
        "every_digit": rng.integers(0, 1 << 24, (n, 3)).astype(np.uint32),
        "extremes": rng.choice(np.array([0x800000, 0x7FFFFF, 0x000000, 0xFFFFFF, 0x800001], np.uint32), (n, 3)),
    }


@pytest.mark.parametrize("n", [1, 65, TILE + 1, 5 * TILE + 9])
def test_morton_edge_cases(spz, tmp_path, oracle, n):
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_numpy
    base = oracle.pack(make_cloud_numpy(n, 1, 30 + n), n, 1, False, 0).tobytes()
    for label, fields in morton_cases(n, n).items():
        raw = with_positions(base, fields)
        st, hdr = on_device(raw)
        for descending in (False, True):
            want = morton_order(raw, descending)
            if label == "one_position":
                assert np.array_equal(want, np.arange(n))
            got = D.morton_order(st, hdr, descending=descending)
            out = D.subset(st, hdr, got)
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), want), f"{label} n={n} {descending}"
            assert out.cpu().numpy().tobytes() == expected_stream(raw, want), f"{label} n={n} {descending}"
        order, f = run_sort(spz, tmp_path, raw)
        assert np.array_equal(order, morton_order(raw)) and zlib.decompress(f, 31) == expected_stream(raw, order)


@pytest.mark.parametrize("chunk", [1, 7, 256, 1000, 10_000])
def test_chunk_bounds_equal_numpy(cuda, oracle, chunk):
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_clustered
    n = 4 * TILE + 13
    for fb in (0, 12, 23):
        raw = oracle.pack(make_cloud_clustered(n, 0, fb, clusters=30), n, 0, False, 0).tobytes()
        raw = raw[:13] + bytes([fb]) + raw[14:]                 # the same integers read at another fractionalBits
        for stream in (raw, expected_stream(raw, morton_order(raw))):
            st, hdr = on_device(stream)
            got = D.chunk_bounds(st, hdr, chunk=chunk)
            torch.cuda.synchronize()
            want = chunk_bounds(stream, chunk)
            assert tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"fb={fb} chunk={chunk}"


@pytest.fixture(scope="module")
def big(spz, tmp_path_factory):
    """10 M SH3 points from spz_amd.synth, written by save_spz."""
    from spz_amd.synth import make_cloud_numpy
    n, deg = 10_000_000, 3
    c = make_cloud_numpy(n, deg, 77)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    del c
    po = spz.PackOptions()
    path = str(tmp_path_factory.mktemp("big") / "big.spz")
    assert spz.save_spz(g, po, path)
    raw = spz._pack_to_stream(g, po)
    order = morton_order(raw)
    return path, raw, order, expected_stream(raw, order)


def test_ten_million_every_surface_writes_the_same_bytes(spz, big, tmp_path):
    import torch
    from spz_amd import abi, device as D
    path, raw, want_order, want = big
    n = want_order.size
    # Python
    out = str(tmp_path / "py.spz")
    order = spz.sort_spz(path, out)
    assert np.array_equal(order, want_order)
    with open(out, "rb") as f:
        file_py = f.read()
    assert zlib.decompress(file_py, 31) == want
    # CLI
    cli = str(tmp_path / "cli.spz")
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_sort"), path, cli], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    with open(cli, "rb") as f:
        assert f.read() == file_py
    # device morton_order + subset
    st, hdr = on_device(raw)
    got = D.morton_order(st, hdr)
    sub = D.subset(st, hdr, got)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want_order)
    assert sub.cpu().numpy().tobytes() == want
    # C ABI host form on the same device stream
    L = abi.load_library()
    ctx, nbytes = C.c_void_p(), C.c_uint64()
    h_order = np.empty(n, np.uint32)
    ms = (C.c_float * 2)()
    rc = L.spz_amd_sort_open(st.data_ptr(), st.numel(), C.byref(hdr), None, 0, torch.cuda.current_device(),
                             C.byref(ctx), C.byref(nbytes), h_order.ctypes.data, ms)
    assert rc == abi.OK and nbytes.value == len(want)
    try:
        h_out = np.empty(nbytes.value, np.uint8)
        assert L.spz_amd_sort_fetch(ctx, h_out.ctypes.data) == abi.OK
        assert L.spz_amd_sort_device_data(ctx) is not None
    finally:
        L.spz_amd_sort_close(ctx)
    assert np.array_equal(h_order, want_order)
    assert h_out.tobytes() == want


def test_ten_million_keys_and_cli_key_file(spz, big, tmp_path):
    path, raw, _, _ = big
    n = parse_stream(raw)["num_points"]
    rng = np.random.default_rng(8)
    k = rng.standard_normal(n).astype(np.float32)
    k[rng.integers(0, n, 1000)] = np.nan
    want = key_order(k, True)
    out = str(tmp_path / "py.spz")
    order = spz.sort_spz(path, out, keys=k, descending=True)
    assert np.array_equal(order, want)
    with open(out, "rb") as f:
        file_py = f.read()
    assert zlib.decompress(file_py, 31) == expected_stream(raw, want)
    kf = tmp_path / "k.f32"
    kf.write_bytes(k.astype("<f4").tobytes())
    cli = tmp_path / "cli.spz"
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_sort")
    r = subprocess.run([exe, path, str(cli), "--keys", str(kf), "--descending"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert cli.read_bytes() == file_py
    # a key file one float short: exit 1, no output
    kf.write_bytes(k[:-1].astype("<f4").tobytes())
    cli.unlink()
    r = subprocess.run([exe, path, str(cli), "--keys", str(kf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and not cli.exists()
