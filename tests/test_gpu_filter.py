"""spz.filter_spz / spz_amd.device.select + subset / the C ABI (DESIGN §8 "filter") on the GPU: the output stream is the
numpy restatement of tests/test_filter_host.py byte for byte, the file is zlib's level-6 gzip of it, the reference's own
load_spz reads the kept points back bit for bit, and the selection is np.nonzero of the same predicate on the floats
load_spz returns."""
import os
import zlib

import numpy as np
import pytest

from conftest import FIELDS, load_golden
from test_filter_host import SH_DIM, expected_stream, golden_streams, index_sets, parse_stream

pytestmark = pytest.mark.gpu

PER = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3}


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


def run_filter(spz, tmp_path, raw, **kw):
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    if dst.exists():
        dst.unlink()
    kept = spz.filter_spz(str(src), str(dst), **kw)
    return kept, dst.read_bytes()


def test_golden_streams_every_mode_and_degree(spz, tmp_path):
    ref = reference()
    for name, raw in golden_streams().items():
        h = parse_stream(raw)
        n, deg = h["num_points"], h["sh_degree"]
        sets = index_sets(n)
        rng = np.random.default_rng(11)
        mask = rng.random(n) < 0.5
        for d2 in [None] + list(range(deg + 1)):
            for label, kw, idx in (("mask", dict(mask=mask), np.nonzero(mask)[0]),
                                   ("reversed_dup", dict(indices=sets["reversed_dup"]), sets["reversed_dup"])):
                kept, f = run_filter(spz, tmp_path, raw, sh_degree=d2, **kw)
                want = expected_stream(raw, idx, d2)
                assert kept == idx.size
                assert zlib.decompress(f, 31) == want, f"{name} {label} sh{d2}: stream"
                assert f == gz(want), f"{name} {label} sh{d2}: the file is not zlib's member of the stream"
                if ref is not None:
                    dd = deg if d2 is None else d2
                    got = ref.load_spz(np.frombuffer(f, np.uint8), idx.size, dd)
                    full = ref.load_spz(np.frombuffer(gz(raw), np.uint8), n, deg)
                    assert got["num_points"] == idx.size
                    for k, w in PER.items():
                        assert np.array_equal(got[k].view(np.uint32), full[k].reshape(n, w)[idx].reshape(-1).view(np.uint32)), f"{name} {k}"
                    sh = full["sh"].reshape(n, SH_DIM[deg], 3)[idx, :SH_DIM[dd], :].reshape(-1)
                    assert np.array_equal(got["sh"].view(np.uint32), sh.view(np.uint32)), f"{name} sh"


def edited_stream():
    """A v1 and a v3 stream with alpha bytes 0 and 255 and (v1) NaN positions."""
    lg, cl = load_golden("legacy.npz"), load_golden("clouds.npz")
    out = {}
    for name, raw in (("v1", lg["v1_stream"].tobytes()), ("v3", cl["d2_stream_from0"].tobytes()),
                      ("fb8", lg["fb8_stream"].tobytes())):
        s = bytearray(raw)
        h = parse_stream(raw)
        n = h["num_points"]
        pos_b = 6 if h["version"] == 1 else 9
        a0 = 16 + n * pos_b
        s[a0 + 0], s[a0 + 1], s[a0 + 2] = 0, 255, 255
        if h["version"] == 1:
            s[16 + 6 * 3: 16 + 6 * 3 + 2] = (0x7E00).to_bytes(2, "little")   # point 3: x is a NaN half
        out[name] = bytes(s)
    return out


def test_box_and_min_alpha_equal_the_predicate_on_the_decoded_floats(spz, tmp_path):
    import torch
    from spz_amd import abi, device as D
    for name, raw in edited_stream().items():
        h = parse_stream(raw)
        n = h["num_points"]
        for coord in (abi.UNSPECIFIED, abi.RUB, abi.RDF, abi.LUF):
            o = spz.UnpackOptions()
            o.to_coord = spz.CoordinateSystem(coord)
            c = spz._unpack_from_stream(raw, o)
            p = np.asarray(c.positions).reshape(n, 3)
            alpha = np.asarray(c.alphas)
            finite = p[np.all(np.isfinite(p), axis=1)]
            # bounds that are positions themselves: points exactly on the faces
            lo = np.sort(finite, axis=0)[len(finite) // 5]
            hi = np.sort(finite, axis=0)[(4 * len(finite)) // 5]
            cases = [
                dict(box=[lo, hi]),
                dict(box=[[-np.inf] * 3, [np.inf] * 3]),
                dict(min_alpha=float(np.sort(alpha)[n // 2])),
                dict(min_alpha=-np.inf), dict(min_alpha=np.inf),
                dict(box=[lo, hi], min_alpha=float(np.sort(alpha)[n // 3])),
            ]
            for kw in cases:
                keep = np.ones(n, bool)
                if "box" in kw:
                    b = np.asarray(kw["box"], np.float32)
                    keep &= np.all((b[0] <= p) & (p <= b[1]), axis=1)
                if "min_alpha" in kw:
                    keep &= alpha >= np.float32(kw["min_alpha"])
                idx = np.nonzero(keep)[0]
                kept, f = run_filter(spz, tmp_path, raw, coord=spz.CoordinateSystem(coord), **kw)
                assert kept == idx.size, f"{name} coord {coord} {kw}"
                assert zlib.decompress(f, 31) == expected_stream(raw, idx), f"{name} coord {coord} {kw}"
                # the device form on the same stream
                st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
                hdr = abi.peek_header(raw)[1]
                got = D.select(st, hdr, to_coord=coord, **{k: (np.asarray(v).tolist() if k == "box" else v) for k, v in kw.items()})
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), idx)
        st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
        hdr = abi.peek_header(raw)[1]
        inside = D.select(st, hdr, box=[[-np.inf] * 3, [np.inf] * 3]).cpu().numpy()
        assert (3 not in inside) == (name == "v1")                                 # a NaN position is never inside
        assert 0 in D.select(st, hdr, min_alpha=-np.inf).cpu().numpy()             # byte 0 decodes to -inf
        assert {1, 2} <= set(D.select(st, hdr, min_alpha=np.inf).cpu().numpy())    # byte 255 decodes to +inf


ODD_RUNS_N = 1_048_577   # 1025 select tiles of 1024 points for the 1024 threads of the offset scan: runs of two counts,
                         # the last owning thread holds one, half the block holds none


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, ODD_RUNS_N])
def test_sizes_around_the_wave_and_the_tile(spz, tmp_path, oracle, n):
    from spz_amd.synth import make_cloud_numpy
    deg = 0 if n == ODD_RUNS_N else 3 if n % 2 else 2
    if n == ODD_RUNS_N:
        tiles = -(-n // 1024)
        assert tiles % 2 == 1 and 1024 < tiles < 2 * 1024
    raw = oracle.pack(make_cloud_numpy(n, deg, 100 + n), n, deg, True, 6).tobytes()
    rng = np.random.default_rng(n)
    mask = (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)
    for d2 in range(deg + 1):
        kept, f = run_filter(spz, tmp_path, raw, mask=mask, sh_degree=d2)
        idx = np.nonzero(mask)[0]
        assert kept == idx.size
        assert zlib.decompress(f, 31) == expected_stream(raw, idx, d2)
    kept, f = run_filter(spz, tmp_path, raw)
    assert kept == n and zlib.decompress(f, 31) == raw


def test_no_point_kept_gives_the_zero_point_stream(spz, tmp_path):
    raw = golden_streams()["v3_sh3"]
    n = parse_stream(raw)["num_points"]
    kept, f = run_filter(spz, tmp_path, raw, mask=np.zeros(n, np.uint8), sh_degree=1)
    assert kept == 0
    s = zlib.decompress(f, 31)
    assert s == expected_stream(raw, np.zeros(0, np.int64), 1) and len(s) == 16 and f == gz(s)
    kept, f = run_filter(spz, tmp_path, raw, indices=np.zeros(0, np.uint32))
    assert kept == 0 and zlib.decompress(f, 31) == expected_stream(raw, np.zeros(0, np.int64))


def test_out_of_range_index_and_too_high_degree(spz, tmp_path, capfd):
    raw = golden_streams()["v2"]
    n = parse_stream(raw)["num_points"]
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    with pytest.raises(ValueError):
        spz.filter_spz(str(src), str(dst), indices=np.array([0, n], np.uint32))
    assert "[SPZ ERROR] filterSpz: index" in capfd.readouterr().out
    assert not dst.exists()
    raw0 = golden_streams()["v3_sh0"]
    src.write_bytes(gz(raw0))
    with pytest.raises(ValueError):
        spz.filter_spz(str(src), str(dst), sh_degree=1)
    with pytest.raises(ValueError):
        spz.filter_spz(str(src), str(dst), mask=np.ones(parse_stream(raw0)["num_points"] + 1, bool))
    assert not dst.exists()


def test_device_select_and_subset_on_a_side_stream(spz, cuda):
    import torch
    from spz_amd import abi, device as D
    raw = golden_streams()["v3_sh3"]
    n = parse_stream(raw)["num_points"]
    hdr = abi.peek_header(raw)[1]
    side = torch.cuda.Stream()
    rng = np.random.default_rng(3)
    mask_np = rng.random(n) < 0.3
    with torch.cuda.stream(side):
        st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda, non_blocking=False)
        mask = torch.from_numpy(mask_np).to(cuda)
        idx = D.select(st, hdr, mask=mask, stream=side)
        out = D.subset(st, hdr, idx, sh_degree=1, stream=side)
        rev = torch.flip(torch.arange(n, dtype=torch.int32, device=cuda), [0])
        out_rev = D.subset(st, hdr, rev, stream=side)
    side.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.nonzero(mask_np)[0])
    assert out.cpu().numpy().tobytes() == expected_stream(raw, np.nonzero(mask_np)[0], 1)
    assert out_rev.cpu().numpy().tobytes() == expected_stream(raw, np.arange(n)[::-1])
    with pytest.raises(ValueError):
        D.subset(st, hdr, torch.tensor([0, n], dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        D.subset(st, hdr, torch.tensor([-1], dtype=torch.int32, device=cuda))


def test_c_abi_with_a_caller_workspace(cuda):
    """spz_amd_select_device / spz_amd_subset_device called directly: a workspace at an odd address, and the device
    form's documented clamp of an index past the end."""
    import ctypes as C

    import torch
    from spz_amd import abi
    L = abi.load_library()
    raw = golden_streams()["v1"]
    n = parse_stream(raw)["num_points"]
    hdr = abi.peek_header(raw)[1]
    st = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    ws = torch.empty(int(L.spz_amd_filter_workspace_bytes(n)) + 1, dtype=torch.uint8, device=cuda)
    idx = torch.empty(n, dtype=torch.int32, device=cuda)
    sel = abi.Selection()
    sel.use_min_alpha, sel.min_alpha = 1, 0.0
    count = C.c_uint64(0)
    rc = L.spz_amd_select_device(st.data_ptr(), st.numel(), C.byref(hdr), C.byref(sel), None, idx.data_ptr(),
                                 ws.data_ptr() + 1, C.byref(count), None)
    assert rc == abi.OK
    import spz_amd.spz as m
    alpha = np.asarray(m._unpack_from_stream(raw, m.UnpackOptions()).alphas)
    want = np.nonzero(alpha >= 0.0)[0]
    assert count.value == want.size and np.array_equal(idx[:count.value].cpu().numpy(), want)
    sel.min_alpha = float("nan")
    assert L.spz_amd_select_device(st.data_ptr(), st.numel(), C.byref(hdr), C.byref(sel), None, idx.data_ptr(),
                                   ws.data_ptr(), C.byref(count), None) == abi.ERR_INVALID_ARG
    # clamp: an index past the end reads the last point
    ix = torch.tensor([n + 7, 0], dtype=torch.int32, device=cuda)
    lay = abi.stream_layout(2, 0, 1)
    out = torch.empty(lay.total_bytes, dtype=torch.uint8, device=cuda)
    assert L.spz_amd_subset_device(st.data_ptr(), st.numel(), C.byref(hdr), ix.data_ptr(), 2, 0, out.data_ptr(),
                                   out.numel() - 1, None) == abi.ERR_CAPACITY
    assert L.spz_amd_subset_device(st.data_ptr(), st.numel(), C.byref(hdr), ix.data_ptr(), 2, 4, out.data_ptr(),
                                   out.numel(), None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_subset_device(st.data_ptr(), st.numel(), C.byref(hdr), ix.data_ptr(), 2, 0, out.data_ptr(),
                                   out.numel(), None) == abi.OK
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == expected_stream(raw, [n - 1, 0], 0)


@pytest.fixture(scope="module")
def big(spz, tmp_path_factory):
    """10 M SH3 points from spz_amd.synth, written by save_spz."""
    from spz_amd.synth import make_cloud_numpy
    n, deg = 10_000_000, 3
    c = make_cloud_numpy(n, deg, 2024)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    del c
    po = spz.PackOptions()
    po.from_coord = spz.RDF
    path = str(tmp_path_factory.mktemp("big") / "big.spz")
    assert spz.save_spz(g, po, path)
    saved = spz._save_spz_bytes(g, po)
    raw = spz._pack_to_stream(g, po)
    return path, raw, saved, n


def test_ten_million_sh3_half_mask_to_sh1(spz, big, tmp_path):
    path, raw, _, n = big
    rng = np.random.default_rng(50)
    mask = rng.random(n) < 0.5
    out = str(tmp_path / "half.spz")
    kept = spz.filter_spz(path, out, mask=mask, sh_degree=1)
    idx = np.nonzero(mask)[0]
    assert kept == idx.size
    with open(out, "rb") as f:
        got = zlib.decompress(f.read(), 31)
    assert got == expected_stream(raw, idx, 1)


def test_ten_million_keep_all_is_the_input(spz, big, tmp_path):
    path, raw, saved, n = big
    out = str(tmp_path / "all.spz")
    assert spz.filter_spz(path, out) == n
    with open(out, "rb") as f:
        got = f.read()
    with open(path, "rb") as f:
        assert got == f.read()
    assert got == saved
