"""spz.merge_spz / spz_amd.device.merge_packed / the C ABI host form / the spz_merge CLI (DESIGN "Merge") on the GPU:
every golden pairing equal to the restatement of tests/test_merge_host.py byte for byte and every file zlib's level-6
gzip of it, split -> merge giving back the file, the lossless case equal to the concatenated floats, a placed input
equal to the transform's sections, the refusals, wave / tile boundaries and 1024 inputs, and 10 M points written with
the same bytes by every surface."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import FIELDS, ROOT
from test_filter_host import golden_streams, parse_stream
from test_merge_host import OPTIONS, PAIRINGS, PLACEMENT, expected_merge
from test_transform_host import params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def write_inputs(tmp_path, raws, tag="in"):
    paths = []
    for i, raw in enumerate(raws):
        p = tmp_path / f"{tag}{i}.spz"
        p.write_bytes(gz(raw))
        paths.append(str(p))
    return paths


def synth_stream(oracle, n, deg, seed, version=3, fractional_bits=12):
    """A v2/v3 stream of spz_amd.synth points; another fractional_bits only relabels the fixed-point positions."""
    from spz_amd.synth import make_cloud_numpy
    s = oracle.pack(make_cloud_numpy(n, deg, seed), n, deg, False, 0, version)
    s[13] = fractional_bits
    return s.tobytes()


def empty_stream(deg=0, fb=12):
    h = np.zeros(16, np.uint8)
    h[:12] = np.array([0x5053474E, 3, 0], "<u4").view(np.uint8)
    h[12], h[13] = deg, fb
    return h.tobytes()


def device_merge(cuda, raws, **kw):
    import torch
    from spz_amd import abi, device as D
    ts = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(cuda) for r in raws]
    hs = [abi.peek_header(r)[1] for r in raws]
    out, hdr, bad = D.merge_packed(ts, hs, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), hdr, int(bad.item())


def test_golden_pairings_byte_for_byte(spz, tmp_path, oracle):
    g = golden_streams()
    for pair in PAIRINGS:
        raws = [g[p] for p in pair]
        paths = write_inputs(tmp_path, raws)
        flags = {parse_stream(r)["flags"] & 1 for r in raws}
        for placed in (False, True):
            xfs = [None, params(**PLACEMENT)] if placed else None
            for kw in OPTIONS:
                kw = dict(kw)
                if len(flags) > 1:
                    kw["antialiased"] = 1
                want, bad = expected_merge(oracle, raws, xfs, **kw)
                what = f"{pair} placed={placed} {kw}"
                dst = tmp_path / "out.spz"
                if dst.exists():
                    dst.unlink()
                tr = [None, PLACEMENT] if placed else None
                if bad:
                    with pytest.raises(ValueError):
                        spz.merge_spz(paths, str(dst), transforms=tr, **kw)
                    assert not dst.exists(), what
                    continue
                n = spz.merge_spz(paths, str(dst), transforms=tr, **kw)
                f = dst.read_bytes()
                assert n == sum(parse_stream(r)["num_points"] for r in raws)
                assert zlib.decompress(f, 31) == want, what
                assert f == gz(want), f"{what}: the file is not zlib's member of the stream"


def saved_file(spz, path, n, deg, seed):
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(n, deg, seed)
    g = spz.GaussianCloud()
    g.sh_degree = deg
    for k in FIELDS:
        setattr(g, k, c[k])
    assert spz.save_spz(g, spz.PackOptions(), str(path))
    return str(path)


def test_split_then_merge_returns_the_file(spz, tmp_path):
    n = 70_001
    a = saved_file(spz, tmp_path / "a.spz", n, 3, 41)
    for k in (0, 1, 256, 40_000, n):
        lo, hi = str(tmp_path / "lo.spz"), str(tmp_path / "hi.spz")
        assert spz.filter_spz(a, lo, indices=np.arange(0, k, dtype=np.uint32)) == k
        assert spz.filter_spz(a, hi, indices=np.arange(k, n, dtype=np.uint32)) == n - k
        out = str(tmp_path / "m.spz")
        assert spz.merge_spz([lo, hi], out) == n
        with open(out, "rb") as f, open(a, "rb") as g:
            assert f.read() == g.read(), f"split at {k}"
    out = str(tmp_path / "one.spz")
    spz.merge_spz([a], out)
    with open(out, "rb") as f, open(a, "rb") as g:
        assert f.read() == g.read()


def test_lossless_merge_is_the_concatenated_floats(spz, tmp_path):
    paths = [saved_file(spz, tmp_path / f"p{i}.spz", n, 2, 50 + i) for i, n in enumerate((3000, 1, 4099))]
    out = str(tmp_path / "m.spz")
    assert spz.merge_spz(paths, out) == 7100
    got = spz.load_spz(out, spz.UnpackOptions())
    parts = [spz.load_spz(p, spz.UnpackOptions()) for p in paths]
    for k in FIELDS:
        want = np.concatenate([np.asarray(getattr(c, k), np.float32) for c in parts])
        assert np.array_equal(np.asarray(getattr(got, k), np.float32).view(np.uint32), want.view(np.uint32)), k


def test_placed_input_equals_the_transform(cuda, oracle):
    import torch
    from spz_amd import abi, device as D
    a, b = synth_stream(oracle, 3001, 3, 61), synth_stream(oracle, 2050, 3, 62)
    for fb in (None, 10, 14):
        got, hdr, bad = device_merge(cuda, [a, b], transforms=[None, PLACEMENT], fractional_bits=fb)
        assert bad == 0
        f2 = 12 if fb is None else fb
        st = torch.frombuffer(bytearray(b), dtype=torch.uint8).to(cuda)
        t, tbad = D.transform_packed(st, abi.peek_header(b)[1], fractional_bits=f2, **PLACEMENT)
        torch.cuda.synchronize()
        m, tr = parse_stream(got)["sections"], parse_stream(t.cpu().numpy().tobytes())["sections"]
        for s in range(6):
            assert np.array_equal(m[s][3001:], tr[s]), f"fb {fb} section {s}"


def test_out_of_range_and_antialiased_refusals(spz, tmp_path, capfd, oracle):
    a, b = synth_stream(oracle, 4099, 1, 71), synth_stream(oracle, 300, 1, 72)
    paths = write_inputs(tmp_path, [a, b])
    dst = tmp_path / "out.spz"
    _, bad = expected_merge(oracle, [a, b], fractional_bits=20)
    assert bad > 0
    with pytest.raises(ValueError):
        spz.merge_spz(paths, str(dst), fractional_bits=20)
    assert f"{bad} of 4399 points" in capfd.readouterr().out
    assert not dst.exists()
    c = bytearray(b)
    c[14] = 1   # antialiased
    paths = write_inputs(tmp_path, [a, bytes(c)], "aa")
    with pytest.raises(ValueError):
        spz.merge_spz(paths, str(dst))
    msg = capfd.readouterr().out
    assert "antialiased = 0" in msg and "antialiased = 1" in msg and not dst.exists()
    assert spz.merge_spz(paths, str(dst), antialiased=1) == 4399
    want, _ = expected_merge(oracle, [a, bytes(c)], antialiased=1)
    assert zlib.decompress(dst.read_bytes(), 31) == want


def test_wave_and_tile_boundaries(cuda, oracle):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257]
    raws = []
    for i, n in enumerate(sizes):
        deg, ver, fb = i % 4, (3, 2, 3, 2)[i % 4], (12, 12, 10, 8)[i % 4]
        raws.append(empty_stream(deg) if n == 0 else synth_stream(oracle, n, deg, 80 + i, ver, fb))
    for kw in (dict(), dict(sh_degree=1), dict(fractional_bits=14)):
        for xfs in (None, [PLACEMENT if i % 3 == 1 else None for i in range(len(raws))]):
            got, hdr, bad = device_merge(cuda, raws, transforms=xfs, **kw)
            want, wbad = expected_merge(oracle, raws, [params(**x) if x else None for x in xfs] if xfs else None, **kw)
            assert got == want and bad == wbad == 0, f"{kw} placed={xfs is not None}"
    # every input alone, at its own settings
    for raw in raws:
        got, _, _ = device_merge(cuda, [raw])
        assert got == expected_merge(oracle, [raw])[0]


def test_1024_tiny_inputs(cuda, oracle):
    from spz_amd import abi
    rng = np.random.default_rng(5)
    raws = [synth_stream(oracle, int(n), 1 + i % 3, 1000 + i) if n else empty_stream(1)
            for i, n in enumerate(rng.integers(0, 4, abi.MERGE_MAX_INPUTS))]
    xfs = [PLACEMENT if i % 5 == 0 else None for i in range(len(raws))]
    got, hdr, bad = device_merge(cuda, raws, transforms=xfs)
    want, _ = expected_merge(oracle, raws, [params(**x) if x else None for x in xfs])
    assert got == want and hdr.num_points == sum(parse_stream(r)["num_points"] for r in raws)
    got, _, _ = device_merge(cuda, raws)
    assert got == expected_merge(oracle, raws)[0]


def test_ten_million_every_surface_writes_the_same_bytes(spz, tmp_path, cuda):
    import torch
    from spz_amd import abi, device as D
    n = 5_000_000
    paths = [saved_file(spz, tmp_path / f"big{i}.spz", n, 3, 2025 + i) for i in range(2)]
    py = str(tmp_path / "py.spz")
    assert spz.merge_spz(paths, py) == 2 * n
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_merge")
    r = subprocess.run([exe, *paths, "-o", str(tmp_path / "cli.spz")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(py, "rb") as f:
        file_py = f.read()
    assert file_py == (tmp_path / "cli.spz").read_bytes()
    stream = zlib.decompress(file_py, 31)
    # the lossless case: the header and the concatenated sections
    ins = []
    for p in paths:
        with open(p, "rb") as f:
            ins.append(zlib.decompress(f.read(), 31))
    hs = [parse_stream(s) for s in ins]
    ho = parse_stream(stream)
    assert (ho["num_points"], ho["sh_degree"], ho["fractional_bits"], ho["version"]) == (2 * n, 3, 12, 3)
    for s in range(6):
        assert np.array_equal(ho["sections"][s][:n], hs[0]["sections"][s]), s
        assert np.array_equal(ho["sections"][s][n:], hs[1]["sections"][s]), s
    del hs, ho
    # merge_packed + gzip
    ts = [torch.frombuffer(bytearray(s), dtype=torch.uint8).to(cuda) for s in ins]
    heads = [abi.peek_header(s)[1] for s in ins]
    out, hdr, bad = D.merge_packed(ts, heads)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and out.cpu().numpy().tobytes() == stream
    # the C ABI host form
    L = abi.load_library()
    arr = (abi.MergeInput * 2)()
    for i in range(2):
        arr[i].d_stream, arr[i].size, arr[i].hdr, arr[i].xf = ts[i].data_ptr(), ts[i].numel(), heads[i], None
    ctx, oh, nb, nbad, ms = C.c_void_p(), abi.Header(), C.c_uint64(), C.c_uint64(), (C.c_float * 1)()
    assert L.spz_amd_merge_open(arr, 2, -1, -1, -1, 0, C.byref(ctx), C.byref(oh), C.byref(nb), C.byref(nbad), ms) == abi.OK
    try:
        host = np.empty(nb.value, np.uint8)
        assert L.spz_amd_merge_fetch(ctx, host.ctypes.data) == abi.OK
        assert nbad.value == 0 and oh.num_points == 2 * n and ms[0] > 0
        assert host.tobytes() == stream
    finally:
        L.spz_amd_merge_close(ctx)
    assert gz(stream) == file_py
