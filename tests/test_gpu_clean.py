"""spz.clean_spz / spz_clean / spz_amd_clean_open / spz_amd.device.knn_scores + radius_counts (DESIGN §8 "Clean") on the
GPU, against the numpy restatement of tests/clean_ref.py: the scores bit for bit, the k-th squared distances and the
radius counts exactly, the mask equal to scores <= threshold, the threshold within 1e-12, the stream byte for byte
equal to filter_spz with the same mask, and two runs equal."""
import ctypes as C
import os
import struct
import subprocess
import time
import zlib

import numpy as np
import pytest

from clean_ref import clean, knn_d2, radius_counts, radius_r2, scores_of, stored_positions, threshold_of
from conftest import ROOT
from test_decimate_host import fields_cases, with_fields
from test_filter_host import MAGIC, golden_streams, parse_stream
from test_sort_host import sortable_goldens

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def run_file(spz, tmp_path, raw, **kw):
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    if dst.exists():
        dst.unlink()
    r = spz.clean_spz(str(src), str(dst), return_details=True, **kw)
    return r, dst.read_bytes()


def filtered(spz, tmp_path, raw, mask):
    src, dst = tmp_path / "fin.spz", tmp_path / "fout.spz"
    src.write_bytes(gz(raw))
    spz.filter_spz(str(src), str(dst), mask=np.asarray(mask, bool))
    return dst.read_bytes()


def on_device(raw):
    import torch
    from spz_amd import abi
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda"), abi.peek_header(raw)[1]


def check(spz, tmp_path, raw, k=None, std_ratio=2.0, radius=None, min_neighbors=None):
    """The file form against the restatement; returns (kept, mask, scores, thr, file bytes)."""
    (kept, mask, scores, thr), got = run_file(spz, tmp_path, raw, k=k, std_ratio=std_ratio, radius=radius,
                                              min_neighbors=min_neighbors)
    want = clean(raw, k=k, std_ratio=std_ratio, radius=radius, min_neighbors=min_neighbors)
    n = parse_stream(raw)["num_points"]
    assert mask.shape == (n,) and mask.dtype == bool
    assert kept == int(mask.sum())
    if k is not None:
        assert np.array_equal(scores.view(np.uint64), want["scores"].view(np.uint64)), "scores bit for bit"
        if n:
            assert thr == pytest.approx(want["threshold"], rel=1e-12, abs=1e-300)
        base = scores <= thr if n > 1 else np.ones(n, bool)
    else:
        assert scores is None and thr is None
        base = np.ones(n, bool)
    if radius is not None:
        base = base & (want["counts"] >= min_neighbors) if n > 1 else base
    assert np.array_equal(mask, base), "the mask is scores <= threshold (and the radius rule)"
    assert got == filtered(spz, tmp_path, raw, mask), "the stream is the filter's"
    return kept, mask, scores, thr, got


@pytest.mark.parametrize("name", sorted(sortable_goldens()))
def test_goldens(spz, tmp_path, name):
    raw = sortable_goldens()[name]
    for k in (1, 8, 20, 64):
        check(spz, tmp_path, raw, k=k)
    check(spz, tmp_path, raw, radius=0.05, min_neighbors=4)
    check(spz, tmp_path, raw, k=20, std_ratio=0.5, radius=0.2, min_neighbors=2)


@pytest.mark.parametrize("case", sorted(fields_cases()))
def test_position_fields(spz, tmp_path, case):
    raw = with_fields(sortable_goldens()["v3_sh1"], fields_cases()[case])
    for k in (1, 8, 20, 64):
        check(spz, tmp_path, raw, k=k, std_ratio=1.0)
    for radius, m in ((1e-3, 1), (0.05, 8), (2000.0, 256)):
        check(spz, tmp_path, raw, radius=radius, min_neighbors=m)


def stream_of(fields, deg=0, fb=12, seed=0, flags=0, version=3):
    """A v2/v3 stream of the stored position fields `fields` ((N, 3) 24-bit ints), other bytes random."""
    f = np.asarray(fields, np.uint32).reshape(-1, 3)
    n = f.shape[0]
    rng = np.random.default_rng(seed)
    dim = {0: 0, 1: 3, 2: 8, 3: 15}[deg]
    pos = np.stack([(f >> s) & 0xFF for s in (0, 8, 16)], axis=2).astype(np.uint8).reshape(-1)
    rot = 3 if version == 2 else 4
    rest = rng.integers(0, 256, n * (1 + 3 + 3 + rot + 3 * dim), dtype=np.uint8)
    return struct.pack("<IIIBBBB", MAGIC, version, n, deg, fb, flags, 0) + pos.tobytes() + rest.tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, 20, 21, 5000])
def test_edge_sizes(spz, tmp_path, n):
    rng = np.random.default_rng(n)
    fields = rng.integers(0x7f0000, 0x810000, (n, 3))
    raw = stream_of(fields, deg=1, seed=n, flags=1)
    kept, mask, _, _, got = check(spz, tmp_path, raw, k=20)
    if n <= 1:
        assert kept == n
    check(spz, tmp_path, raw, radius=0.5, min_neighbors=3)
    h = parse_stream(zlib.decompress(got, 31))
    assert h["num_points"] == kept and h["version"] == 3 and h["flags"] == 1


def test_resident_forms_determinism_and_the_file_form(spz, tmp_path, cuda):
    import torch
    from spz_amd import device as D
    rng = np.random.default_rng(11)
    fields = np.concatenate([rng.integers(0x7c0000, 0x840000, (6000, 3)), rng.integers(0, 1 << 24, (300, 3)),
                             np.full((400, 3), 0x801234)])
    raw = stream_of(fields[rng.permutation(fields.shape[0])], deg=2, seed=3)
    st, hdr = on_device(raw)
    P = stored_positions(raw)
    for k in (1, 8, 20, 64):
        s1, kth1 = D.knn_scores(st, hdr, k)
        s2, kth2 = D.knn_scores(st, hdr, k)
        torch.cuda.synchronize()
        assert torch.equal(s1, s2) and torch.equal(kth1, kth2), "two runs differ"
        d2 = knn_d2(P, k)
        assert np.array_equal(kth1.cpu().numpy(), d2[:, -1]), "k-th d2"
        assert np.array_equal(s1.cpu().numpy().view(np.uint64), scores_of(d2, 12).view(np.uint64)), "scores"
    for radius, m in ((0.01, 4), (0.3, 64)):
        c = D.radius_counts(st, hdr, radius, m)
        torch.cuda.synchronize()
        assert np.array_equal(c.cpu().numpy(), radius_counts(P, radius_r2(radius, 12), m)), "counts"
    # the file form: its scores are the resident ones, its mask selects its bytes
    s, _ = D.knn_scores(st, hdr, 20)
    c = D.radius_counts(st, hdr, 0.3, 64)
    (kept, mask, scores, thr), got = run_file(spz, tmp_path, raw, k=20, radius=0.3, min_neighbors=64)
    (kept2, _, _, thr2), got2 = run_file(spz, tmp_path, raw, k=20, radius=0.3, min_neighbors=64)
    assert got == got2 and kept == kept2 and thr == thr2, "two runs differ"
    assert np.array_equal(s.cpu().numpy().view(np.uint64), scores.view(np.uint64))
    keep = (s <= thr) & (c >= 64)
    assert np.array_equal(keep.cpu().numpy(), mask)
    out = D.subset(st, hdr, D.select(st, hdr, mask=keep))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == zlib.decompress(got, 31)


def walk_cloud(seed=33):
    """4097 stored position fields whose nearest-neighbour distances span several octree levels: a dense and a loose
    cluster, uniform points over the whole cube and four points repeated fifty times each; shuffled."""
    rng = np.random.default_rng(seed)
    dense = 0x800000 + rng.integers(0, 1 << 10, (1500, 3))
    loose = 0x300000 + rng.integers(0, 1 << 16, (1400, 3))
    spread = rng.integers(0, 1 << 24, (997, 3))
    fields = np.concatenate([dense, loose, spread, np.repeat(dense[:4], 50, axis=0)])
    return fields[rng.permutation(fields.shape[0])]


def test_radius_counts_agree_with_the_nearest_neighbour(cuda):
    """The two searches of the shared walk against each other: a point has a neighbour within the radius exactly where
    its nearest neighbour's squared distance is <= R2.  The radius is the median nearest-neighbour distance of the CPU
    reference, so both outcomes are common."""
    import torch
    from spz_amd import abi, device as D
    raw = stream_of(walk_cloud(), deg=0, seed=33)
    assert parse_stream(raw)["num_points"] == 4097
    nearest = knn_d2(stored_positions(raw), 1)[:, -1]
    radius = float(np.sqrt(np.median(nearest))) * 2.0 ** -12
    r2 = C.c_uint64(0)
    assert abi.load_library().spz_amd_clean_radius_r2(radius, 12, C.byref(r2)) == 0
    st, hdr = on_device(raw)
    _, kth = D.knn_scores(st, hdr, 1)
    counts = D.radius_counts(st, hdr, radius, 1)
    torch.cuda.synchronize()
    within = kth.cpu().numpy() <= r2.value
    assert np.array_equal(counts.cpu().numpy() >= 1, within)
    assert 0.1 <= within.mean() <= 0.9, "each outcome for at least a tenth of the points"


def test_c_abi_host_form(cuda):
    import torch
    from spz_amd import abi
    L = abi.load_library()
    rng = np.random.default_rng(4)
    raw = stream_of(rng.integers(0x700000, 0x900000, (7000, 3)), deg=1, seed=4, flags=1)
    st, hdr = on_device(raw)
    n = hdr.num_points
    want = clean(raw, k=12, std_ratio=1.5, radius=0.5, min_neighbors=5)
    ctx, nbytes, kept, thr = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_double()
    mask, scores = np.zeros(n, np.uint8), np.zeros(n, np.float64)
    ms = (C.c_float * 3)()
    rc = L.spz_amd_clean_open(st.data_ptr(), st.numel(), C.byref(hdr), 12, 1.5, 0.5, 5, torch.cuda.current_device(),
                              C.byref(ctx), C.byref(nbytes), C.byref(kept), C.byref(thr), mask.ctypes.data,
                              scores.ctypes.data, ms)
    assert rc == 0
    try:
        out = np.zeros(nbytes.value, np.uint8)
        assert L.spz_amd_clean_fetch(ctx, out.ctypes.data) == 0
        assert L.spz_amd_clean_device_data(ctx) is not None
    finally:
        L.spz_amd_clean_close(ctx)
    assert np.array_equal(scores.view(np.uint64), want["scores"].view(np.uint64))
    assert thr.value == pytest.approx(want["threshold"], rel=1e-12)
    assert np.array_equal(mask.astype(bool), (scores <= thr.value) & (want["counts"] >= 5))
    assert kept.value == int(mask.sum())
    idx = np.flatnonzero(mask)
    h = parse_stream(out.tobytes())
    assert h["num_points"] == kept.value and h["flags"] == 1
    src = parse_stream(raw)
    for s in range(6):
        assert np.array_equal(h["sections"][s], src["sections"][s][idx]), f"section {s}"


def test_version_1_is_refused(spz, tmp_path):
    raw = golden_streams()["v1"]
    (tmp_path / "in.spz").write_bytes(gz(raw))
    with pytest.raises(ValueError):
        spz.clean_spz(str(tmp_path / "in.spz"), str(tmp_path / "out.spz"), k=8)
    assert not (tmp_path / "out.spz").exists()


def test_cli(spz, tmp_path, cuda):
    rng = np.random.default_rng(6)
    raw = stream_of(rng.integers(0x780000, 0x880000, (4000, 3)), deg=2, seed=6)
    (tmp_path / "in.spz").write_bytes(gz(raw))
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_clean")
    for args, kw in ((["--k", "10", "--std-ratio", "1"], dict(k=10, std_ratio=1.0)),
                     (["--radius", "0.4", "--min-neighbors", "6"], dict(radius=0.4, min_neighbors=6))):
        r = subprocess.run([exe, "in.spz", "out.spz"] + args, capture_output=True, text=True, cwd=str(tmp_path),
                           timeout=300)
        assert r.returncode == 0, r.stderr
        (_, mask, _, _), got = run_file(spz, tmp_path, raw, **kw)
        assert (tmp_path / "out.spz").exists()
        assert zlib.decompress((tmp_path / "out.spz").read_bytes(), 31) == zlib.decompress(got, 31)


def clustered_scene(seed=21):
    """1 M points: 90 % in 1 % of the volume, 10 000 exact duplicates there, 1 % uniform floaters, the rest in 200
    blobs; shuffled.  Returns (fields, is_floater, is_core)."""
    rng = np.random.default_rng(seed)
    edge = int(0.2154 * (1 << 24))
    lo = (1 << 23) - edge // 2
    core = lo + rng.integers(0, edge, (890_000, 3))
    dup = np.repeat(core[:1], 10_000, axis=0)
    floaters = rng.integers(0, 1 << 24, (10_000, 3))
    centres = rng.integers(1 << 20, (1 << 24) - (1 << 20), (200, 3))
    blobs = centres[rng.integers(0, 200, 90_000)] + rng.normal(0, 1 << 14, (90_000, 3)).astype(np.int64)
    blobs = np.clip(blobs, 0, (1 << 24) - 1)
    fields = np.concatenate([core, dup, floaters, blobs])
    kind = np.concatenate([np.full(900_000, 1), np.full(10_000, 2), np.full(90_000, 3)])
    inside = np.all((fields >= lo) & (fields < lo + edge), axis=1)
    perm = rng.permutation(fields.shape[0])
    return fields[perm], ((kind == 2) & ~inside)[perm], (kind == 1)[perm]


def test_one_million_point_clustered_scene(spz, tmp_path):
    pytest.importorskip("scipy.spatial")
    fields, floater, core = clustered_scene()
    raw = stream_of(fields, deg=0, seed=1)
    src, dst = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(raw))
    spz.clean_spz(str(src), str(dst), k=20)                      # warm-up
    t0 = time.perf_counter()
    kept, mask, scores, thr = spz.clean_spz(str(src), str(dst), k=20, return_details=True)
    wall = time.perf_counter() - t0
    assert wall < 30.0, f"clean_spz took {wall:.1f} s for 1 M points"
    d2 = knn_d2(stored_positions(raw), 20)                       # scipy cKDTree, exact d2
    want = scores_of(d2, 12)
    assert np.array_equal(scores.view(np.uint64), want.view(np.uint64)), "scores bit for bit"
    assert thr == pytest.approx(threshold_of(want, 2.0), rel=1e-12)
    assert np.array_equal(mask, scores <= thr)
    assert 1.0 - mask[floater].mean() >= 0.9, "the planted floaters are removed"
    assert 1.0 - mask[core].mean() <= 1e-3, "the core stays"
    assert dst.read_bytes() == filtered(spz, tmp_path, raw, mask)
