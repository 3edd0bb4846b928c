"""spz.clean_spz / spz::cleanSpz / spz_clean (DESIGN §8 "Clean") without a GPU: the restatement of tests/clean_ref.py
against an independent O(n^2) loop, the workspace size, the argument checks (which must fail before any device work)
and the CLI's usage line."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from clean_ref import (clean, k_eff, knn_d2, radius_counts, radius_r2, scores_of, stored_positions, threshold_of)
from conftest import ROOT
from test_decimate_host import fields_cases, with_fields
from test_filter_host import parse_stream
from test_sort_host import sortable_goldens


def loop_clean(P, fb, k, std_ratio, r2, m):
    """The contract, one pair at a time."""
    n = len(P)
    ke = min(k, n - 1) if n else 0
    scores, counts = [], []
    for i in range(n):
        d2 = sorted(sum((int(P[i][a]) - int(P[j][a])) ** 2 for a in range(3)) for j in range(n) if j != i)
        s = 0.0
        for x in d2[:ke]:
            s += math.sqrt(x)
        scores.append(s / ke * 2.0 ** -fb if ke else 0.0)
        counts.append(min(sum(1 for x in d2 if x <= r2), m))
    mean = sum(scores) / n if n else 0.0
    std = math.sqrt(sum((x - mean) ** 2 for x in scores) / (n - 1)) if n > 1 else 0.0
    thr = mean + std_ratio * std
    keep = [n <= 1 or (scores[i] <= thr and counts[i] >= m) for i in range(n)]
    return scores, counts, thr, keep


def tiny_positions():
    rng = np.random.default_rng(5)
    return {
        "random": rng.integers(-(1 << 23), 1 << 23, (30, 3)),
        "duplicates": np.repeat(rng.integers(-50, 50, (6, 3)), 5, axis=0),
        "line": np.stack([np.arange(12) ** 2, np.zeros(12, int), np.zeros(12, int)], axis=1),
        "two": np.array([[0, 0, 0], [3, 4, 0]]),
        "one": np.array([[7, 7, 7]]),
    }


@pytest.mark.parametrize("case", sorted(tiny_positions()))
@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_restatement_equals_a_pair_loop(case, k):
    P = tiny_positions()[case].astype(np.int64)
    fb, ratio, m = 12, 1.0, 2
    r2 = radius_r2(0.01, fb)
    scores, counts, thr, keep = loop_clean(P, fb, k, ratio, r2, m)
    d2 = knn_d2(P, k)
    assert d2.shape == (len(P), k_eff(len(P), k))
    got = scores_of(d2, fb)
    assert np.array_equal(got, np.array(scores, np.float64)), "scores bit for bit"
    assert np.array_equal(radius_counts(P, r2, m), counts)
    assert threshold_of(got, ratio) == pytest.approx(thr, rel=1e-12, abs=1e-300)
    want_keep = np.array(keep, bool)
    if len(P) > 1:
        want_keep = (got <= threshold_of(got, ratio)) & (radius_counts(P, r2, m) >= m)
    assert np.array_equal(want_keep, np.array(keep, bool))


def test_duplicates_count_at_distance_zero():
    P = np.array([[1, 2, 3]] * 4 + [[100, 2, 3]], np.int64)
    d2 = knn_d2(P, 3)
    assert np.array_equal(d2[:4], np.zeros((4, 3), np.int64))
    assert np.array_equal(d2[4], [99 ** 2] * 3)


def test_tree_route_equals_brute_force():
    pytest.importorskip("scipy.spatial")
    raw = with_fields(sortable_goldens()["v3_sh1"], fields_cases()["clustered"])
    P = stored_positions(raw)
    for k in (1, 8, 20):
        assert np.array_equal(knn_d2(P, k, "tree"), knn_d2(P, k, "brute"))


@pytest.mark.parametrize("case", sorted(fields_cases()))
def test_restated_stream_keeps_what_the_mask_says(case):
    raw = with_fields(sortable_goldens()["v3_sh1"], fields_cases()[case])
    h = parse_stream(raw)
    r = clean(raw, k=8, std_ratio=1.0, radius=0.05, min_neighbors=3)
    assert r["keep"].shape == (h["num_points"],)
    assert np.array_equal(r["keep"], (r["scores"] <= r["threshold"]) & (r["counts"] >= 3))
    assert np.all(r["kth_d2"] == knn_d2(raw, 8)[:, -1])


def test_radius_r2_rule():
    assert radius_r2(1.0, 12) == 1 << 24
    assert radius_r2(0.1, 12) == math.floor((0.1 * 4096) ** 2)
    assert radius_r2(1e-9, 12) == 0


# ---- the C ABI without a device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from spz_amd import abi
    return abi.load_library()


def test_workspace_bytes_is_host_only_and_monotone(lib):
    sizes = [0, 1, 63, 64, 2047, 2048, 2049, 1 << 20, 10_000_000]
    ws = [int(lib.spz_amd_clean_workspace_bytes(n)) for n in sizes]
    assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:]))
    for n, w in zip(sizes[1:], ws[1:]):
        assert w >= int(lib.spz_amd_sort_workspace_bytes(n)) + 21 * n


def test_radius_r2_of_the_library_equals_the_restatement(lib):
    from spz_amd import abi
    r2 = C.c_uint64()
    for radius, fb in ((1.0, 12), (0.1, 12), (0.37, 8), (3.0, 23), (1e-9, 12), (1e30, 12)):
        assert lib.spz_amd_clean_radius_r2(radius, fb, C.byref(r2)) == abi.OK
        assert r2.value == min(radius_r2(radius, fb), (1 << 64) - 1)
    for radius, fb in ((0.0, 12), (-1.0, 12), (math.inf, 12), (math.nan, 12), (1.0, -1), (1.0, 25)):
        assert lib.spz_amd_clean_radius_r2(radius, fb, C.byref(r2)) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_clean_radius_r2(1.0, 12, None) == abi.ERR_INVALID_ARG


def test_device_entry_points_reject_bad_arguments_without_launching(lib):
    from spz_amd import abi
    raw = bytearray(sortable_goldens()["v3_sh1"])
    n = parse_stream(bytes(raw))["num_points"]
    buf = (C.c_uint8 * len(raw)).from_buffer(raw)
    p = C.addressof(buf)
    hdr = abi.peek_header(bytes(raw))[1]
    dummy = (C.c_uint8 * 64)()
    d = C.addressof(dummy)
    v1 = abi.Header(1, n, hdr.sh_degree, 12, 0, 0)
    bad = abi.Header(4, n, hdr.sh_degree, 12, 0, 0)
    big = abi.Header(3, abi.REFERENCE_MAX_POINTS + 1, 0, 12, 0, 0)
    big_size = abi.stream_layout(big.num_points, 0, 3).total_bytes
    ks = lib.spz_amd_knn_scores_device
    assert ks(None, len(raw), C.byref(hdr), 8, d, d, d, None) == abi.ERR_INVALID_ARG
    assert ks(p, len(raw), None, 8, d, d, d, None) == abi.ERR_INVALID_ARG
    assert ks(p, len(raw) - 1, C.byref(hdr), 8, d, d, d, None) == abi.ERR_SHORT_STREAM
    for k in (0, -1, 65):
        assert ks(p, len(raw), C.byref(hdr), k, d, d, d, None) == abi.ERR_INVALID_ARG
    assert ks(p, len(raw), C.byref(hdr), 8, None, d, d, None) == abi.ERR_INVALID_ARG
    assert ks(p, len(raw), C.byref(hdr), 8, d, d, None, None) == abi.ERR_INVALID_ARG
    assert ks(p, len(raw), C.byref(v1), 8, d, d, d, None) == abi.ERR_UNSUPPORTED
    assert ks(p, len(raw), C.byref(bad), 8, d, d, d, None) == abi.ERR_VERSION
    assert ks(p, big_size, C.byref(big), 8, d, d, d, None) == abi.ERR_TOO_MANY_POINTS
    rc = lib.spz_amd_radius_counts_device
    for m in (0, 257):
        assert rc(p, len(raw), C.byref(hdr), 100, m, d, d, None) == abi.ERR_INVALID_ARG
    assert rc(p, len(raw), C.byref(hdr), 100, 4, None, d, None) == abi.ERR_INVALID_ARG
    assert rc(p, len(raw), C.byref(hdr), 100, 4, d, None, None) == abi.ERR_INVALID_ARG
    assert rc(p, len(raw), C.byref(v1), 100, 4, d, d, None) == abi.ERR_UNSUPPORTED
    assert rc(p, big_size, C.byref(big), 100, 4, d, d, None) == abi.ERR_TOO_MANY_POINTS
    ctx, nbytes = C.c_void_p(), C.c_uint64()
    op = lib.spz_amd_clean_open

    def o(h, k, ratio, radius, m, size=len(raw), scores=None):
        return op(p, size, C.byref(h), k, ratio, radius, m, 0, C.byref(ctx), C.byref(nbytes), None, None, None,
                  scores, None)

    assert o(hdr, 0, 2.0, 1.0, 0) == abi.ERR_INVALID_ARG                  # no rule
    assert o(hdr, 65, 2.0, 0.0, 0) == abi.ERR_INVALID_ARG
    assert o(hdr, -3, 2.0, 0.0, 0) == abi.ERR_INVALID_ARG
    for ratio in (math.nan, math.inf, -math.inf):
        assert o(hdr, 8, ratio, 0.0, 0) == abi.ERR_INVALID_ARG
    for radius in (0.0, -1.0, math.nan, math.inf):
        assert o(hdr, 0, 2.0, radius, 4) == abi.ERR_INVALID_ARG
    assert o(hdr, 0, 2.0, 1.0, 257) == abi.ERR_INVALID_ARG
    assert o(hdr, 0, 2.0, 1.0, 4, scores=d) == abi.ERR_INVALID_ARG        # scores without the statistical rule
    assert o(v1, 8, 2.0, 0.0, 0) == abi.ERR_UNSUPPORTED
    assert o(hdr, 8, 2.0, 0.0, 0, len(raw) - 1) == abi.ERR_SHORT_STREAM
    assert o(big, 8, 2.0, 0.0, 0, big_size) == abi.ERR_TOO_MANY_POINTS
    assert op(p, len(raw), C.byref(hdr), 8, 2.0, 0.0, 0, 0, None, C.byref(nbytes), None, None, None, None,
              None) == abi.ERR_INVALID_ARG
    assert ctx.value is None and nbytes.value == 0
    assert lib.spz_amd_clean_fetch(None, d) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_clean_device_data(None) is None
    lib.spz_amd_clean_close(None)


# ---- argument checks: ValueError before any device work ----------------------------------------------------------
@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


@pytest.fixture()
def some_file(tmp_path):
    p = tmp_path / "in.spz"
    p.write_bytes(b"not read: the arguments are checked first")
    return str(p)


@pytest.mark.parametrize("kw", [
    dict(), dict(std_ratio=1.0), dict(k=0), dict(k=65), dict(k=2.0), dict(k=True), dict(k="8"),
    dict(k=8, std_ratio=math.nan), dict(k=8, std_ratio=math.inf), dict(k=8, std_ratio="2"), dict(k=8, std_ratio=None),
    dict(radius=0.1), dict(min_neighbors=3), dict(radius=0.0, min_neighbors=3), dict(radius=-1.0, min_neighbors=3),
    dict(radius=math.nan, min_neighbors=3), dict(radius=math.inf, min_neighbors=3), dict(radius=0.1, min_neighbors=0),
    dict(radius=0.1, min_neighbors=257), dict(radius=0.1, min_neighbors=2.0), dict(radius=True, min_neighbors=3),
    dict(k=8, return_details=1), dict(k=8, return_details=None),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()) or "none")
def test_bad_arguments_raise_value_error_before_device_work(spz, some_file, tmp_path, kw):
    with pytest.raises(ValueError):
        spz.clean_spz(some_file, str(tmp_path / "out.spz"), **kw)
    assert not (tmp_path / "out.spz").exists()


def test_device_clean_functions_check_their_arguments():
    torch = pytest.importorskip("torch")
    from spz_amd import device as D
    hdr = D.make_header(10, 2)
    st = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        D.knn_scores(st, hdr, 8)                              # not a CUDA tensor
    with pytest.raises(ValueError):
        D.radius_counts(st, hdr, 0.1, 3)
    v1 = D.make_header(10, 2, version=1)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            D.knn_scores(st, v1 if bad == 2.0 else hdr, bad)
    for radius, m in ((0.0, 3), (math.nan, 3), (0.1, 0), (0.1, 257), (0.1, 2.5)):
        with pytest.raises(ValueError):
            D.radius_counts(st, hdr, radius, m)


# ---- the CLI -----------------------------------------------------------------------------------------------------
USAGE = "Usage: spz_clean <input.spz> <output.spz> [--k <K> [--std-ratio <S>]] [--radius <R> --min-neighbors <M>]"


@pytest.mark.parametrize("argv", [
    ["spz_clean"], ["spz_clean", "a.spz", "b.spz"], ["spz_tool", "spz_clean", "a.spz"],
    ["spz_clean", "a.spz", "b.spz", "--k"], ["spz_clean", "a.spz", "b.spz", "--k", "0"],
    ["spz_clean", "a.spz", "b.spz", "--k", "65"], ["spz_clean", "a.spz", "b.spz", "--k", "2.5"],
    ["spz_clean", "a.spz", "b.spz", "--std-ratio", "2"], ["spz_clean", "a.spz", "b.spz", "--k", "8", "--std-ratio", "x"],
    ["spz_clean", "a.spz", "b.spz", "--k", "8", "--std-ratio", "nan"], ["spz_clean", "a.spz", "b.spz", "--radius", "1"],
    ["spz_clean", "a.spz", "b.spz", "--min-neighbors", "3"],
    ["spz_clean", "a.spz", "b.spz", "--radius", "0", "--min-neighbors", "3"],
    ["spz_clean", "a.spz", "b.spz", "--radius", "-1", "--min-neighbors", "3"],
    ["spz_clean", "a.spz", "b.spz", "--radius", "1", "--min-neighbors", "257"],
    ["spz_clean", "a.spz", "b.spz", "--k", "8", "--k", "9"], ["spz_clean", "a.spz", "b.spz", "--bogus", "3"],
    ["spz_clean", "--k", "8", "a.spz", "b.spz"],
])
def test_cli_usage(argv, tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith(USAGE)
    assert not (tmp_path / "b.spz").exists()


def test_cli_unreadable_input_exits_1_without_output(tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_clean")
    r = subprocess.run([exe, "missing.spz", "b.spz", "--k", "8"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=60)
    assert r.returncode == 1
    assert not (tmp_path / "b.spz").exists()
