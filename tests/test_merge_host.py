"""spz.merge_spz / spz::mergeSpz / spz_merge (DESIGN "Merge") without a GPU: the header resolver's defaults and
refusals (spz_amd_merge_resolve), the argument checks, which must raise before any device work, the CLI's usage line,
and a numpy restatement of the output stream built from the contract's table — per input and section, the input's
bytes where they are copied, else the bytes of Oracle.pack(T(Oracle.unpack(stream))) (tests/test_transform_host.py) —
checked against the oracle's decode of both.  tests/test_gpu_merge.py compares the device's output with it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_filter_host import MAGIC, SH_DIM, golden_streams, parse_stream
from test_transform_host import expected_stream as transformed_stream
from test_transform_host import params


def resolve_header(hs, sh_degree=None, fractional_bits=None, antialiased=None):
    """The output header fields the contract gives for parsed input headers hs."""
    d2 = max(h["sh_degree"] for h in hs) if sh_degree is None else int(sh_degree)
    votes = {h["fractional_bits"] for h in hs if h["version"] >= 2}
    f2 = int(fractional_bits) if fractional_bits is not None else (votes.pop() if len(votes) == 1 else 12)
    aa = int(antialiased) if antialiased is not None else hs[0]["flags"] & 1
    return d2, f2, aa


def expected_merge(oracle, raws, xfs=None, sh_degree=None, fractional_bits=None, antialiased=None):
    """(stream, out-of-range count) of the merge of the raw streams `raws` with placements xfs (None or a parameter
    block per input), restated from the contract's table."""
    hs = [parse_stream(r) for r in raws]
    xfs = xfs if xfs is not None else [None] * len(raws)
    d2, f2, aa = resolve_header(hs, sh_degree, fractional_bits, antialiased)
    n = sum(h["num_points"] for h in hs)
    head = np.zeros(16, np.uint8)
    head[:12] = np.array([MAGIC, 3, n], "<u4").view(np.uint8)
    head[12], head[13], head[14], head[15] = d2, f2, aa, 0
    secs = [[] for _ in range(6)]
    bad = 0
    orec = 3 * SH_DIM[d2]
    for raw, h, xf in zip(raws, hs, xfs):
        ni = h["num_points"]
        if ni == 0:
            continue
        moves = xf is not None and bool(xf.apply_positions)
        rot = xf is not None and bool(xf.apply_rotation)
        scl = xf is not None and bool(xf.apply_scales)
        t_raw, t_bad = transformed_stream(oracle, raw, xf if xf is not None else params(), f2)
        t = parse_stream(t_raw)["sections"]
        src = h["sections"]
        if h["version"] >= 2 and h["fractional_bits"] == f2 and not moves:
            secs[0].append(src[0])
        else:
            secs[0].append(t[0])
            bad += t_bad
        secs[1].append(src[1])
        secs[2].append(src[2])
        secs[3].append(t[3] if scl else src[3])
        secs[4].append(src[4] if h["version"] >= 3 and not rot else t[4])
        rec = t[5] if rot else src[5]
        out = np.full((ni, orec), 128, np.uint8)
        keep = min(rec.shape[1], orec)
        out[:, :keep] = rec[:, :keep]
        secs[5].append(out)
    parts = [head] + [np.ascontiguousarray(np.concatenate(s)).reshape(-1) if s else np.zeros(0, np.uint8) for s in secs]
    return np.concatenate(parts).tobytes(), bad


PAIRINGS = [("v1", "v3_sh3"), ("v2", "v3_sh3"), ("fb8", "v3_sh2"), ("fb23", "fb8"), ("v3_sh0", "v3_sh3"),
            ("v3_sh3", "v3_sh1"), ("v2", "v1"), ("fb0", "v3_sh1")]
OPTIONS = [dict(), dict(sh_degree=0), dict(sh_degree=1), dict(sh_degree=3), dict(fractional_bits=8),
           dict(fractional_bits=12), dict(fractional_bits=16)]
PLACEMENT = dict(rotation=[0.2, -0.4, 0.1, 0.9], translation=[0.5, -1.0, 0.25], scale=1.25)


def assert_floats_equal(got, want, what):
    """Bit for bit, except that any NaN equals any NaN."""
    g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert g.shape == w.shape, what
    gn, wn = np.isnan(g), np.isnan(w)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    assert np.array_equal(g.view(np.uint32)[~gn], w.view(np.uint32)[~wn]), f"{what}: floats differ"


# ---- the restatement against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRINGS, ids="+".join)
@pytest.mark.parametrize("placed", [False, True])
def test_restated_merge_decodes_as_the_table_says(oracle, pair, placed):
    g = golden_streams()
    raws = [g[p] for p in pair]
    xfs = [None, params(**PLACEMENT)] if placed else None
    for kw in OPTIONS:
        aa = kw.get("antialiased", None if len({parse_stream(r)["flags"] & 1 for r in raws}) == 1 else 1)
        out, bad = expected_merge(oracle, raws, xfs, antialiased=aa, **kw)
        rc, got = oracle.unpack(np.frombuffer(out, np.uint8))
        assert rc == 0, f"{pair} {kw}: the oracle rejects the restated stream"
        hs = [parse_stream(r) for r in raws]
        d2, f2, _ = resolve_header(hs, kw.get("sh_degree"), kw.get("fractional_bits"), aa)
        assert got["num_points"] == sum(h["num_points"] for h in hs) and got["sh_degree"] == d2
        at = 0
        for i, (raw, h) in enumerate(zip(raws, hs)):
            xf = xfs[i] if xfs else None
            ni, di = h["num_points"], h["sh_degree"]
            rc, plain = oracle.unpack(np.frombuffer(raw, np.uint8))
            t_raw, _ = transformed_stream(oracle, raw, xf if xf is not None else params(), f2)
            rc, placed_c = oracle.unpack(np.frombuffer(t_raw, np.uint8))
            rot = xf is not None and bool(xf.apply_rotation)
            sl = slice(at, at + ni)
            what = f"{pair} {kw} input {i}"
            per = {"positions": 3, "scales": 3, "alphas": 1, "colors": 3, "rotations": 4}
            want = {"positions": placed_c, "scales": placed_c, "alphas": plain, "colors": plain,
                    "rotations": plain if h["version"] >= 3 and not rot else placed_c}
            for k, w in per.items():
                assert_floats_equal(got[k].reshape(-1, w)[sl], want[k][k].reshape(-1, w), f"{what} {k}")
            sh_src = (placed_c if rot else plain)["sh"].reshape(ni, SH_DIM[di], 3)
            sh_want = np.zeros((ni, SH_DIM[d2], 3), np.float32)
            keep = min(SH_DIM[di], SH_DIM[d2])
            sh_want[:, :keep] = sh_src[:, :keep]
            assert_floats_equal(got["sh"].reshape(got["num_points"], SH_DIM[d2], 3)[sl], sh_want, f"{what} sh")
            at += ni


def test_restated_lossless_cases(oracle):
    g = golden_streams()
    a, b = g["v3_sh2"], g["v3_sh2"]
    ha, hb = parse_stream(a), parse_stream(b)
    out, bad = expected_merge(oracle, [a, b])
    assert bad == 0
    ho = parse_stream(out)
    for s in range(6):
        assert np.array_equal(ho["sections"][s], np.concatenate([ha["sections"][s], hb["sections"][s]]))
    # one v3 file at its own degree and fractionalBits, no placement: its stream
    for name in ("v3_sh0", "v3_sh1", "v3_sh2", "v3_sh3", "fb8", "fb23"):
        assert expected_merge(oracle, [g[name]])[0] == g[name], name


# ---- the resolver -------------------------------------------------------------------------------------------------
def hdr(n=10, deg=3, version=3, fb=12, aa=False):
    from spz_amd import device as D
    return D.make_header(n, deg, version, fb, aa)


def test_resolver_defaults():
    from spz_amd import abi
    rc, h, nbytes = abi.merge_resolve([hdr(10, 1), hdr(5, 3, 2, 12)])
    assert rc == abi.OK and (h.version, h.num_points, h.sh_degree, h.fractional_bits, h.flags, h.reserved) == (3, 15, 3, 12, 0, 0)
    assert nbytes == abi.stream_layout(15, 3, 3).total_bytes
    assert abi.merge_resolve([hdr(fb=8), hdr(fb=8, version=2), hdr(version=1, fb=0)])[1].fractional_bits == 8   # v1 does not vote
    assert abi.merge_resolve([hdr(fb=8), hdr(fb=10)])[1].fractional_bits == 12
    assert abi.merge_resolve([hdr(version=1, fb=3)])[1].fractional_bits == 12
    assert abi.merge_resolve([hdr(aa=True), hdr(aa=True)])[1].flags == 1
    h = abi.merge_resolve([hdr(deg=1, fb=8), hdr(deg=2, fb=8)], sh_degree=0, fractional_bits=20, antialiased=1)[1]
    assert (h.sh_degree, h.fractional_bits, h.flags) == (0, 20, 1)
    assert abi.merge_resolve([hdr(0, 0)])[1].num_points == 0
    assert abi.merge_resolve([hdr(1)] * abi.MERGE_MAX_INPUTS)[1].num_points == abi.MERGE_MAX_INPUTS
    assert abi.merge_resolve([hdr(5_000_000), hdr(5_000_000)])[1].num_points == 10_000_000


@pytest.mark.parametrize("case", ["empty", "too_many_inputs", "too_many_points", "sh_degree", "fractional_bits",
                                  "antialiased", "antialiased_conflict", "version", "degree"])
def test_resolver_refusals(case):
    from spz_amd import abi
    hs, kw, want = [hdr(), hdr()], {}, abi.ERR_INVALID_ARG
    if case == "empty":
        hs = []
    elif case == "too_many_inputs":
        hs = [hdr(1)] * (abi.MERGE_MAX_INPUTS + 1)
    elif case == "too_many_points":
        hs, want = [hdr(5_000_000), hdr(5_000_001)], abi.ERR_TOO_MANY_POINTS
    elif case == "sh_degree":
        kw = dict(sh_degree=4)
    elif case == "fractional_bits":
        kw = dict(fractional_bits=25)
    elif case == "antialiased":
        kw = dict(antialiased=2)
    elif case == "antialiased_conflict":
        hs = [hdr(aa=False), hdr(aa=True)]
    elif case == "version":
        hs, want = [hdr(), hdr(version=4)], abi.ERR_VERSION
    elif case == "degree":
        hs, want = [hdr(), hdr(deg=4)], abi.ERR_SH_DEGREE
    rc, h, _ = abi.merge_resolve(hs, **kw)
    assert rc == want and h is None
    if case == "antialiased_conflict":
        assert abi.merge_resolve(hs, antialiased=0)[0] == abi.OK


def test_workspace_bytes():
    from spz_amd import abi
    L = abi.load_library()
    assert L.spz_amd_merge_workspace_bytes(0) == 0 and L.spz_amd_merge_workspace_bytes(abi.MERGE_MAX_INPUTS + 1) == 0
    assert 0 < L.spz_amd_merge_workspace_bytes(1) < L.spz_amd_merge_workspace_bytes(abi.MERGE_MAX_INPUTS)


# ---- argument checks: ValueError before any device work (no device here) -----------------------------------------
@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


@pytest.fixture()
def two_files(tmp_path):
    out = []
    for k in range(2):
        p = tmp_path / f"in{k}.spz"
        p.write_bytes(b"not read: the arguments are checked first")
        out.append(str(p))
    return out


BAD = [
    dict(sh_degree=4), dict(sh_degree=-1), dict(sh_degree=1.0), dict(sh_degree=True), dict(fractional_bits=25),
    dict(fractional_bits=-1), dict(fractional_bits="12"), dict(antialiased=2), dict(antialiased=-1), dict(antialiased=True),
    dict(transforms=[None]), dict(transforms=[None, None, None]), dict(transforms="ab"), dict(transforms=[None, 3]),
    dict(transforms=[None, dict(scale=0.0)]), dict(transforms=[dict(rotation=[0, 0, 0, 0]), None]),
    dict(transforms=[dict(translation=[0, float("inf"), 0]), None]), dict(transforms=[dict(bogus=1), None]),
    dict(transforms=[dict(coord=9), None]), dict(transforms=[dict(fractional_bits=12), None]),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v!r}"[:40] for k, v in kw.items()))
def test_bad_arguments_raise_value_error_before_device_work(spz, two_files, tmp_path, kw):
    with pytest.raises(ValueError):
        spz.merge_spz(two_files, str(tmp_path / "out.spz"), **kw)
    assert not (tmp_path / "out.spz").exists()


def test_input_counts_raise_value_error(spz, two_files, tmp_path):
    with pytest.raises(ValueError):
        spz.merge_spz([], str(tmp_path / "out.spz"))
    with pytest.raises(ValueError):
        spz.merge_spz([two_files[0]] * 1025, str(tmp_path / "out.spz"))
    assert not (tmp_path / "out.spz").exists()


def test_device_merge_checks_its_arguments():
    torch = pytest.importorskip("torch")
    from spz_amd import device as D
    st = torch.zeros(16, dtype=torch.uint8)
    h = hdr(0, 0)
    for kw in (dict(sh_degree=4), dict(fractional_bits=30), dict(antialiased=2), dict(transforms=[None, None]),
               dict(transforms=[dict(scale=-1.0)])):
        with pytest.raises(ValueError):
            D.merge_packed([st], [h], **kw)
    with pytest.raises(ValueError):
        D.merge_packed([], [])
    with pytest.raises(ValueError):
        D.merge_packed([st], [h, h])
    with pytest.raises(ValueError):
        D.merge_packed([st], [h])   # not a CUDA tensor


# ---- the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["spz_merge"], ["spz_merge", "a.spz"], ["spz_merge", "-o", "b.spz"], ["spz_tool", "spz_merge"],
    ["spz_tool", "spz_merge", "a.spz"], ["spz_merge", "a.spz", "-o"], ["spz_merge", "a.spz", "-o", "b.spz", "-o", "c.spz"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--sh-degree", "4"], ["spz_merge", "a.spz", "-o", "b.spz", "--sh-degree"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--fractional-bits", "25"], ["spz_merge", "a.spz", "-o", "b.spz", "--antialiased", "2"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--antialiased", "x"], ["spz_merge", "a.spz", "-o", "b.spz", "--bogus"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--rotate", "0", "0", "0", "1"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--sh-degree", "+2"], ["spz_merge", "a.spz", "-o", "b.spz", "--sh-degree", " 2"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--fractional-bits", "-0"], ["spz_merge", "a.spz", "-o", "b.spz", "--antialiased", "+1"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--sh-degree", "1", "--sh-degree", "2"],
    ["spz_merge", "a.spz", "-o", "b.spz", "--antialiased", "0", "--antialiased", "0"],
])
def test_cli_usage(argv, tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith("Usage: spz_merge <input.spz>... -o <output.spz>")
    assert not (tmp_path / "b.spz").exists() and not (tmp_path / "c.spz").exists()


def test_cli_unreadable_input_exits_1_without_output(tmp_path):
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_merge")
    r = subprocess.run([exe, "missing.spz", "-o", "b.spz"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert not (tmp_path / "b.spz").exists()
