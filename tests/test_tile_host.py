"""The tile tree (DESIGN §8 "Tile") without a GPU: the restatement of tests/tile_ref.py against brute force (every tile's
points and cells_l recounted from the raw cell coordinates, the leaves a partition, the contract's invariants), the
screen-space-error cut on hand-built tilesets, the workspace sizes and the argument checks of the C ABI and of
spz_amd.device (which must fail before any device work).  tests/test_gpu_tile.py compares the device with the
restatement."""
import ctypes as C

import numpy as np
import pytest

from decimate_ref import cell_u, decimate
from test_decimate_host import fields_cases, with_fields
from test_filter_host import SH_DIM, parse_stream
from test_sort_host import sortable_goldens, sorted_stream
from tile_ref import (content_bounds, content_stream, fill_interior_bounds, leaf_stream, point_bytes, radius_of_byte,
                      select_tiles, tile_tree)


def check_tree(raw, cap, tiles, order, arena_bytes):
    """Brute force over the raw u, and the invariants the contract states."""
    h = parse_stream(raw)
    n = h["num_points"]
    u = cell_u(raw)
    leaves = [t for t in tiles if t["content_level"] < 0]
    interior = [t for t in tiles if t["content_level"] >= 0]
    assert len(tiles) <= max(1, 2 * len(leaves) - 1)
    assert [t["id"] for t in tiles] == list(range(len(tiles)))
    # pre-order: ascending range start, the larger level first
    keys = [(t["range_begin"], -t["level"]) for t in tiles]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # the leaves partition 0..n in id order
    at = 0
    for t in leaves:
        assert t["range_begin"] == at and t["first_child"] == -1 and t["child_count"] == 0
        at = t["range_end"]
    assert at == n
    if n == 0:
        assert len(tiles) == 1 and tiles[0]["bytes"] == 16
        return
    for t in tiles:
        L, cell = t["level"], np.array(t["cell"])
        inside = np.all((u >> L) == cell, axis=1)
        members = np.flatnonzero(inside)
        assert members.size == t["range_end"] - t["range_begin"] > 0
        assert sorted(order[t["range_begin"]:t["range_end"]].tolist()) == members.tolist()
        if t["content_level"] < 0:
            assert members.size <= cap or L == 0
            assert t["num_points"] == members.size and t["content_begin"] == t["range_begin"]
        else:
            assert members.size > cap and L > 0 and t["child_count"] >= 2
            cells = [np.unique(u[members] >> l, axis=0).shape[0] for l in range(L + 1)]
            l = t["content_level"]
            assert 0 <= l <= L and t["num_points"] == cells[l] <= cap
            assert l == 0 or cells[l - 1] > cap
            # the content's place in the decimate's output: the occupied level-l cells before the node's first point
            first = order[t["range_begin"]]
            before = np.unique(u[order[:t["range_begin"]]] >> l, axis=0).shape[0] if t["range_begin"] else 0
            assert t["content_begin"] == before, (t, first)
            kids = [tiles[k] for k in t["children"]]
            assert t["first_child"] == t["id"] + 1 == kids[0]["id"] and len(kids) == t["child_count"]
            assert kids[0]["range_begin"] == t["range_begin"] and kids[-1]["range_end"] == t["range_end"]
            for a, b in zip(kids, kids[1:]):
                assert a["range_end"] == b["range_begin"]
            for k in kids:
                assert k["parent"] == t["id"] and k["level"] < L
                assert k["content_level"] <= l
                # the child's cell lies in the parent's, and every cell between them holds the child's points only
                assert np.all((np.array(k["cell"]) >> (L - k["level"])) == cell)
        assert t["offset"] % 16 == 0 and t["bytes"] == 16 + t["num_points"] * point_bytes(
            h["version"] if t["content_level"] < 0 else 3, h["sh_degree"])
    assert tiles[0]["parent"] == -1 and all(t["parent"] >= 0 for t in tiles[1:])
    assert arena_bytes == tiles[-1]["offset"] + ((tiles[-1]["bytes"] + 15) & ~15)


CAPS = [1, 7, 64, 4096]


@pytest.mark.parametrize("name", sorted(sortable_goldens()))
def test_restatement_on_goldens_against_brute_force(name):
    raw = sortable_goldens()[name]
    n = parse_stream(raw)["num_points"]
    for cap in CAPS + [max(n, 1), n + 1]:
        tiles, order, arena = tile_tree(raw, cap)
        check_tree(raw, cap, tiles, order, arena)
        if cap >= n:
            assert len(tiles) == 1 and tiles[0]["content_level"] == -1


@pytest.mark.parametrize("case", sorted(fields_cases()))
def test_restatement_on_seeded_clouds_against_brute_force(case):
    raw = with_fields(sortable_goldens()["v3_sh1"], fields_cases()[case])
    for cap in (1, 3, 7, 50):
        tiles, order, arena = tile_tree(raw, cap)
        check_tree(raw, cap, tiles, order, arena)


def two_clusters(n=60):
    """Two tight clusters far apart: chains of single-child cells between the root and each cluster."""
    rng = np.random.default_rng(5)
    f = np.where(np.arange(n)[:, None] < n // 2, 0x100000, 0xE00000) + rng.integers(0, 8, (n, 3))
    base = sortable_goldens()["v3_sh1"]
    assert parse_stream(base)["num_points"] >= n
    from test_filter_host import expected_stream
    return with_fields(expected_stream(base, np.arange(n)), f.astype(np.uint32))


def test_chains_are_skipped_and_piles_are_leaves_above_the_cap():
    raw = two_clusters()
    tiles, order, arena = tile_tree(raw, 5)
    check_tree(raw, 5, tiles, order, arena)
    root = tiles[0]
    assert root["child_count"] == 2 and root["level"] == 24
    for k in root["children"]:
        assert tiles[k]["level"] <= 3          # the child took the place of ~20 single-child cells
    pile = with_fields(raw, np.full((60, 3), 0x123456, np.uint32))
    tiles, order, arena = tile_tree(pile, 7)
    assert len(tiles) == 1 and tiles[0]["level"] == 0 and tiles[0]["num_points"] == 60 > 7
    check_tree(pile, 7, tiles, order, arena)


def test_interior_bounds_come_from_the_decimate_and_leaf_bytes_from_the_sort(oracle):
    raw = sortable_goldens()["v3_sh2"]
    tiles, order, _ = tile_tree(raw, 7)
    levels = sorted({t["content_level"] for t in tiles if t["content_level"] >= 0})
    assert levels
    dec = {l: decimate(oracle, raw, l)[0] for l in levels}
    fill_interior_bounds(tiles, dec)
    srt = sorted_stream(raw, order)
    joined = [b"" for _ in range(6)]
    for t in tiles:
        assert np.all(t["box_min"] <= t["box_max"]) and t["max_radius"] > 0
        if t["content_level"] < 0:
            got = parse_stream(leaf_stream(raw, order, t))
            assert leaf_stream(raw, order, t) == content_stream(srt, t["range_begin"], t["num_points"])
            for k in range(6):
                joined[k] += got["sections"][k].tobytes()
        else:
            assert parse_stream(dec[t["content_level"]])["num_points"] >= t["content_begin"] + t["num_points"]
            for k in t["children"]:   # a coarse tile's box lies in its cell, so its children's boxes overlap it
                assert np.all(tiles[k]["box_min"] <= t["box_max"] + 2.0 ** (t["level"] - 12))
    want = parse_stream(srt)
    for k in range(6):
        assert joined[k] == want["sections"][k].tobytes()
    assert radius_of_byte(160) == np.float32(3.0) and radius_of_byte(0) == np.float32(3.0) * np.float32(np.exp(-10.0))
    lo, hi, r = content_bounds(raw, 0, 0)
    assert np.isnan(lo).all() and np.isnan(hi).all() and r == 0


# ---- the cut -----------------------------------------------------------------------------------------------------
def hand_tileset(depth=3):
    """A full octree of `depth` levels over [0, 8)^3: geometric_error halves per level, leaves 0."""
    tiles = []

    def add(lo, edge, level, parent):
        t = dict(id=len(tiles), parent=parent, children=[], box_min=np.array(lo, np.float32),
                 box_max=np.array(lo, np.float32) + np.float32(edge), max_radius=np.float32(0.05),
                 geometric_error=np.float32(edge / 4 if level else 0.0))
        tiles.append(t)
        if parent >= 0:
            tiles[parent]["children"].append(t["id"])
        if level:
            h = edge / 2
            for z in (0, 1):
                for y in (0, 1):
                    for x in (0, 1):
                        add([lo[0] + x * h, lo[1] + y * h, lo[2] + z * h], h, level - 1, t["id"])

    add([0.0, 0.0, 0.0], 8.0, depth, -1)
    return tiles


def ancestors_or_self(tiles, i):
    out = []
    while i >= 0:
        out.append(i)
        i = tiles[i]["parent"]
    return out


def test_select_tiles_on_a_hand_built_tileset():
    tiles = hand_tileset()
    leaves = [t["id"] for t in tiles if not t["children"]]
    assert select_tiles(tiles, [100, 100, 100], 1000.0, 0.0) == leaves
    assert select_tiles(tiles, [4, 4, 4], 1000.0, 1e12) == [0]
    # a camera next to one corner refines only there
    cut = select_tiles(tiles, [-0.5, -0.5, -0.5], 500.0, 120.0)
    assert 0 not in cut and any(not tiles[i]["children"] for i in cut) and any(tiles[i]["children"] for i in cut)
    fine = [i for i in cut if not tiles[i]["children"]]
    coarse = [i for i in cut if tiles[i]["children"]]
    far = lambda i: float(np.linalg.norm((tiles[i]["box_min"] + tiles[i]["box_max"]) / 2 + 0.5))
    assert max(far(i) for i in fine) < max(far(i) for i in coarse)
    rng = np.random.default_rng(8)
    for _ in range(50):
        eye = rng.uniform(-20, 28, 3)
        err = float(rng.choice([0.0, 1.0, 8.0, 64.0, 512.0]))
        cut = select_tiles(tiles, eye, 800.0, err)
        assert cut == sorted(set(cut))
        for leaf in leaves:   # exactly one ancestor-or-self of every leaf is in the cut
            assert len(set(ancestors_or_self(tiles, leaf)) & set(cut)) == 1


def test_select_tiles_on_a_restated_tree(oracle):
    raw = sortable_goldens()["v3_sh1"]
    tiles, order, _ = tile_tree(raw, 7)
    levels = sorted({t["content_level"] for t in tiles if t["content_level"] >= 0})
    fill_interior_bounds(tiles, {l: decimate(oracle, raw, l)[0] for l in levels})
    leaves = [t["id"] for t in tiles if not t["children"]]
    assert select_tiles(tiles, [0, 0, 50], 600.0, 0.0) == leaves
    assert select_tiles(tiles, [0, 0, 50], 600.0, 1e30) == [0]
    for err in (0.5, 4.0, 32.0):
        cut = select_tiles(tiles, [0.3, -0.2, 3.0], 600.0, err)
        for leaf in leaves:
            assert len(set(ancestors_or_self(tiles, leaf)) & set(cut)) == 1
        assert sum(tiles[i]["range_end"] - tiles[i]["range_begin"] for i in cut) == parse_stream(raw)["num_points"]


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from spz_amd import abi
    return abi.load_library()


def test_table_row_layout_matches_the_header(lib):
    from spz_amd import abi
    assert C.sizeof(abi.TileInfo) == 104 and abi.TileInfo.offset.offset == 56 and abi.TileInfo.box_min.offset == 72
    assert C.sizeof(abi.TileSummary) == 224


def test_workspace_bytes_is_host_only_and_monotone(lib):
    sizes = [0, 1, 63, 64, 65, 4095, 4096, 4097, 1 << 20, 10_000_000]
    for deg in range(4):
        ws = [int(lib.spz_amd_tile_workspace_bytes(n, deg, 65536)) for n in sizes]
        assert ws[0] > 0 and all(a <= b for a, b in zip(ws, ws[1:]))
        for n, w in zip(sizes[1:], ws[1:]):
            assert w >= int(lib.spz_amd_sort_workspace_bytes(n)) + (16 + (20 + 3 * SH_DIM[deg]) * n) + 13 * n
    assert lib.spz_amd_tile_workspace_bytes(1000, 3, 65536) > lib.spz_amd_tile_workspace_bytes(1000, 0, 65536)
    assert lib.spz_amd_tile_workspace_bytes(10 ** 6, 0, 10 ** 6) > lib.spz_amd_tile_workspace_bytes(10 ** 6, 0, 10)
    assert lib.spz_amd_tile_content_workspace_bytes(100) >= 404


def test_entry_points_reject_bad_arguments_without_launching(lib):
    from spz_amd import abi
    raw = bytearray(sortable_goldens()["v3_sh1"])
    n = parse_stream(bytes(raw))["num_points"]
    buf = (C.c_uint8 * len(raw)).from_buffer(raw)
    p = C.addressof(buf)
    hdr = abi.peek_header(bytes(raw))[1]
    dummy = (C.c_uint8 * 256)()
    d = C.addressof(dummy)
    v1 = abi.Header(1, n, hdr.sh_degree, 12, 0, 0)
    bad = abi.Header(4, n, hdr.sh_degree, 12, 0, 0)
    big = abi.Header(3, abi.REFERENCE_MAX_POINTS + 1, 0, 12, 0, 0)
    big_size = abi.stream_layout(big.num_points, 0, 3).total_bytes
    tt = lib.spz_amd_tile_tree_device
    assert tt(None, len(raw), C.byref(hdr), 64, 100, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), None, 64, 100, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw) - 1, C.byref(hdr), 64, 100, d, d, d, None) == abi.ERR_SHORT_STREAM
    assert tt(p, len(raw), C.byref(v1), 64, 100, d, d, d, None) == abi.ERR_UNSUPPORTED
    assert tt(p, len(raw), C.byref(bad), 64, 100, d, d, d, None) == abi.ERR_VERSION
    assert tt(p, big_size, C.byref(big), 64, 100, d, d, d, None) == abi.ERR_TOO_MANY_POINTS
    assert tt(p, len(raw), C.byref(hdr), 0, 100, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), abi.REFERENCE_MAX_POINTS + 1, 100, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), 64, 0, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), 64, 2 ** 31, d, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), 64, 100, None, d, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), 64, 100, d, None, d, None) == abi.ERR_INVALID_ARG
    assert tt(p, len(raw), C.byref(hdr), 64, 100, d, d, None, None) == abi.ERR_INVALID_ARG
    tc = lib.spz_amd_tile_content_device
    assert tc(None, 1, -1, p, len(raw), d, 256, d, None) == abi.ERR_INVALID_ARG
    assert tc(d, 0, -1, p, len(raw), d, 256, d, None) == abi.ERR_INVALID_ARG
    assert tc(d, 1, -2, p, len(raw), d, 256, d, None) == abi.ERR_INVALID_ARG
    assert tc(d, 1, 25, p, len(raw), d, 256, d, None) == abi.ERR_INVALID_ARG
    assert tc(d, 1, 3, None, len(raw), d, 256, d, None) == abi.ERR_INVALID_ARG
    assert tc(d, 1, 3, p, 15, d, 256, d, None) == abi.ERR_SHORT_STREAM
    assert tc(d, 1, 3, p, len(raw), d, 256, None, None) == abi.ERR_INVALID_ARG
    ctx, tiles, arena = C.c_void_p(), C.c_uint64(), C.c_uint64()
    op = lib.spz_amd_tile_open

    def o(h, cap, max_tiles, size=len(raw)):
        return op(p, size, C.byref(h), cap, max_tiles, 0, C.byref(ctx), C.byref(tiles), C.byref(arena), None)

    assert o(hdr, 0, 100) == abi.ERR_INVALID_ARG
    assert o(hdr, abi.REFERENCE_MAX_POINTS + 1, 100) == abi.ERR_INVALID_ARG
    assert o(hdr, 64, 0) == abi.ERR_INVALID_ARG
    assert o(v1, 64, 100) == abi.ERR_UNSUPPORTED
    assert o(hdr, 64, 100, len(raw) - 1) == abi.ERR_SHORT_STREAM
    assert o(big, 64, 100, big_size) == abi.ERR_TOO_MANY_POINTS
    assert op(p, len(raw), C.byref(hdr), 64, 100, 0, None, C.byref(tiles), C.byref(arena), None) == abi.ERR_INVALID_ARG
    assert ctx.value is None and tiles.value == 0 and arena.value == 0
    assert lib.spz_amd_tile_table(None, d) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_tile_fetch(None, 0, d) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_tile_fetch_arena(None, d) == abi.ERR_INVALID_ARG
    assert lib.spz_amd_tile_device_data(None, 0) is None
    lib.spz_amd_tile_close(None)


def test_device_tile_functions_check_their_arguments():
    torch = pytest.importorskip("torch")
    from spz_amd import device as D
    hdr = D.make_header(10, 2)
    st = torch.zeros(16, dtype=torch.uint8)
    for f in (D.tile_tree, D.tile_packed):
        with pytest.raises(ValueError):
            f(st, hdr, 64)                                   # not a CUDA tensor
        with pytest.raises(ValueError):
            f(st, D.make_header(10, 2, version=1), 64)
        for bad in (0, -1, 2.0, True, 10_000_001):
            with pytest.raises(ValueError):
                f(st, hdr, bad)
        for bad in (0, 2 ** 31, 1.5, False):
            with pytest.raises(ValueError):
                f(st, hdr, 64, max_tiles=bad)


# ---- the file layer without a GPU: tileset.json, the C++ cut, argument checks, the CLI ------------------------------
@pytest.fixture(scope="module")
def spz():
    import spz_amd.spz as m
    return m


def to_dict(spz, tiles, coord=None):
    """A restated / hand-built tile list as the dict spz.load_tileset returns."""
    out = []
    for t in tiles:
        out.append(dict(id=t["id"], file="tile_%06d.spz" % t["id"], parent=t["parent"], children=list(t["children"]),
                        level=t.get("level", 0), cell=tuple(t.get("cell", (0, 0, 0))),
                        content_level=t.get("content_level", -1 if not t["children"] else 0),
                        num_points=t.get("num_points", 1), geometric_error=float(t["geometric_error"]),
                        box=(tuple(float(v) for v in t["box_min"]), tuple(float(v) for v in t["box_max"])),
                        max_radius=float(t["max_radius"])))
    return dict(format="spz-tileset", version=1, coord=coord or spz.CoordinateSystem.RUB, num_points=123,
                sh_degree=2, fractional_bits=12, max_points=7, tiles=out)


def test_tileset_json_round_trip_through_the_host_library(spz, oracle, tmp_path):
    import json
    raw = sortable_goldens()["v3_sh1"]
    tiles, order, _ = tile_tree(raw, 7)
    levels = sorted({t["content_level"] for t in tiles if t["content_level"] >= 0})
    fill_interior_bounds(tiles, {l: decimate(oracle, raw, l)[0] for l in levels})
    d = to_dict(spz, tiles, spz.CoordinateSystem.RDF)
    d["tiles"][-1]["box"] = ((float("nan"),) * 3, (float("nan"),) * 3)     # a tile without points
    d["tiles"][1]["geometric_error"] = float(np.float32(1.0) / np.float32(3.0))
    path = str(tmp_path / "tileset.json")
    spz.save_tileset(d, path)
    back = spz.load_tileset(path)
    for k in ("format", "version", "coord", "num_points", "sh_degree", "fractional_bits", "max_points"):
        assert back[k] == d[k], k
    assert len(back["tiles"]) == len(d["tiles"])
    for a, b in zip(back["tiles"], d["tiles"]):
        for k in ("id", "file", "parent", "children", "level", "cell", "content_level", "num_points"):
            assert a[k] == b[k], k
        for k in ("geometric_error", "max_radius"):    # the same f32
            assert np.float32(a[k]).view(np.uint32) == np.float32(b[k]).view(np.uint32), k
        assert np.array_equal(np.array(a["box"], np.float32).view(np.uint32), np.array(b["box"], np.float32).view(np.uint32))
    js = json.loads(open(path).read().replace("null", "NaN"))
    assert js["format"] == "spz-tileset" and js["version"] == 1 and js["coord"] == "RDF"
    assert set(js["tiles"][0]) == {"id", "file", "parent", "children", "level", "cell", "content_level", "num_points",
                                   "geometric_error", "box", "max_radius"}
    (tmp_path / "bad.json").write_text('{"format": "other", "version": 1}')
    with pytest.raises(ValueError):
        spz.load_tileset(str(tmp_path / "bad.json"))
    with pytest.raises(ValueError):
        spz.load_tileset(str(tmp_path / "missing.json"))


def camera_at(eye):
    """[I | -eye]: a camera at `eye` looking down +z."""
    return [1, 0, 0, -eye[0], 0, 1, 0, -eye[1], 0, 0, 1, -eye[2]]


def test_cpp_select_tiles_equals_the_float64_restatement(spz):
    tiles = hand_tileset()
    d = to_dict(spz, tiles)
    leaves = [t["id"] for t in tiles if not t["children"]]
    assert spz.select_tiles(d, camera_at([100, 100, 100]), 1000.0, 1000.0, 0.0) == leaves
    assert spz.select_tiles(d, camera_at([4, 4, 4]), 1000.0, 1000.0, 1e12) == [0]
    rng = np.random.default_rng(8)
    for _ in range(60):
        eye = [float(np.float32(v)) for v in rng.uniform(-20, 28, 3)]
        err = float(rng.choice([0.0, 1.0, 8.0, 64.0, 512.0]))
        fx, fy = float(rng.choice([500.0, 800.0])), float(rng.choice([400.0, 900.0]))
        got = spz.select_tiles(d, camera_at(eye), fx, fy, err, 0.2)
        assert got == select_tiles(tiles, eye, max(fx, fy), err, 0.2)
        for leaf in leaves:
            assert len(set(ancestors_or_self(tiles, leaf)) & set(got)) == 1
    with pytest.raises(ValueError):
        spz.select_tiles(d, [1, 0, 0], 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        spz.select_tiles(d, camera_at([0, 0, 0]), 1.0, 1.0, -1.0)
    with pytest.raises(ValueError):
        spz.select_tiles(dict(tiles=[]), camera_at([0, 0, 0]), 1.0, 1.0, 1.0)


@pytest.mark.parametrize("kw", [
    dict(), dict(max_points=0), dict(max_points=-3), dict(max_points=10_000_001), dict(max_points=2.0),
    dict(max_points=True), dict(max_points=64, max_tiles=0), dict(max_points=64, max_tiles=2 ** 31),
    dict(max_points=64, max_tiles=1.5),
], ids=lambda kw: ",".join(f"{k}={v!r}" for k, v in kw.items()) or "none")
def test_tile_spz_bad_arguments_raise_before_device_work(spz, tmp_path, kw):
    src = tmp_path / "in.spz"
    src.write_bytes(b"not read: the arguments are checked first")
    with pytest.raises((ValueError, TypeError)):
        spz.tile_spz(str(src), str(tmp_path / "out"), **kw)
    assert not (tmp_path / "out").exists()


def test_tile_spz_refuses_a_used_output_directory_before_reading(spz, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    (out / "keep.txt").write_text("x")
    with pytest.raises(Exception):
        spz.tile_spz(str(tmp_path / "missing.spz"), str(out), max_points=64)
    assert sorted(p.name for p in out.iterdir()) == ["keep.txt"]
    f = tmp_path / "file"
    f.write_text("x")
    with pytest.raises(Exception):
        spz.tile_spz(str(tmp_path / "missing.spz"), str(f), max_points=64)


TILE_USAGE = "Usage: spz_tile <input.spz> <outdir> --max-points <N> [--max-tiles <M>] [--coord "


@pytest.mark.parametrize("argv", [
    ["spz_tile"], ["spz_tile", "a.spz", "out"], ["spz_tool", "spz_tile", "a.spz"],
    ["spz_tile", "a.spz", "out", "--max-points"], ["spz_tile", "a.spz", "out", "--max-points", "0"],
    ["spz_tile", "a.spz", "out", "--max-points", "10000001"], ["spz_tile", "a.spz", "out", "--max-points", "1e3"],
    ["spz_tile", "a.spz", "out", "--max-points", "64", "--max-tiles", "0"],
    ["spz_tile", "a.spz", "out", "--max-points", "64", "--coord", "XYZ"],
    ["spz_tile", "a.spz", "out", "--max-points", "64", "--max-points", "65"],
    ["spz_tile", "a.spz", "out", "--max-tiles", "5"], ["spz_tile", "a.spz", "out", "--bogus", "3"],
    ["spz_tile", "--max-points", "64", "a.spz", "out"],
])
def test_cli_usage(argv, tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "spz_amd", "bin", argv[0])
    r = subprocess.run([exe] + argv[1:], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1
    assert r.stderr.startswith(TILE_USAGE)
    assert not (tmp_path / "out").exists()


def test_spz_tool_lists_the_tile_tool_and_a_missing_input_writes_nothing(tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tool")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "spz_tile" in r.stderr
    r = subprocess.run([os.path.join(ROOT, "spz_amd", "bin", "spz_tile"), "missing.spz", "out", "--max-points", "64"],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode == 1 and not (tmp_path / "out").exists()
