"""spz_amd.device.tile_tree / tile_packed and spz_amd_tile_open (DESIGN §8 "Tile") on the GPU, all comparisons exact: the
tile table against the restatement of tests/tile_ref.py (every integer field; bounds and max_radius bit for bit), every
leaf's bytes against the sorted range, every interior tile's bytes against the index range of the device's own
decimate_packed at its content_level (the existing operation is the reference there, not the code under test), the
edge cases of the contract, the two forms and two runs against each other."""
import ctypes as C

import numpy as np
import pytest

from decimate_ref import level_counts
from test_decimate_host import duplicate_stream, with_fields
from test_filter_host import expected_stream, parse_stream
from test_gpu_decimate import cloud_stream, on_device
from test_sort_host import sortable_goldens, sorted_stream
from test_tile_host import check_tree, two_clusters
from tile_ref import INT_FIELDS, content_stream, fill_interior_bounds, leaf_stream, tile_tree

pytestmark = pytest.mark.gpu


def device_decimates(st, hdr, levels):
    from spz_amd import device as D
    return {l: D.decimate_packed(st, hdr, l)[0].cpu().numpy().tobytes() for l in levels}


def check_tileset(raw, cap, rows, tile_bytes, st, hdr):
    """Table and bytes of one device tileset against the restatement; returns the restated tiles."""
    want, order, arena_bytes = tile_tree(raw, cap)
    assert len(rows) == len(want), f"{len(rows)} tiles, the restatement has {len(want)}"
    levels = sorted({t["content_level"] for t in want if t["content_level"] >= 0})
    dec = device_decimates(st, hdr, levels)
    fill_interior_bounds(want, dec)
    for r, t in zip(rows, want):
        for k in INT_FIELDS:
            assert np.array_equal(np.asarray(r[k]).reshape(-1), np.asarray(t[k]).reshape(-1)), (t["id"], k, r[k], t[k])
        for k in ("box_min", "box_max", "max_radius", "geometric_error"):
            got = np.asarray(r[k], np.float32).reshape(-1).view(np.uint32)
            exp = np.asarray(t[k], np.float32).reshape(-1).view(np.uint32)
            assert np.array_equal(got, exp), (t["id"], k, r[k], t[k])
    srt = sorted_stream(raw, order) if len(order) else raw
    for t, b in zip(want, tile_bytes):
        if t["content_level"] < 0:
            assert b == (leaf_stream(raw, order, t) if len(order) else raw[:16]), f"leaf {t['id']}"
            assert b == content_stream(srt, t["range_begin"], t["num_points"])
        else:
            assert b == content_stream(dec[t["content_level"]], t["content_begin"], t["num_points"]), f"tile {t['id']}"
            assert parse_stream(b)["version"] == 3
    # the leaves' sections in tile order are the sorted stream's
    joined = [b"".join(parse_stream(b)["sections"][k].tobytes() for t, b in zip(want, tile_bytes) if t["content_level"] < 0)
              for k in range(6)]
    ws = parse_stream(srt)
    for k in range(6):
        assert joined[k] == ws["sections"][k].tobytes(), f"section {k}"
    check_tree(raw, cap, want, order, arena_bytes)
    return want


def run_device(raw, cap, max_tiles=65536, stream=None):
    from spz_amd import device as D
    st, hdr = on_device(raw)
    rows, tiles, arena = D.tile_packed(st, hdr, cap, max_tiles, stream=stream)
    return rows, [t.cpu().numpy().tobytes() for t in tiles], arena.cpu().numpy().tobytes(), st, hdr


def run_host_form(raw, cap, max_tiles=65536):
    import torch
    from spz_amd import abi
    L = abi.load_library()
    st, hdr = on_device(raw)
    ctx, tiles, arena = C.c_void_p(), C.c_uint64(), C.c_uint64()
    ms = (C.c_float * 4)()
    rc = L.spz_amd_tile_open(st.data_ptr(), st.numel(), C.byref(hdr), cap, max_tiles, torch.cuda.current_device(),
                             C.byref(ctx), C.byref(tiles), C.byref(arena), ms)
    if rc != 0:
        assert ctx.value is None and tiles.value == 0
        return rc, None, None, None
    try:
        table = np.zeros(tiles.value, np.dtype(abi.TileInfo))
        assert L.spz_amd_tile_table(ctx, table.ctypes.data) == 0
        whole = np.zeros(arena.value, np.uint8)
        assert L.spz_amd_tile_fetch_arena(ctx, whole.ctypes.data) == 0
        out = []
        for r in table:
            b = np.zeros(int(r["bytes"]), np.uint8)
            assert L.spz_amd_tile_fetch(ctx, int(r["id"]), b.ctypes.data) == 0
            assert L.spz_amd_tile_device_data(ctx, int(r["id"])) is not None
            out.append(b.tobytes())
        assert L.spz_amd_tile_fetch(ctx, tiles.value, whole.ctypes.data) == abi.ERR_INVALID_ARG
    finally:
        L.spz_amd_tile_close(ctx)
    return 0, table, out, whole.tobytes()


def caps_for(n):
    return sorted({1, 7, 64, 4096, max(n, 1), n + 1})


@pytest.mark.parametrize("name", ["v3_sh0", "v3_sh1", "v3_sh2", "v3_sh3", "v2", "fb8", "fb23"])
def test_goldens_every_cap(cuda, name):
    raw = sortable_goldens()[name]
    n = parse_stream(raw)["num_points"]
    for cap in caps_for(n):
        rows, tiles, arena, st, hdr = run_device(raw, cap)
        check_tileset(raw, cap, rows, tiles, st, hdr)
        if cap >= n:
            assert len(rows) == 1 and rows[0]["content_level"] == -1   # a single leaf root


@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("n,deg", [(63, 0), (64, 1), (65, 2), (1023, 0), (1025, 3), (2049, 1), (4097, 0), (20000, 3)])
def test_synthetic_clouds_at_wave_tile_and_cap_edges(cuda, oracle, clustered, n, deg):
    raw = cloud_stream(oracle, n, deg, n + 3, clustered)
    for cap in (1, 7, 64, 4096, n, n + 1):
        rows, tiles, arena, st, hdr = run_device(raw, cap, max_tiles=2 * n)
        check_tileset(raw, cap, rows, tiles, st, hdr)


def test_empty_one_point_piles_and_chains(cuda, oracle):
    for raw, cap in ((cloud_stream(oracle, 0, 2, 1), 5), (cloud_stream(oracle, 1, 3, 2), 1),
                     (cloud_stream(oracle, 1, 0, 2, antialiased=True), 9), (duplicate_stream(128, 200), 7),
                     (duplicate_stream(0, 65), 64), (two_clusters(), 5), (two_clusters(), 1), (two_clusters(), 29),
                     (two_clusters(), 30)):
        rows, tiles, arena, st, hdr = run_device(raw, cap)
        want = check_tileset(raw, cap, rows, tiles, st, hdr)
        rc, table, out, whole = run_host_form(raw, cap)
        assert rc == 0 and out == tiles and whole == arena and table.tobytes() == rows.tobytes()
        if parse_stream(raw)["num_points"] == 0:
            assert len(want) == 1 and tiles[0] == raw[:16] and np.isnan(rows[0]["box_min"]).all()
    rows, tiles, _, _, _ = run_device(duplicate_stream(128, 200), 7)
    assert len(rows) == 1 and rows[0]["level"] == 0 and rows[0]["num_points"] == 200   # the stated exception
    rows, tiles, _, _, _ = run_device(two_clusters(), 5)
    assert rows[0]["child_count"] == 2 and all(rows[k]["level"] <= 3 for k in range(1, len(rows)) if rows[k]["parent"] == 0)


def test_runs_boundaries_and_wide_levels(cuda, oracle):
    """Runs of equal and of nearby positions around 64-, 1024- and 2048-point edges; extremes of the lattice."""
    raw = cloud_stream(oracle, 6000, 1, 12)
    rng = np.random.default_rng(2)
    runs = rng.integers(1, 300, 200)
    ids = np.repeat(np.arange(runs.size), runs)[:6000]
    base = rng.integers(0, 1 << 24, (runs.size, 3))
    f = (base[ids] + rng.integers(0, 4, (ids.size, 3))) & 0xFFFFFF
    ext = np.array([0x000000, 0x7FFFFF, 0x800000, 0xFFFFFF, 0x7FFFFE, 0x800001], np.uint32)
    for fields in (f, ext[rng.integers(0, ext.size, (6000, 3))]):
        r = with_fields(raw, fields)
        for cap in (1, 3, 100, 1024, 5999):
            rows, tiles, arena, st, hdr = run_device(r, cap, max_tiles=12000)
            check_tileset(r, cap, rows, tiles, st, hdr)


def test_forms_runs_and_a_side_stream_agree(cuda, oracle):
    import torch
    raw = cloud_stream(oracle, 30000, 3, 8, clustered=True, antialiased=True)
    for cap in (64, 4096):
        rows, tiles, arena, st, hdr = run_device(raw, cap)
        rows2, tiles2, arena2, _, _ = run_device(raw, cap)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        rows3, tiles3, arena3, _, _ = run_device(raw, cap, stream=side)
        rc, table, out, whole = run_host_form(raw, cap)
        assert rc == 0
        assert arena == arena2 == arena3 == whole and tiles == tiles2 == tiles3 == out
        assert rows.tobytes() == rows2.tobytes() == rows3.tobytes() == table.tobytes()
        check_tileset(raw, cap, rows, tiles, st, hdr)
        for b in tiles:    # every tile is a stream the reader accepts, with the input's antialiased bit
            rc, full = oracle.unpack(np.frombuffer(b, np.uint8))
            assert rc == 0 and parse_stream(b)["flags"] == 1


def test_tree_alone_leaves_interior_boxes_empty(cuda, oracle):
    from spz_amd import device as D
    raw = cloud_stream(oracle, 5000, 1, 5)
    st, hdr = on_device(raw)
    table, summary = D.tile_tree(st, hdr, 64)
    s = D.tile_summary(summary)
    want, order, arena_bytes = tile_tree(raw, 64)
    assert s.ok == 1 and s.num_tiles == len(want) and s.arena_bytes == arena_bytes
    assert list(s.cells) == level_counts(raw).tolist()
    rows = D.tile_table_numpy(table, len(want))
    for r, t in zip(rows, want):
        for k in INT_FIELDS:
            assert np.array_equal(np.asarray(r[k]).reshape(-1), np.asarray(t[k]).reshape(-1)), (t["id"], k)
        if t["content_level"] < 0:
            assert np.array_equal(r["box_min"].view(np.uint32), t["box_min"].view(np.uint32))
            assert np.array_equal(r["box_max"].view(np.uint32), t["box_max"].view(np.uint32))
            assert r["max_radius"] == t["max_radius"]
        else:
            assert np.isnan(r["box_min"]).all() and np.isnan(r["box_max"]).all() and r["max_radius"] == 0


def test_version_1_and_the_tile_cap(cuda, oracle):
    from spz_amd import abi, device as D
    from test_filter_host import golden_streams
    v1 = golden_streams()["v1"]
    assert run_host_form(v1, 64)[0] == abi.ERR_UNSUPPORTED
    raw = cloud_stream(oracle, 5000, 0, 9)
    count = len(tile_tree(raw, 16)[0])
    assert run_host_form(raw, 16, count - 1)[0] == abi.ERR_CAPACITY
    rc, table, out, whole = run_host_form(raw, 16, count)
    assert rc == 0 and len(table) == count
    st, hdr = on_device(raw)
    with pytest.raises(abi.SpzAmdError) as e:
        D.tile_packed(st, hdr, 16, count - 1)
    assert e.value.status == abi.ERR_CAPACITY
    table_t, summary = D.tile_tree(st, hdr, 16, count - 1)
    s = D.tile_summary(summary)
    assert s.ok == 0 and s.num_tiles == count
    assert not table_t.any().item(), "the table is written although the tree does not fit"


def test_ten_million_points(cuda, oracle):
    """10 M clustered SH3 points, cap 65536: the partition and the table's invariants from the table alone, and the
    leaves' bytes against the device's own sorted stream."""
    import torch
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_clustered
    n, cap = 10_000_000, 65536
    raw = oracle.pack(make_cloud_clustered(n, 3, 21), n, 3, False, 0).tobytes()
    st, hdr = on_device(raw)
    rows, tiles, arena = D.tile_packed(st, hdr, cap)
    leaves = rows[rows["content_level"] < 0]
    inner = rows[rows["content_level"] >= 0]
    assert len(rows) <= 2 * len(leaves) - 1 and np.array_equal(rows["id"], np.arange(len(rows)))
    assert leaves["range_begin"][0] == 0 and leaves["range_end"][-1] == n
    assert np.array_equal(leaves["range_begin"][1:], leaves["range_end"][:-1])
    assert np.all((leaves["num_points"] <= cap) | (leaves["level"] == 0))
    assert np.all(leaves["num_points"] == leaves["range_end"] - leaves["range_begin"])
    assert np.all(inner["num_points"] <= cap) and np.all(inner["range_end"] - inner["range_begin"] > cap)
    assert np.all(inner["child_count"] >= 2) and rows["child_count"].sum() == len(rows) - 1
    par = rows["parent"][1:]
    assert rows["parent"][0] == -1 and np.all(par >= 0) and np.all(par < rows["id"][1:])
    assert np.all(rows["level"][1:] < rows["level"][par]) and np.all(rows["content_level"][1:] <= rows["content_level"][par])
    assert np.all(rows["range_begin"][1:] >= rows["range_begin"][par]) and np.all(rows["range_end"][1:] <= rows["range_end"][par])
    assert np.all(rows["box_min"] <= rows["box_max"]) and np.all(rows["max_radius"] > 0)
    assert np.all(rows["offset"] % 16 == 0) and np.all(rows["offset"][1:] >= rows["offset"][:-1] + rows["bytes"][:-1])
    srt = D.subset(st, hdr, D.morton_order(st, hdr))
    lay = [16]
    for b in (9, 1, 3, 3, 4, 45):
        lay.append(lay[-1] + b * n)
    for k, b in enumerate((9, 1, 3, 3, 4, 45)):   # the leaves' sections, concatenated on the device
        parts = []
        for r, t in zip(rows, tiles):
            if r["content_level"] < 0:
                m = int(r["num_points"])
                o = 16 + sum(w * m for w in (9, 1, 3, 3, 4, 45)[:k])
                parts.append(t[o:o + b * m])
        assert torch.equal(torch.cat(parts), srt[lay[k]:lay[k + 1]]), f"section {k}"


def gz(b):
    import zlib
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def test_files_python_and_cli_give_the_device_forms_bytes(cuda, oracle, tmp_path):
    """tile_spz and spz_tile: every written file is zlib's member of the arena's bytes, tileset.json holds the table, the
    leaf files merged in tile order are sort_spz's bytes, and a refused tree writes nothing."""
    import os
    import subprocess
    import zlib
    import spz_amd.spz as spz
    from conftest import ROOT
    raw = cloud_stream(oracle, 9000, 2, 17, clustered=True)
    src = tmp_path / "in.spz"
    src.write_bytes(gz(raw))
    cap = 256
    rows, tiles, arena, st, hdr = run_device(raw, cap)
    want = check_tileset(raw, cap, rows, tiles, st, hdr)
    ts = spz.tile_spz(str(src), str(tmp_path / "py"), max_points=cap)
    exe = os.path.join(ROOT, "spz_amd", "bin", "spz_tile")
    r = subprocess.run([exe, "in.spz", "cli", "--max-points", str(cap)], capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr
    assert spz.load_tileset(str(tmp_path / "py" / "tileset.json")) == spz.load_tileset(str(tmp_path / "cli" / "tileset.json"))
    back = spz.load_tileset(str(tmp_path / "py" / "tileset.json"))
    assert len(ts["tiles"]) == len(rows) == len(back["tiles"])
    assert sorted(os.listdir(tmp_path / "py")) == sorted(["tileset.json"] + [t["file"] for t in ts["tiles"]])
    for t, b, r_, w in zip(back["tiles"], tiles, rows, want):
        for d in ("py", "cli"):
            member = (tmp_path / d / t["file"]).read_bytes()
            assert member == gz(b), t["file"]                     # zlib's bytes of the arena's stream
            assert zlib.decompress(member, 31) == b
        assert t["file"] == "tile_%06d.spz" % t["id"] and t["children"] == w["children"]
        assert (t["id"], t["parent"], t["level"], t["content_level"], t["num_points"]) == (
            w["id"], w["parent"], w["level"], w["content_level"], w["num_points"])
        assert tuple(t["cell"]) == tuple(w["cell"])
        assert np.array_equal(np.array(t["box"], np.float32).view(np.uint32),
                              np.stack([r_["box_min"], r_["box_max"]]).view(np.uint32))
        assert np.float32(t["max_radius"]) == r_["max_radius"] and np.float32(t["geometric_error"]) == r_["geometric_error"]
        cloud = spz.load_spz(str(tmp_path / "py" / t["file"]))      # every file loads
        assert cloud.num_points == t["num_points"]
    # the leaves merged in tile order are the sorted file
    leaves = [str(tmp_path / "py" / t["file"]) for t in back["tiles"] if t["content_level"] < 0]
    spz.merge_spz(leaves, str(tmp_path / "merged.spz"))
    spz.sort_spz(str(src), str(tmp_path / "sorted.spz"))
    assert (tmp_path / "merged.spz").read_bytes() == (tmp_path / "sorted.spz").read_bytes()
    assert spz.select_tiles(back, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 5], 500.0, 500.0, 0.0) == [
        t["id"] for t in back["tiles"] if t["content_level"] < 0]
    # the error-0 cut: its files merged and rendered equal the render of the sort_spz copy bit for bit
    views = spz.orbit_views(2, width=160, height=96, fov_y=50.0, scene=str(src), coord=spz.RUB)
    v = views[0]
    cut = spz.select_tiles(back, v["world_to_camera"], v["fx"], v["fy"], 0.0)
    assert cut == [t["id"] for t in back["tiles"] if t["content_level"] < 0]
    spz.merge_spz([str(tmp_path / "py" / back["tiles"][i]["file"]) for i in cut], str(tmp_path / "cut0.spz"))
    assert (tmp_path / "cut0.spz").read_bytes() == (tmp_path / "sorted.spz").read_bytes()
    for v in views:
        a = spz.render_spz(str(tmp_path / "cut0.spz"), **dict(v, coord=spz.RUB))
        b = spz.render_spz(str(tmp_path / "sorted.spz"), **dict(v, coord=spz.RUB))
        assert a.shape == (96, 160, 4) and a[..., 3].max() > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a coarser cut is still a cut: one ancestor-or-self per leaf, fewer points, and it merges and renders
    coarse = spz.select_tiles(back, v["world_to_camera"], v["fx"], v["fy"], 4.0)
    covered = sum(want[i]["range_end"] - want[i]["range_begin"] for i in coarse)
    assert covered == 9000 and sum(back["tiles"][i]["num_points"] for i in coarse) <= 9000
    spz.merge_spz([str(tmp_path / "py" / back["tiles"][i]["file"]) for i in coarse], str(tmp_path / "cut4.spz"))
    assert spz.load_spz(str(tmp_path / "cut4.spz")).num_points == sum(back["tiles"][i]["num_points"] for i in coarse)
    # coord flips the boxes only
    flipped = spz.tile_spz(str(src), str(tmp_path / "rdf"), max_points=cap, coord=spz.CoordinateSystem.RDF)
    for a, b in zip(flipped["tiles"], back["tiles"]):
        lo, hi = np.array(b["box"], np.float32)
        assert np.array_equal(np.array(a["box"], np.float32), np.array([[lo[0], -hi[1], -hi[2]], [hi[0], -lo[1], -lo[2]]], np.float32))
        assert (tmp_path / "rdf" / a["file"]).read_bytes() == (tmp_path / "py" / b["file"]).read_bytes()
    # a tree above max_tiles: no directory, no file
    with pytest.raises(Exception):
        spz.tile_spz(str(src), str(tmp_path / "none"), max_points=cap, max_tiles=len(rows) - 1)
    assert not (tmp_path / "none").exists()
    r = subprocess.run([exe, "in.spz", "none", "--max-points", str(cap), "--max-tiles", str(len(rows) - 1)],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 1 and not (tmp_path / "none").exists()
