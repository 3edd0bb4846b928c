"""A numpy restatement of the tile tree (include/spz_amd.h "tile", DESIGN §8 "Tile"): nodes, chain skipping,
content_level, ids, ranges, the arena layout, bounds and max_radius, written top-down from the sorted cell coordinates
(the device builds it bottom-up from one byte per point).  It does not restate the decimate: an interior tile's bounds
come from the bytes of a decimate output through content_bounds.  A helper module, not a test file:
tests/test_tile_host.py checks it against brute force and tests/test_gpu_tile.py compares the device with it."""
import math

import numpy as np

from decimate_ref import cell_u
from test_filter_host import SH_DIM, expected_stream, parse_stream
from test_sort_host import morton_order, position_fields

INT_FIELDS = ("id", "parent", "first_child", "child_count", "level", "cell", "range_begin", "range_end",
              "content_level", "num_points", "content_begin", "offset", "bytes")


def point_bytes(version, deg):
    return 16 + (4 if version >= 3 else 3) + 3 * SH_DIM[deg]


def radius_of_byte(b):
    """3 exp(scale) in f32 of a scale byte: exp in f64 of the f32 log scale, rounded to f32, times 3 in f32."""
    ls = np.float32(np.float32(b) / np.float32(16.0) - np.float32(10.0))
    return np.float32(3.0) * np.float32(math.exp(float(ls)))


def content_bounds(stream, begin, count):
    """(lo (3,) f32, hi (3,) f32, max_radius f32) of points begin .. begin + count of a v2/v3 stream."""
    if count == 0:
        nan = np.full(3, np.nan, np.float32)
        return nan, nan.copy(), np.float32(0.0)
    h = parse_stream(stream)
    f = position_fields(stream)[begin:begin + count].astype(np.int64)
    s = np.where(f >= 1 << 23, f - (1 << 24), f)
    scale = 2.0 ** -h["fractional_bits"]
    lo = (s.min(axis=0).astype(np.float64) * scale).astype(np.float32)
    hi = (s.max(axis=0).astype(np.float64) * scale).astype(np.float32)
    return lo, hi, radius_of_byte(int(h["sections"][3][begin:begin + count].max()))


def cell_index(us, level):
    """For sorted u (N, 3): the index of every point's level-`level` cell among the occupied ones."""
    flag = np.zeros(us.shape[0], np.int64)
    if us.shape[0] > 1:
        flag[1:] = np.any((us[1:] >> level) != (us[:-1] >> level), axis=1)
    return np.cumsum(flag)


def tile_tree(stream, cap):
    """(tiles, order, arena_bytes): the tiles in id order as dicts of the table's integer fields (children: the ids in Morton order),
    and the sort's order.  Leaves also carry their bounds; interior tiles get theirs from fill_interior_bounds."""
    h = parse_stream(stream)
    n, fb, version, deg = h["num_points"], h["fractional_bits"], h["version"], h["sh_degree"]
    assert version >= 2 and cap >= 1
    order = morton_order(stream)
    tiles = []

    def emit(level, cell, s, e, parent, leaf):
        t = dict(id=len(tiles), parent=parent, first_child=-1, child_count=0, level=level, cell=[int(c) for c in cell],
                 range_begin=s, range_end=e, content_level=-1, num_points=e - s, content_begin=s, children=[],
                 geometric_error=np.float32(0.0))
        tiles.append(t)
        if parent >= 0:
            tiles[parent]["children"].append(t["id"])
            tiles[parent]["child_count"] += 1
        return t

    if n == 0:
        emit(0, (0, 0, 0), 0, 0, -1, True)
    else:
        us = cell_u(stream)[order]
        seg = {l: cell_index(us, l) for l in range(25)}
        root = next(l for l in range(25) if seg[l][-1] == 0)

        def visit(level, s, e, parent):
            cell = us[s] >> level
            if e - s <= cap or level == 0:
                emit(level, cell, s, e, parent, True)
                return
            kid = seg[level - 1][s:e]
            cuts = [s] + (s + 1 + np.flatnonzero(kid[1:] != kid[:-1])).tolist() + [e]
            if len(cuts) == 2:                       # one occupied child: it takes this node's place
                visit(level - 1, s, e, parent)
                return
            t = emit(level, cell, s, e, parent, False)
            t["first_child"] = t["id"] + 1
            for l in range(level + 1):               # the smallest l with cells_l(node) <= cap
                cells = int(seg[l][e - 1] - seg[l][s]) + 1
                if cells <= cap:
                    t.update(content_level=l, num_points=cells, content_begin=int(seg[l][s]),
                             geometric_error=np.float32(2.0 ** (l - fb)))
                    break
            for a, b in zip(cuts[:-1], cuts[1:]):
                visit(level - 1, a, b, t["id"])

        visit(root, 0, n, -1)
    off = 0
    sorted_raw = expected_stream(stream, order) if n else bytes(stream)
    for t in tiles:
        t["bytes"] = 16 + t["num_points"] * point_bytes(version if t["content_level"] < 0 else 3, deg)
        t["offset"] = off
        off += (t["bytes"] + 15) & ~15
        if t["content_level"] < 0:
            t["box_min"], t["box_max"], t["max_radius"] = content_bounds(sorted_raw, t["content_begin"], t["num_points"])
    return tiles, order, off


def fill_interior_bounds(tiles, decimated):
    """Bounds of the interior tiles from `decimated`: {content_level: the decimate's stream at that level}."""
    for t in tiles:
        if t["content_level"] >= 0:
            t["box_min"], t["box_max"], t["max_radius"] = content_bounds(decimated[t["content_level"]], t["content_begin"],
                                                                         t["num_points"])


def content_stream(source, begin, count):
    """The stream of points begin .. begin + count of `source`: a tile's bytes."""
    return expected_stream(source, np.arange(begin, begin + count))


def leaf_stream(stream, order, t):
    return expected_stream(stream, order[t["range_begin"]:t["range_end"]])


# ---- the screen-space-error cut, float64 ---------------------------------------------------------------------------
def tile_sphere(t):
    lo, hi = np.asarray(t["box_min"], np.float64), np.asarray(t["box_max"], np.float64)
    return (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0 + float(t["max_radius"])


def select_tiles(tiles, eye, focal, max_pixel_error, near=0.2):
    """The ids of the cut: descend while sse = geometric_error * focal / max(|centre - eye| - radius, near) exceeds
    max_pixel_error and the tile has children; ids in tile order."""
    eye = np.asarray(eye, np.float64)
    out = []

    def visit(i):
        t = tiles[i]
        if t["children"]:
            c, r = tile_sphere(t)
            d = max(float(np.linalg.norm(c - eye)) - r, near)
            if float(t["geometric_error"]) * focal / d > max_pixel_error:
                for k in t["children"]:
                    visit(k)
                return
        out.append(i)

    visit(0)
    return sorted(out)
