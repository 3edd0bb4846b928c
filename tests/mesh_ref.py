"""A numpy restatement of the mesh contract (include/spz_amd.h "mesh"): the fuse of one view into a TSDF grid and the
marching-tetrahedra extraction, with the operation order of the contract.  Stored sums are float32; the projection and
the interpolation are float64, every operation rounded on its own (numpy does not contract)."""
import itertools

import numpy as np

TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MEDIAN, EXPECTED = 0, 1


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


def tet_corners():
    """(6, 4): the cube corners (x + 2 y + 4 z) of the six Kuhn tetrahedra, permutations in lexicographic order."""
    out = []
    for p in itertools.permutations(range(3)):
        v1 = 1 << p[0]
        out.append((0, v1, v1 | (1 << p[1]), 7))
    return np.array(out, dtype=np.uint8)


def tet_table():
    """corners (6, 4), num_triangles (6, 16), edges (6, 16, 6) generated from the rule: mask bit v = tet vertex v
    inside; a lone vertex gives its three edges in ascending number; {0, j} | {k, l} the quad (0k, 0l, jl, jk) as two
    triangles; the last two indices swapped so that the normal (edge midpoints as positions) points from the inside
    centroid to the outside centroid."""
    corners = tet_corners()
    ntri = np.zeros((6, 16), np.uint8)
    edges = np.zeros((6, 16, 6), np.uint8)
    eid = {pair: q for q, pair in enumerate(TET_EDGES)}
    for t in range(6):
        pos = np.array([corner_xyz(int(c)) for c in corners[t]], dtype=np.float64)
        mid = [(pos[a] + pos[b]) / 2 for a, b in TET_EDGES]
        for m in range(1, 15):
            inside = [v for v in range(4) if (m >> v) & 1]
            outside = [v for v in range(4) if not (m >> v) & 1]
            if len(inside) in (1, 3):
                lone = inside[0] if len(inside) == 1 else outside[0]
                tris = [[q for q, pair in enumerate(TET_EDGES) if lone in pair]]
            else:
                with0, other = (inside, outside) if 0 in inside else (outside, inside)
                j, (k, l) = with0[1], other
                e = lambda a, b: eid[(min(a, b), max(a, b))]
                q = (e(0, k), e(0, l), e(j, l), e(j, k))
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            want = pos[outside].mean(axis=0) - pos[inside].mean(axis=0)
            for r, tri in enumerate(tris):
                a, b, c = (mid[q] for q in tri)
                if np.dot(np.cross(b - a, c - a), want) < 0:
                    tri[1], tri[2] = tri[2], tri[1]
                edges[t, m, 3 * r: 3 * r + 3] = tri
            ntri[t, m] = len(tris)
    return corners, ntri, edges


def volume(lo, dims, voxel_size, truncation):
    return {"lo": np.asarray(lo, np.float32), "dims": tuple(int(d) for d in dims),
            "voxel_size": np.float32(voxel_size), "truncation": np.float32(truncation)}


def dims_from_box(lo, hi, voxel_size):
    return tuple(int(np.floor((np.float64(h) - np.float64(l)) / np.float64(voxel_size)) + 2) for l, h in zip(lo, hi))


def lattice_points(vol):
    """(nz, ny, nx, 3) float64: lo + (i, j, k) s from the float32 fields."""
    nx, ny, nz = vol["dims"]
    s = np.float64(vol["voxel_size"])
    lo = vol["lo"].astype(np.float64)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([lo[0] + i.astype(np.float64) * s, lo[1] + j.astype(np.float64) * s,
                     lo[2] + k.astype(np.float64) * s], axis=-1)


def integrate(grid, vol, view, depth, image, kind=MEDIAN, min_alpha=0.5):
    """One view into grid ((5, nz, ny, nx) float32) in place.  view: dict with world_to_camera (3, 4), fx, fy, cx, cy,
    width, height, near (all taken as float32).  depth (H, W, 2), image (H, W, 4) float32.  Returns the update mask."""
    f64 = np.float64
    M = np.asarray(view["world_to_camera"], np.float32).astype(f64)
    fx, fy, cx, cy = (f64(np.float32(view[k])) for k in ("fx", "fy", "cx", "cy"))
    near = f64(np.float32(view["near"]))
    W, H = int(view["width"]), int(view["height"])
    trunc = f64(vol["truncation"])
    p = lattice_points(vol)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        x = ((M[0, 0] * px + M[0, 1] * py) + M[0, 2] * pz) + M[0, 3]
        y = ((M[1, 0] * px + M[1, 1] * py) + M[1, 2] * pz) + M[1, 3]
        z = ((M[2, 0] * px + M[2, 1] * py) + M[2, 2] * pz) + M[2, 3]
        ok = z > near
        u = np.floor(fx * (x / z) + cx)
        v = np.floor(fy * (y / z) + cy)
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        ui = np.where(ok, u, 0).astype(np.int64)
        vi = np.where(ok, v, 0).astype(np.int64)
        if kind == EXPECTED:
            a = image[vi, ui, 3]
            ok &= a >= np.float32(min_alpha)
            D = (depth[vi, ui, 0] / a).astype(np.float32)
        else:
            D = depth[vi, ui, 1]
        ok &= np.isfinite(D) & (D > 0)
        sdf = D.astype(f64) - z
        ok &= ~(sdf < -trunc)
        d = np.minimum(f64(1.0), sdf / trunc).astype(np.float32)
    grid[0][ok] = grid[0][ok] + np.float32(1)
    grid[1][ok] = grid[1][ok] + d[ok]
    for c in range(3):
        grid[2 + c][ok] = grid[2 + c][ok] + image[vi, ui, c][ok]
    return ok


def extract(grid, vol, min_weight=1.0, return_ids=False):
    """(vertices (n_v, 3) float32, colors (n_v, 3) float32, triangles (n_t, 3) uint32) of grid ((5, nz, ny, nx)
    float32) in the contract's order: vertices by ascending edge id, triangles by cube, tet, case.  With return_ids
    two more: the edge id 7 lin(a) + code - 1 of every vertex (n_v, int64) and the linear index of the cube of every
    triangle (n_t, int64), which say where in the device's two scans a vertex and a triangle come from."""
    nx, ny, nz = vol["dims"]
    corners, ntri, edges = tet_table()
    W = grid[0].reshape(-1)
    with np.errstate(all="ignore"):
        f = (grid[1].reshape(-1) / W).astype(np.float32)
        col = [(grid[2 + c].reshape(-1) / W).astype(np.float32) for c in range(3)]
    ok = (W >= np.float32(min_weight)).reshape(nz, ny, nx)
    inside = (f < 0).reshape(nz, ny, nx)
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    cm = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        valid &= ok[sl]
        cm |= inside[sl].astype(np.int64) << c
    active = valid & (cm != 0) & (cm != 255)
    off = lambda c: (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    tri_edges, tri_cubes = [], []
    for k, j, i in zip(*np.nonzero(active)):   # ascending cube linear index
        lin = (int(k) * ny + int(j)) * nx + int(i)
        m8 = int(cm[k, j, i])
        for t in range(6):
            m = sum(((m8 >> int(corners[t][v])) & 1) << v for v in range(4))
            for r in range(int(ntri[t, m])):
                ids = []
                for q in edges[t, m, 3 * r: 3 * r + 3]:
                    va, vb = TET_EDGES[int(q)]
                    ca, cb = int(corners[t][va]), int(corners[t][vb])
                    ids.append(7 * (lin + off(ca)) + (cb - ca) - 1)
                tri_edges.append(ids)
                tri_cubes.append(lin)
    tri_edges = np.array(tri_edges, dtype=np.int64).reshape(-1, 3)
    used = np.unique(tri_edges)
    triangles = np.searchsorted(used, tri_edges).astype(np.uint32)
    a = used // 7
    code = used % 7 + 1
    delta = np.stack([code & 1, (code >> 1) & 1, (code >> 2) & 1], axis=1).astype(np.float64)
    b = a + delta[:, 0].astype(np.int64) + delta[:, 1].astype(np.int64) * nx + delta[:, 2].astype(np.int64) * nx * ny
    fa, fb = f[a].astype(np.float64), f[b].astype(np.float64)
    t = fa / (fa - fb)
    idx = np.stack([a % nx, (a // nx) % ny, a // (nx * ny)], axis=1).astype(np.float64)
    lo = vol["lo"].astype(np.float64)
    s = np.float64(vol["voxel_size"])
    vertices = (lo[None, :] + (idx + t[:, None] * delta) * s).astype(np.float32)
    colors = np.stack([(col[c][a].astype(np.float64) + t * (col[c][b].astype(np.float64) - col[c][a].astype(np.float64)))
                       for c in range(3)], axis=1).astype(np.float32)
    mesh = vertices.reshape(-1, 3), colors.reshape(-1, 3), triangles.reshape(-1, 3)
    return mesh + (used, np.array(tri_cubes, dtype=np.int64)) if return_ids else mesh


def grid_from_field(f, valid=None, color=None):
    """A (5, nz, ny, nx) float32 grid with W = 1 (0 where not valid), S = f and C = color ((3, nz, ny, nx)) or 0.5."""
    f = np.asarray(f, np.float32)
    g = np.zeros((5,) + f.shape, np.float32)
    g[0] = 1.0 if valid is None else np.asarray(valid, np.float32)
    g[1] = f * g[0]
    g[2:5] = (0.5 if color is None else np.asarray(color, np.float32)) * g[0]
    return g


# ---- invariants of a triangle mesh ------------------------------------------------------------------------------------
def edge_counts(triangles):
    """(undirected, directed): dicts edge -> number of triangles."""
    und, dire = {}, {}
    for a, b, c in np.asarray(triangles, np.int64):
        for e in ((a, b), (b, c), (c, a)):
            dire[e] = dire.get(e, 0) + 1
            k = (min(e), max(e))
            und[k] = und.get(k, 0) + 1
    return und, dire


def edge_multiplicity(triangles):
    """edge_counts for a large mesh, without the dicts: (edges (m, 2) int64 with a < b, the number of triangles on each
    of them (m), the number of triangles on each directed edge (one entry per distinct directed edge))."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    n = int(t.max()) + 1 if t.size else 1
    _, directed = np.unique(a * n + b, return_counts=True)
    key, undirected = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    return np.stack([key // n, key % n], axis=1), undirected, directed


# ---- where in the device's scans an id lies (spz_mesh.hip: blocks of kScanTile values, their sums 256 at a time) ------
SCAN_TILE, SCAN_CHUNK = 2048, 256


def scan_blocks(count):
    """The blocks of a scan over `count` values."""
    return -(-int(count) // SCAN_TILE)


def scan_chunk_counts(ids, count):
    """How many of `ids` (positions in a scan over `count` values) fall into each chunk of 256 blocks: one entry per
    chunk the scan walks."""
    ids = np.asarray(ids, np.int64)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < count)
    return np.bincount(ids // SCAN_TILE // SCAN_CHUNK, minlength=-(-scan_blocks(count) // SCAN_CHUNK))


def euler_characteristic(num_vertices, triangles):
    und, _ = edge_counts(triangles)
    return int(num_vertices) - len(und) + len(triangles)


def triangle_normals(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


# ---- the analytic fields of the tests (lattice 20 x 18 x 22, unit spacing, lo = 0) ------------------------------------
FIELD_DIMS = (20, 18, 22)
SPHERE_C, SPHERE_R = (9.3, 8.6, 10.4), 6.7


def field_coords(dims=FIELD_DIMS):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)


def sphere_field():
    x, y, z = field_coords()
    return np.sqrt((x - SPHERE_C[0]) ** 2 + (y - SPHERE_C[1]) ** 2 + (z - SPHERE_C[2]) ** 2) - SPHERE_R


def torus_field(R=5.2, r=2.1):
    x, y, z = field_coords()
    q = np.sqrt((x - SPHERE_C[0]) ** 2 + (y - SPHERE_C[1]) ** 2) - R
    return np.sqrt(q * q + (z - SPHERE_C[2]) ** 2) - r


def plane_field():
    x, _, _ = field_coords()
    return x - 7.0


def field_color(dims=FIELD_DIMS):
    x, y, z = field_coords(dims)
    return np.stack([x / float(dims[0]), y / float(dims[1]), z / float(dims[2])]).astype(np.float32)


def analytic_grids():
    """name -> (grid, volume) of the four analytic fields."""
    vol = volume((0.0, 0.0, 0.0), FIELD_DIMS, 1.0, 4.0)
    x, _, _ = field_coords()
    col = field_color()
    return {"sphere": (grid_from_field(sphere_field(), color=col), vol),
            "torus": (grid_from_field(torus_field(), color=col), vol),
            "half_sphere": (grid_from_field(sphere_field(), valid=x < 10, color=col), vol),
            "plane": (grid_from_field(plane_field(), color=col), vol)}
