"""A float64 numpy restatement of the render contract (include/spz_amd.h "render"; DESIGN §8 "Render"): the per-Gaussian
preprocess (3DGS forward pass with a general principal point), the 16x16 tile rectangles, the (depth, index) order and
the per-pixel blend.  Vectorised over Gaussians for the preprocess and over a tile's pixels for the blend, which loops
over the tile's entries.  The records are rounded to float32 as the device stores them, and the blend reads them so.
For long lists and large views: walk() is the same blend vectorised over a tile's list as well (bit for bit _blend's
values), and render_tiles() renders only the tiles asked for.

A cloud is a dict of the GaussianCloud arrays (float32): positions, scales, rotations (xyzw), alphas, colors, sh
([point][coeff][rgb]), already in the camera's frame."""
import numpy as np

TILE = 16
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}


def camera(world_to_camera, fx, fy, cx, cy, width, height, near=0.2, background=(0.0, 0.0, 0.0), max_sh_degree=3):
    """The camera as the device sees it: every value rounded to float32 first."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    m = np.asarray(world_to_camera, dtype=np.float32).astype(np.float64).reshape(3, 4)
    return {"R": m[:, :3].copy(), "t": m[:, 3].copy(), "fx": f(fx), "fy": f(fy), "cx": f(cx), "cy": f(cy),
            "width": int(width), "height": int(height), "near": f(near),
            "background": np.asarray(background, dtype=np.float32).astype(np.float64),
            "max_sh_degree": int(max_sh_degree)}


def look_at(eye, target, up):
    """spz::lookAt in float64, rounded to float32: z = normalize(target - eye), x = normalize(z x up), y = z x x."""
    eye, target, up = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    u = up / np.linalg.norm(up)
    x = np.cross(z, u)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-(R @ eye))[:, None]], axis=1).astype(np.float32)


def tiles(cam):
    return (cam["width"] + TILE - 1) // TILE, (cam["height"] + TILE - 1) // TILE


def preprocess(cloud, sh_degree, cam, antialiased=False):
    """The records (input order): mean (n, 2), conic (n, 3), opacity, rgb (n, 3), depth (+inf: invisible), rect (n, 4)
    as float32 / int64, plus visible (bool), r3 = 3 sqrt(lambda) before the ceil, camera_xyz = R p + t, det0 and a0c0
    (all f64)."""
    n = cloud["alphas"].size
    P = cloud["positions"].reshape(n, 3).astype(np.float64)
    R, t = cam["R"], cam["t"]
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):  # non-finite inputs become invisible Gaussians
        x = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + t[0]
        y = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + t[1]
        z = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + t[2]
        vis = z > cam["near"]
        fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        W, H = float(cam["width"]), float(cam["height"])
        mx = fx * x / z + cx - 0.5
        my = fy * y / z + cy - 0.5
        q = cloud["rotations"].reshape(n, 4).astype(np.float64)
        q = q / np.sqrt((q * q).sum(axis=1))[:, None]
        qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        Rq = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                       2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                       2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], axis=1)
        Rq = Rq.reshape(n, 3, 3)
        s = np.exp(cloud["scales"].reshape(n, 3).astype(np.float64))
        M = Rq * s[:, None, :]
        S = M @ np.transpose(M, (0, 2, 1))
        lxp, lxn = (W - cx) / fx + 0.3 * W / fx, cx / fx + 0.3 * W / fx
        lyp, lyn = (H - cy) / fy + 0.3 * H / fy, cy / fy + 0.3 * H / fy
        tx = z * np.clip(x / z, -lxn, lxp)
        ty = z * np.clip(y / z, -lyn, lyp)
        J = np.zeros((n, 2, 3))
        J[:, 0, 0] = fx / z
        J[:, 0, 2] = -(fx * tx) / (z * z)
        J[:, 1, 1] = fy / z
        J[:, 1, 2] = -(fy * ty) / (z * z)
        T = J @ R
        cov = T @ S @ np.transpose(T, (0, 2, 1))
        a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
        det0 = a * c - b * b
        a, c = a + 0.3, c + 0.3
        det = a * c - b * b
        vis &= det > 0
        op = 1.0 / (1.0 + np.exp(-cloud["alphas"].astype(np.float64)))
        if antialiased:
            op = op * np.sqrt(np.maximum(det0, 0.0) / det)
        conic = np.stack([c / det, -b / det, a / det], axis=1)
        mid = 0.5 * (a + c)
        lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det))
        r3 = 3.0 * np.sqrt(lam)
        radius = np.ceil(r3)
        vis &= np.isfinite(mx) & np.isfinite(my) & np.isfinite(radius) & np.isfinite(conic).all(axis=1)
        vis &= np.isfinite(op)  # a NaN alpha: min(0.99, NaN) has no one reading, so the Gaussian is not blended at all
        tw, th = tiles(cam)
        x0 = np.clip(np.floor((mx - radius) / 16.0), 0, tw)
        x1 = np.clip(np.floor((mx + radius + 15.0) / 16.0), 0, tw)
        y0 = np.clip(np.floor((my - radius) / 16.0), 0, th)
        y1 = np.clip(np.floor((my + radius + 15.0) / 16.0), 0, th)
        vis &= (x1 > x0) & (y1 > y0)
        campos = -(R.T @ t)
        d = P - campos
        d = d / np.sqrt((d * d).sum(axis=1))[:, None]
        rgb = sh_colour(cloud, sh_degree, min(sh_degree, cam["max_sh_degree"]), d)
    rec = {
        "mean": np.where(vis[:, None], np.stack([mx, my], axis=1), 0).astype(np.float32),
        "conic": np.where(vis[:, None], conic, 0).astype(np.float32),
        "opacity": np.where(vis, op, 0).astype(np.float32),
        "rgb": np.where(vis[:, None], rgb, 0).astype(np.float32),
        "depth": np.where(vis, z, np.inf).astype(np.float32),
        "rect": np.where(vis[:, None], np.stack([x0, y0, x1, y1], axis=1), 0).astype(np.int64),
        "visible": vis,
        "r3": r3,
        "camera_xyz": np.stack([x, y, z], axis=1),  # p_c = R p + t, for tests that sort Gaussians by where they lie
        "det0": det0,                               # of the 2D covariance before the 0.3, and the product it is cut from
        "a0c0": (a - 0.3) * (c - 0.3),
    }
    return rec


def sh_colour(cloud, file_degree, degree, d):
    n = cloud["alphas"].size
    col = cloud["colors"].reshape(n, 3).astype(np.float64)
    D = SH_DIM[file_degree]
    sh = cloud["sh"].reshape(n, D, 3).astype(np.float64) if D else np.zeros((n, 0, 3))
    x, y, z = (d[:, k:k + 1] for k in range(3))
    r = C0 * col
    if degree >= 1:
        r = r - C1 * y * sh[:, 0] + C1 * z * sh[:, 1] - C1 * x * sh[:, 2]
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + C2[0] * xy * sh[:, 3] + C2[1] * yz * sh[:, 4] + C2[2] * (2.0 * zz - xx - yy) * sh[:, 5]
             + C2[3] * xz * sh[:, 6] + C2[4] * (xx - yy) * sh[:, 7])
        if degree >= 3:
            r = (r + C3[0] * y * (3.0 * xx - yy) * sh[:, 8] + C3[1] * xy * z * sh[:, 9]
                 + C3[2] * y * (4.0 * zz - xx - yy) * sh[:, 10] + C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[:, 11]
                 + C3[4] * x * (4.0 * zz - xx - yy) * sh[:, 12] + C3[5] * z * (xx - yy) * sh[:, 13]
                 + C3[6] * x * (xx - 3.0 * yy) * sh[:, 14])
    r = r + 0.5
    return np.maximum(r, 0.0)


def depth_order(rec):
    """Visible Gaussians by ascending (float32 depth, index)."""
    idx = np.nonzero(rec["visible"])[0]
    return idx[np.lexsort((idx, rec["depth"][idx]))]


def entry_count(rec):
    r = rec["rect"]
    return int(((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]))[rec["visible"]].sum())


def _blend(rec, order, u, v, cam):
    """Blend the Gaussians `order` (in that order) at the pixels (u, v) (float arrays); returns (rgb (k, 3), T (k))."""
    T = np.ones(u.shape)
    C = np.zeros(u.shape + (3,))
    live = np.ones(u.shape, dtype=bool)
    mean = rec["mean"].astype(np.float64)
    conic = rec["conic"].astype(np.float64)
    op = rec["opacity"].astype(np.float64)
    rgb = rec["rgb"].astype(np.float64)
    for g in order:
        if not live.any():
            break
        dx, dy = u - mean[g, 0], v - mean[g, 1]
        A, B, Cc = conic[g]
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        a = np.minimum(0.99, op[g] * np.exp(np.minimum(power, 0.0)))
        take = live & (power <= 0) & (a >= 1.0 / 255.0)
        Tn = T * (1.0 - a)
        stop = take & (Tn < 1e-4)
        live &= ~stop
        take &= ~stop
        C[take] += (T[take] * a[take])[:, None] * rgb[g][None, :]
        T = np.where(take, Tn, T)
    return C, T


BAND = 1e-4  # a pair within this relative distance of a decision threshold is marginal (render_grad_ref)


def walk(rec, sel, u, v):
    """_blend's walk over the Gaussians sel at the pixels (u, v) (flat float arrays), vectorised over the list: the
    (len(sel), pixels) arrays of power and a, then cumprod along the list.  A pair that is not used multiplies T by
    exactly 1, so cumprod makes _blend's products in _blend's order and every value below has _blend's bits.  A dict:
      take      (L, pixels) bool, the used pairs
      w         (L, pixels) T a of the used pairs, 0 elsewhere
      T         (pixels) the transmittance left
      stopped   (pixels) bool: the pixel reached the stop
      last      (pixels) the list position of the last used pair (-1: none)
      clamped   the number of used pairs whose alpha was clamped at 0.99
      marginal  (pixels) the number of considered pairs within a relative BAND of a decision threshold (the rules of
                render_grad_ref._walk), which a float32 blend might decide the other way"""
    u, v = np.ascontiguousarray(u, dtype=np.float64).ravel(), np.ascontiguousarray(v, dtype=np.float64).ravel()
    sel = np.asarray(sel, dtype=np.int64)
    L, P = sel.size, u.size
    if L == 0:
        return {"take": np.zeros((0, P), dtype=bool), "w": np.zeros((0, P)), "T": np.ones(P),
                "stopped": np.zeros(P, dtype=bool), "last": np.full(P, -1, dtype=np.int64), "clamped": 0,
                "marginal": np.zeros(P, dtype=np.int64)}
    mean = rec["mean"][sel].astype(np.float64)
    conic = rec["conic"][sel].astype(np.float64)
    op = rec["opacity"][sel].astype(np.float64)[:, None]
    dx, dy = u[None, :] - mean[:, 0:1], v[None, :] - mean[:, 1:2]
    A, B, Cc = conic[:, 0:1], conic[:, 1:2], conic[:, 2:3]
    power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
    raw = op * np.exp(np.minimum(power, 0.0))
    a = np.minimum(0.99, raw)
    neg = power <= 0
    cand = neg & (a >= 1.0 / 255.0)
    through = np.cumprod(np.where(cand, 1.0 - a, 1.0), axis=0)  # T after each pair, were there no stop
    before = np.concatenate([np.ones((1, P)), through[:-1]], axis=0)
    stops = cand & (through < 1e-4)
    stopped = stops.any(axis=0)
    at = np.where(stopped, np.argmax(stops, axis=0), L)  # the list position of the pair that stops the pixel
    k = np.arange(L)[:, None]
    live = k <= at[None, :]  # still walking when the pair is considered
    take = cand & (k < at[None, :])
    m = live & (np.abs(power) < 1e-6)
    m |= live & neg & (np.abs(255.0 * a - 1.0) < BAND)
    m |= live & neg & (np.abs(raw / 0.99 - 1.0) < BAND)
    m |= live & cand & (np.abs(through / 1e-4 - 1.0) < BAND)
    T = np.where(stopped, before[np.minimum(at, L - 1), np.arange(P)], through[-1])  # a stop leaves T as it was
    last = np.where(take.any(axis=0), L - 1 - np.argmax(take[::-1], axis=0), -1)
    return {"take": take, "w": np.where(take, before * a, 0.0), "T": T, "stopped": stopped, "last": last,
            "clamped": int((take & (raw > 0.99)).sum()), "marginal": m.sum(axis=0)}


def _colours(rec, order, wk, shape):
    """(rgb, T) of _blend from walk()'s result, bit for bit.  The colours add up along the list with cumsum, one term
    after the other as _blend adds them; an unused pair adds exactly 0."""
    C = np.zeros((wk["T"].size, 3))
    if len(order):
        rgb = rec["rgb"][np.asarray(order, dtype=np.int64)].astype(np.float64)
        for c in range(3):
            C[:, c] = np.cumsum(wk["w"] * rgb[:, c:c + 1], axis=0)[-1]
    return C.reshape(shape + (3,)), wk["T"].reshape(shape)


def _blend_vec(rec, order, u, v, cam=None):
    """_blend through walk(): the same (rgb, T), bit for bit."""
    return _colours(rec, order, walk(rec, order, u, v), np.shape(u))


def tile_lists(rec, cam, tile_list=None):
    """{tile id (ty * tiles_x + tx): the Gaussians of its list in blend order} for the tiles of tile_list (None: the
    touched tiles, those with a list).  From the entries themselves (every visible Gaussian's rectangle), so the cost
    does not grow with the tile count."""
    tw, th = tiles(cam)
    order = depth_order(rec)
    r = rec["rect"][order]
    nx, ny = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    cnt = nx * ny
    g = np.repeat(np.arange(order.size), cnt)              # position in the depth order, ascending
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    key = (r[g, 1] + j // nx[g]) * tw + r[g, 0] + j % nx[g]
    by_tile = np.argsort(key, kind="stable")               # stable: the depth order survives within a tile
    key, g = key[by_tile], order[g[by_tile]]
    ids, start = np.unique(key, return_index=True)
    end = np.append(start[1:], key.size)
    lists = {int(t): g[s:e] for t, s, e in zip(ids, start, end)}
    if tile_list is None:
        return lists
    return {int(t): lists.get(int(t), np.zeros(0, dtype=np.int64)) for t in tile_list}


def tile_pixels(cam, t):
    """(vv, uu): the pixel rows and columns of tile t, as render()'s mgrid."""
    tw, _ = tiles(cam)
    ty, tx = divmod(int(t), tw)
    return np.mgrid[ty * TILE:min(cam["height"], ty * TILE + TILE), tx * TILE:min(cam["width"], tx * TILE + TILE)]


def render_tiles(rec, cam, tile_list, blend=None, marginal=None):
    """render() restricted to the tiles of tile_list: {tile id: (rows, columns, 4) float64}, each equal to render()'s
    image over that tile's pixels.  A view of millions of pixels costs only the tiles asked for.  blend: _blend, to
    walk as render() does (default: walk()).  marginal: a dict that receives {tile id: (rows, columns) int}, each
    pixel's number of marginal pairs."""
    out = {}
    bg = cam["background"]
    for t, sel in tile_lists(rec, cam, tile_list).items():
        vv, uu = tile_pixels(cam, t)
        if blend is None:
            wk = walk(rec, sel, uu, vv)
            C, T = _colours(rec, sel, wk, uu.shape)
            if marginal is not None:
                marginal[t] = wk["marginal"].reshape(uu.shape)
        else:
            C, T = blend(rec, sel, uu.astype(np.float64), vv.astype(np.float64), cam)
        out[t] = np.concatenate([C + T[..., None] * bg, (1.0 - T)[..., None]], axis=2)
    return out


def render(cloud, sh_degree, cam, antialiased=False, rec=None):
    """The (height, width, 4) float64 image of the tiled contract."""
    if rec is None:
        rec = preprocess(cloud, sh_degree, cam, antialiased)
    W, H = cam["width"], cam["height"]
    tw, th = tiles(cam)
    img = np.zeros((H, W, 4))
    order = depth_order(rec)
    r = rec["rect"][order]
    bg = cam["background"]
    for ty in range(th):
        for tx in range(tw):
            sel = order[(r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])]
            vv, uu = np.mgrid[ty * TILE:min(H, ty * TILE + TILE), tx * TILE:min(W, tx * TILE + TILE)]
            C, T = _blend(rec, sel, uu.astype(np.float64), vv.astype(np.float64), cam)
            img[vv, uu, :3] = C + T[..., None] * bg
            img[vv, uu, 3] = 1.0 - T
    return img


def render_bruteforce(cloud, sh_degree, cam, antialiased=False):
    """Every visible Gaussian at every pixel, in depth order, with no tiles."""
    rec = preprocess(cloud, sh_degree, cam, antialiased)
    W, H = cam["width"], cam["height"]
    vv, uu = np.mgrid[0:H, 0:W]
    C, T = _blend(rec, depth_order(rec), uu.astype(np.float64), vv.astype(np.float64), cam)
    img = np.zeros((H, W, 4))
    img[..., :3] = C + T[..., None] * cam["background"]
    img[..., 3] = 1.0 - T
    return img
