"""A float64 numpy restatement of the depth contract (include/spz_amd.h "render depth"; DESIGN §8 "Render"): the blend
of tests/render_ref.py with, for every pair a pixel uses, D += (T a) z and the first Gaussian after which T' < 0.5 taken
as the pixel's median.  The preprocess, the (depth, index) order and the tiles are render_ref's; the records are read as
the float32 values the device stores.

Every function returns a dict of (height, width) arrays:
  accumulated  D (float64), 0 where nothing was blended
  alpha        1 - T (float64)
  median       the median Gaussian's float32 record depth (+inf: none)
  index        the median Gaussian's input index (int64, -1: none)
  gap          the smallest |T' - 0.5| over the pairs the pixel used (+inf when it used none): a pixel whose gap is
               below the float32 blend's rounding may take its median one Gaussian earlier or later on the device"""
import numpy as np

import render_ref as RR


def _blend(rec, order, u, v):
    """RR._blend's loop at the pixels (u, v), with the depth terms; returns (D, T, median, index, gap)."""
    T = np.ones(u.shape)
    D = np.zeros(u.shape)
    live = np.ones(u.shape, dtype=bool)
    median = np.full(u.shape, np.inf, dtype=np.float32)
    index = np.full(u.shape, -1, dtype=np.int64)
    gap = np.full(u.shape, np.inf)
    mean = rec["mean"].astype(np.float64)
    conic = rec["conic"].astype(np.float64)
    op = rec["opacity"].astype(np.float64)
    z = rec["depth"]
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
        D[take] += T[take] * a[take] * float(z[g])
        gap[take] = np.minimum(gap[take], np.abs(Tn[take] - 0.5))
        first = take & (index < 0) & (Tn < 0.5)
        median[first] = z[g]
        index[first] = g
        T = np.where(take, Tn, T)
    return D, T, median, index, gap


def _maps(cam):
    H, W = cam["height"], cam["width"]
    return {"accumulated": np.zeros((H, W)), "alpha": np.zeros((H, W)),
            "median": np.full((H, W), np.inf, dtype=np.float32), "index": np.full((H, W), -1, dtype=np.int64),
            "gap": np.full((H, W), np.inf)}


def _store(out, vv, uu, res):
    D, T, median, index, gap = res
    out["accumulated"][vv, uu] = D
    out["alpha"][vv, uu] = 1.0 - T
    out["median"][vv, uu] = median
    out["index"][vv, uu] = index
    out["gap"][vv, uu] = gap


def render_depth(cloud, sh_degree, cam, antialiased=False, rec=None):
    """The maps of the tiled contract."""
    if rec is None:
        rec = RR.preprocess(cloud, sh_degree, cam, antialiased)
    W, H = cam["width"], cam["height"]
    tw, th = RR.tiles(cam)
    out = _maps(cam)
    order = RR.depth_order(rec)
    r = rec["rect"][order]
    for ty in range(th):
        for tx in range(tw):
            sel = order[(r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])]
            vv, uu = np.mgrid[ty * RR.TILE:min(H, ty * RR.TILE + RR.TILE), tx * RR.TILE:min(W, tx * RR.TILE + RR.TILE)]
            _store(out, vv, uu, _blend(rec, sel, uu.astype(np.float64), vv.astype(np.float64)))
    return out


def render_depth_bruteforce(cloud, sh_degree, cam, antialiased=False):
    """Every visible Gaussian at every pixel, in depth order, with no tiles."""
    rec = RR.preprocess(cloud, sh_degree, cam, antialiased)
    vv, uu = np.mgrid[0:cam["height"], 0:cam["width"]]
    out = _maps(cam)
    _store(out, vv, uu, _blend(rec, RR.depth_order(rec), uu.astype(np.float64), vv.astype(np.float64)))
    return out


def expected(maps):
    """accumulated / alpha where alpha > 0, +inf elsewhere."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(maps["alpha"] > 0, maps["accumulated"] / maps["alpha"], np.inf)
