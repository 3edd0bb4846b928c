"""A float64 numpy restatement of the render scores (include/spz_amd.h "render scores"; DESIGN §8 "Prune"), built on
tests/render_ref.py: its preprocess, depth order and tiles, and the same per-pixel blend loop, which here also adds each
used (pixel, Gaussian) pair's weight w = T a to the Gaussian's sum and maximum.  The sums are in pixel units (the
device's u64 sums times 2^-24)."""
import numpy as np

import render_ref as RR


def _blend_weights(rec, order, u, v, wsum, wmax):
    """render_ref._blend over the pixels (u, v), adding every used pair's w = T a into wsum / wmax; returns T."""
    T = np.ones(u.shape)
    live = np.ones(u.shape, dtype=bool)
    mean = rec["mean"].astype(np.float64)
    conic = rec["conic"].astype(np.float64)
    op = rec["opacity"].astype(np.float64)
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
        if take.any():
            w = (T * a)[take]
            wsum[g] += w.sum()
            wmax[g] = max(wmax[g], w.max())
        T = np.where(take, Tn, T)
    return T


def view_scores(cloud, sh_degree, cam, antialiased=False, rec=None):
    """(weight_sum, weight_max, alpha_sum) of one view: float64 per Gaussian, and the image's sum of 1 - T."""
    if rec is None:
        rec = RR.preprocess(cloud, sh_degree, cam, antialiased)
    n = rec["opacity"].size
    wsum, wmax = np.zeros(n), np.zeros(n)
    W, H = cam["width"], cam["height"]
    tw, th = RR.tiles(cam)
    order = RR.depth_order(rec)
    r = rec["rect"][order]
    alpha = 0.0
    for ty in range(th):
        for tx in range(tw):
            sel = order[(r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])]
            vv, uu = np.mgrid[ty * RR.TILE:min(H, ty * RR.TILE + RR.TILE), tx * RR.TILE:min(W, tx * RR.TILE + RR.TILE)]
            T = _blend_weights(rec, sel, uu.astype(np.float64), vv.astype(np.float64), wsum, wmax)
            alpha += float((1.0 - T).sum())
    return wsum, wmax, alpha


def scores(cloud, sh_degree, cams, antialiased=False):
    """(weight_sum, weight_max) over the views `cams` (render_ref.camera dicts), float64 per Gaussian."""
    n = cloud["alphas"].size
    wsum, wmax = np.zeros(n), np.zeros(n)
    for cam in cams:
        s, m, _ = view_scores(cloud, sh_degree, cam, antialiased)
        wsum += s
        wmax = np.maximum(wmax, m)
    return wsum, wmax


def keep_mask(score, rule, value):
    """The keep mask of a rule over scores (any numeric array): 'keep' K, 'keep_fraction' f (K = min(n, ceil(f n))) or
    'min_score' s (score >= s); the top K by (score descending, index ascending)."""
    n = score.size
    if rule == "min_score":
        return score >= value
    k = int(value) if rule == "keep" else min(n, int(np.ceil(value * n)))
    order = np.lexsort((np.arange(n), -score.astype(np.float64) if score.dtype.kind == "f" else ~score))
    mask = np.zeros(n, dtype=bool)
    mask[order[:k]] = True
    return mask
