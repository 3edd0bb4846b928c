"""A float64 numpy restatement of the image-metrics contract (include/spz_amd.h "image metrics"; DESIGN §8 "Compare"):
values clamped to [0, 1] with NaN -> 0, the first three channels, PSNR / MSE / L1 / max |d|, and SSIM with an 11x11
Gaussian window (sigma 1.5) and zero padding, by separable passes (rows, then columns, taps in order).  numpy only."""
import math

import numpy as np

C1 = 0.01 * 0.01
C2 = 0.03 * 0.03
RADIUS = 5


def window():
    """w_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum, the sum taken in k order (as the device computes it)."""
    e = [math.exp(-((k - RADIUS) ** 2) / (2.0 * 1.5 * 1.5)) for k in range(2 * RADIUS + 1)]
    s = 0.0
    for v in e:
        s += v
    return np.array([v / s for v in e], dtype=np.float64)


def clamp(x):
    """fminf(fmaxf(v, 0), 1): NaN -> 0, +inf -> 1, -inf -> 0; float64 out."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    x = np.where(x > 0.0, x, 0.0)
    return np.where(x < 1.0, x, 1.0)


def blur(x, w=None):
    """'same' Gaussian filter of a (H, W) float64 plane with zero padding: along rows, then along columns."""
    w = window() if w is None else w
    h, wd = x.shape
    p = np.zeros((h, wd + 2 * RADIUS))
    p[:, RADIUS:RADIUS + wd] = x
    acc = np.zeros((h, wd))
    for k in range(2 * RADIUS + 1):
        acc = acc + w[k] * p[:, k:k + wd]
    q = np.zeros((h + 2 * RADIUS, wd))
    q[RADIUS:RADIUS + h] = acc
    out = np.zeros((h, wd))
    for k in range(2 * RADIUS + 1):
        out = out + w[k] * q[k:k + h]
    return out


def ssim_plane(a, b, blur_fn=blur):
    """Per-pixel S of one channel (float64 planes, already clamped)."""
    ma, mb = blur_fn(a), blur_fn(b)
    maa, mbb, mab = blur_fn(a * a), blur_fn(b * b), blur_fn(a * b)
    mu_ab, mu_aa, mu_bb = ma * mb, ma * ma, mb * mb
    sa, sb, sab = maa - mu_aa, mbb - mu_bb, mab - mu_ab
    return ((2.0 * mu_ab + C1) * (2.0 * sab + C2)) / ((mu_aa + mu_bb + C1) * (sa + sb + C2))


def metrics(a, b, blur_fn=blur):
    """dict(mse, psnr, ssim, l1, max_abs) and the (H, W) SSIM map of two (H, W, 3 or 4) images."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.ndim == 3 and b.ndim == 3 and a.shape[:2] == b.shape[:2]
    ca, cb = clamp(a[..., :3]), clamp(b[..., :3])
    d = ca - cb
    n = d.size
    mse = float(np.sum(d * d)) / n
    s = np.stack([ssim_plane(ca[..., c], cb[..., c], blur_fn) for c in range(3)], axis=-1)
    return {"mse": mse, "psnr": math.inf if mse == 0.0 else 10.0 * math.log10(1.0 / mse),
            "ssim": float(np.sum(s)) / n, "l1": float(np.sum(np.abs(d))) / n,
            "max_abs": float(np.max(np.abs(d)))}, (s[..., 0] + s[..., 1] + s[..., 2]) / 3.0


def blur_bruteforce(x):
    """The same filter as one 11x11 window sum per pixel (the outer product of the weights)."""
    w = window()
    g = np.outer(w, w)
    h, wd = x.shape
    p = np.zeros((h + 2 * RADIUS, wd + 2 * RADIUS))
    p[RADIUS:RADIUS + h, RADIUS:RADIUS + wd] = x
    out = np.zeros((h, wd))
    for y in range(h):
        for xx in range(wd):
            out[y, xx] = np.sum(g * p[y:y + 2 * RADIUS + 1, xx:xx + 2 * RADIUS + 1])
    return out
