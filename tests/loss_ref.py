"""The image loss and the Adam step of DESIGN §8 "Refine" on the CPU (include/spz_amd.h "image loss" and "adam step").

loss(): L = (1 - lambda) l1 + lambda (1 - ssim) as torch operations in a chosen dtype, with tests/metrics_ref.py's
window, clamp and padding convention (NaN -> 0, then torch.clamp to [0, 1]; the first three channels; the 11 taps along
rows, then along columns, zero padding, taps in order).  The gradient to the first image comes from autograd, so the
clamp passes what torch.clamp passes: 0 <= a <= 1, both ends included.

adam_step(): one step in numpy float32, operation by operation, as the contract words it."""
import numpy as np
import torch

import metrics_ref as MR

ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")


def _clamp(x):
    return torch.clamp(torch.where(torch.isnan(x), torch.zeros_like(x), x), 0.0, 1.0)


def _blur(x, w):
    """metrics_ref.blur of a (H, W) plane in x's dtype: zero padding, rows then columns, taps in k order."""
    r = MR.RADIUS
    h, wd = x.shape
    p = torch.zeros((h, wd + 2 * r), dtype=x.dtype)
    p[:, r:r + wd] = x
    acc = torch.zeros((h, wd), dtype=x.dtype)
    for k in range(2 * r + 1):
        acc = acc + w[k] * p[:, k:k + wd]
    q = torch.zeros((h + 2 * r, wd), dtype=x.dtype)
    q[r:r + h] = acc
    out = torch.zeros((h, wd), dtype=x.dtype)
    for k in range(2 * r + 1):
        out = out + w[k] * q[k:k + h]
    return out


def loss_terms(a, b, lam, dtype=torch.float64):
    """(L, l1, ssim) as 0-d tensors of `dtype` in a graph from a (a torch tensor (H, W, 3 or 4) of `dtype`); b: array."""
    b = torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dtype)
    ca, cb = _clamp(a[..., :3]), _clamp(b[..., :3])
    w = torch.as_tensor(MR.window()).to(dtype)
    n = ca.numel()
    l1 = torch.abs(ca - cb).sum() / n
    s = 0.0
    for c in range(3):
        x, y = ca[..., c], cb[..., c]
        ma, mb = _blur(x, w), _blur(y, w)
        maa, mbb, mab = _blur(x * x, w), _blur(y * y, w), _blur(x * y, w)
        mu_ab, mu_aa, mu_bb = ma * mb, ma * ma, mb * mb
        sa, sb, sab = maa - mu_aa, mbb - mu_bb, mab - mu_ab
        s = s + (((2.0 * mu_ab + MR.C1) * (2.0 * sab + MR.C2)) / ((mu_aa + mu_bb + MR.C1) * (sa + sb + MR.C2))).sum()
    ssim = s / n
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim


def loss(a, b, lam, dtype=torch.float64):
    """dict(L, l1, ssim: floats; grad: dL/da, a float64 numpy array shaped like a) of two (H, W, 3 or 4) images."""
    t = torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype).clone().requires_grad_(True)
    L, l1, ssim = loss_terms(t, b, lam, dtype)
    L.backward()
    return {"L": float(L.detach()), "l1": float(l1.detach()), "ssim": float(ssim.detach()),
            "grad": t.grad.to(torch.float64).numpy()}


def adam_scalars(t, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """The f32 scalars of step t >= 1, computed in float64 and rounded: dict(beta1, c1, beta2, c2, eps, r, s)."""
    f = np.float32
    return {"beta1": f(beta1), "c1": f(1.0 - beta1), "beta2": f(beta2), "c2": f(1.0 - beta2), "eps": f(eps),
            "r": f(np.sqrt(1.0 - beta2 ** t)), "s": f(lr / (1.0 - beta1 ** t))}


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One step over float32 arrays: (p', m', v', skipped).  Every operation is a float32 operation rounded once; an
    element whose p or g is not finite keeps p, m and v and is counted."""
    k = adam_scalars(t, lr, beta1, beta2, eps)
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = k["beta1"] * m + k["c1"] * g
        v1 = k["beta2"] * v + (k["c2"] * g) * g
        den = np.sqrt(v1) / k["r"] + k["eps"]
        p1 = p - k["s"] * (m1 / den)
    ok = np.isfinite(p) & np.isfinite(g)
    for x in (m1, v1, den, p1):
        assert x.dtype == np.float32
    return np.where(ok, p1, p), np.where(ok, m1, m), np.where(ok, v1, v), int((~ok).sum())
