"""The photo loss, the exposure apply and the exposure's Adam step of DESIGN §8 "Fit" on the CPU (include/spz_amd.h
"photo loss" and "refine images").

photo_loss(): the contract as torch operations in a chosen dtype, on loss_ref's clamp and blur and metrics_ref's window
and constants.  The exposed render is t_c = ((o_c + M_c0 a_0) + M_c1 a_1) + M_c2 a_2; the clamp is torch.clamp after
NaN -> 0, so autograd passes 0 <= t <= 1, both ends included, and nothing elsewhere.  A pixel with a non-finite a has t
infinite or NaN in every channel (inf x = +-inf, inf 0 = NaN), so all its gates are closed: its t is computed outside the
graph, and inside it its a is replaced by 0, so that autograd skips it instead of multiplying an infinity by zero.
The gradients to a and to the 12 exposure values come from autograd.

apply_exposure_f32(): out = M a + o in numpy float32, operation by operation.
exposure_adam_step(): one Adam step over 12 values in float64, as the contract words it."""
import numpy as np
import torch

import loss_ref as LR
import metrics_ref as MR

IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def clamp_weights(weight):
    """Weights as the device reads them: float32, NaN -> 0, clamped to [0, 1]; float64 out."""
    return MR.clamp(weight)


def photo_terms(a, b, lam, weight=None, exposure=None, dtype=torch.float64):
    """(L, l1, ssim) as 0-d tensors of `dtype` in a graph from a (a torch tensor (H, W, 3 or 4) of `dtype`) and
    exposure (None, or a torch tensor (3, 4) of `dtype`); b, weight: arrays.  W == 0: None."""
    b = torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dtype)
    rgb = a[..., :3]
    if exposure is None:
        t = rgb
    else:
        finite = torch.isfinite(rgb).all(dim=-1, keepdim=True)
        safe = torch.where(finite, rgb, torch.zeros_like(rgb))
        e = exposure
        t = ((e[:, 3] + e[:, 0] * safe[..., 0:1]) + e[:, 1] * safe[..., 1:2]) + e[:, 2] * safe[..., 2:3]
        with torch.no_grad():
            raw = ((e[:, 3] + e[:, 0] * rgb[..., 0:1]) + e[:, 1] * rgb[..., 1:2]) + e[:, 2] * rgb[..., 2:3]
        t = torch.where(finite, t, raw)
    ca, cb = LR._clamp(t), LR._clamp(b[..., :3])
    h, wd = ca.shape[:2]
    w = torch.ones((h, wd), dtype=dtype) if weight is None else torch.as_tensor(clamp_weights(weight)).to(dtype)
    total = w.sum()
    if float(total) == 0.0:
        return None
    win = torch.as_tensor(MR.window()).to(dtype)
    l1 = (w[..., None] * torch.abs(ca - cb)).sum() / (3.0 * total)
    s = 0.0
    for c in range(3):
        x, y = ca[..., c], cb[..., c]
        ma, mb = LR._blur(x, win), LR._blur(y, win)
        maa, mbb, mab = LR._blur(x * x, win), LR._blur(y * y, win), LR._blur(x * y, win)
        mu_ab, mu_aa, mu_bb = ma * mb, ma * ma, mb * mb
        sa, sb, sab = maa - mu_aa, mbb - mu_bb, mab - mu_ab
        sc = ((2.0 * mu_ab + MR.C1) * (2.0 * sab + MR.C2)) / ((mu_aa + mu_bb + MR.C1) * (sa + sb + MR.C2))
        s = s + (w * sc).sum()
    ssim = s / (3.0 * total)
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim


def photo_loss(a, b, lam, weight=None, exposure=None, dtype=torch.float64):
    """dict(L, l1, ssim: floats; grad: dL/da, a float64 numpy array shaped like a; exposure_grad: dL/d[M | o], a float64
    (3, 4) array, or None without an exposure) of two (H, W, 3 or 4) images."""
    a = np.asarray(a, dtype=np.float32)
    t = torch.as_tensor(a).to(dtype).clone().requires_grad_(True)
    e = None
    if exposure is not None:
        e = torch.as_tensor(np.asarray(exposure, dtype=np.float64).reshape(3, 4)).to(dtype).clone().requires_grad_(True)
    terms = photo_terms(t, b, lam, weight, e, dtype)
    if terms is None:
        return {"L": 0.0, "l1": 0.0, "ssim": 1.0, "grad": np.zeros(a.shape), "exposure_grad":
                None if e is None else np.zeros((3, 4))}
    L, l1, ssim = terms
    L.backward()
    return {"L": float(L.detach()), "l1": float(l1.detach()), "ssim": float(ssim.detach()),
            "grad": t.grad.to(torch.float64).numpy(),
            "exposure_grad": None if e is None else e.grad.to(torch.float64).numpy()}


def apply_exposure_f32(image, exposure):
    """out_c = ((o_c + M_c0 a_0) + M_c1 a_1) + M_c2 a_2 in float32, the 12 values rounded to float32 first, each
    operation rounded once; a fourth channel is copied."""
    e = np.asarray(exposure, dtype=np.float64).reshape(3, 4).astype(np.float32)
    a = np.asarray(image, dtype=np.float32)
    out = a.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            out[..., c] = ((e[c, 3] + e[c, 0] * a[..., 0]) + e[c, 1] * a[..., 1]) + e[c, 2] * a[..., 2]
    assert out.dtype == np.float32
    return out


def exposure_adam_step(e, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One step over float64 arrays of 12 values: (e', m', v').  A value whose gradient is not finite keeps e, m and v."""
    e, g, m, v = (np.asarray(x, dtype=np.float64) for x in (e, g, m, v))
    with np.errstate(all="ignore"):
        m1 = beta1 * m + (1.0 - beta1) * g
        v1 = beta2 * v + ((1.0 - beta2) * g) * g
        den = np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps
        e1 = e - (lr / (1.0 - beta1 ** t)) * (m1 / den)
    ok = np.isfinite(g)
    return np.where(ok, e1, e), np.where(ok, m1, m), np.where(ok, v1, v)
