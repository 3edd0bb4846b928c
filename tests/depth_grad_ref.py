"""The derivative of the render's image and accumulated depth on the CPU (include/spz_amd.h "render depth backward" and
"depth loss"; DESIGN §8 "Depth fit"): tests/render_grad_ref.py with the record's depth z as a tenth column, rounded to
float32 with a straight-through gradient like the other nine, and a blend that also returns D = sum (T a) z over the
used pairs.  The decisions are render_grad_ref's: depth adds none.

depth_loss() is the depth loss in numpy float64 with math.fsum for the two sums."""
import math

import numpy as np
import torch

import render_grad_ref as GR


def records(cloud, sh_degree, cam, idx, antialiased=False):
    """render_grad_ref.records with z = (R p + t)_z as a tenth column: (len(idx), 10), not rounded."""
    n = cloud["alphas"].numel()
    P = cloud["positions"].reshape(n, 3)[torch.as_tensor(idx, dtype=torch.int64)]
    R, t = cam["R"], cam["t"]
    z = R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2]
    return torch.cat([GR.records(cloud, sh_degree, cam, idx, antialiased), z[:, None]], dim=1)


def blend(rec10, cam, dec, idx):
    """render_grad_ref.blend of the records rec10 with the used pairs of dec: (image (H, W, 4), D (H, W))."""
    dt = rec10.dtype
    W, H = cam["width"], cam["height"]
    row = np.full(dec["visible"].size, -1, dtype=np.int64)
    row[np.asarray(idx)] = np.arange(len(idx))
    bg = torch.as_tensor(cam["background"], dtype=dt)
    img = torch.zeros((H, W, 4), dtype=dt)
    D = torch.zeros((H, W), dtype=dt)
    for tile in dec["tiles"]:
        u, v = torch.as_tensor(tile["u"]), torch.as_tensor(tile["v"])
        if len(tile["sel"]) == 0:
            img[v, u] = torch.cat([bg, torch.zeros(1, dtype=dt)])[None, :].expand(u.numel(), 4)
            continue
        m = rec10[torch.as_tensor(row[tile["sel"]])]
        take = torch.as_tensor(tile["take"])
        dx = u.to(dt)[:, None] - m[None, :, 0]
        dy = v.to(dt)[:, None] - m[None, :, 1]
        power = -0.5 * (m[None, :, 2] * dx * dx + m[None, :, 4] * dy * dy) - m[None, :, 3] * dx * dy
        power = torch.where(take, power, torch.zeros_like(power))  # an unused pair's exp may overflow
        a = torch.clamp(m[None, :, 5] * torch.exp(power), max=0.99)
        a = torch.where(take, a, torch.zeros_like(a))
        through = torch.cumprod(1.0 - a, dim=1)
        T = torch.cat([torch.ones_like(through[:, :1]), through[:, :-1]], dim=1)
        w = T * a
        C = w @ m[:, 6:9]
        Tf = through[:, -1]
        img[v, u] = torch.cat([C + Tf[:, None] * bg[None, :], (1.0 - Tf)[:, None]], dim=1)
        D[v, u] = w @ m[:, 9]
    return img, D


def forward(cloud, sh_degree, cam, dec, antialiased=False, round_records=True):
    """(image, D, rec10) in the dtype of the cloud's tensors; rec10 is in the graph, as render_grad_ref.forward's."""
    idx = np.nonzero(dec["visible"])[0]
    rec10 = records(cloud, sh_degree, cam, idx, antialiased)
    if round_records:
        rec10 = rec10 + (rec10.detach().to(torch.float32).to(rec10.dtype) - rec10.detach())  # straight through
    if rec10.requires_grad:
        rec10.retain_grad()
    img, D = blend(rec10, cam, dec, idx)
    return img, D, rec10


def gradients(cloud_np, sh_degree, cam, dec, G, G_D, antialiased=False, dtype=torch.float64, round_records=True):
    """The gradients of sum(image * G) + sum(D * G_D) to the six arrays (flat float64 numpy arrays keyed like the
    cloud), under "records" to the nine record values of every Gaussian (n, 9), under "depth" to its record depth (n);
    plus "image" and "D".  G None: all zero."""
    cloud = GR.as_tensors(cloud_np, dtype)
    img, D, rec10 = forward(cloud, sh_degree, cam, dec, antialiased, round_records)
    loss = (D * torch.as_tensor(np.asarray(G_D, dtype=np.float32)).to(dtype)).sum()
    if G is not None:
        loss = loss + (img * torch.as_tensor(np.asarray(G, dtype=np.float32)).to(dtype)).sum()
    loss.backward()
    out = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).to(torch.float64).numpy() for k, t in cloud.items()}
    rg = np.zeros((dec["visible"].size, 10))
    if rec10.grad is not None:
        rg[np.nonzero(dec["visible"])[0]] = rec10.grad.to(torch.float64).numpy()
    out["records"] = rg[:, :9].copy()
    out["depth"] = rg[:, 9].copy()
    out["image"] = img.detach().to(torch.float64).numpy()
    out["D"] = D.detach().to(torch.float64).numpy()
    return out


def depth_loss(depth, image, target, weight=None, kind="l1", min_alpha=0.5, scale=1.0):
    """The depth loss of the contract from float32 arrays (float64 ones, for central differences, are taken as they
    are): depth (H, W, 2) or (H, W) = D, image (H, W, 4) or (H, W) = alpha, target (H, W), weight None or (H, W).
    Returns a dict: L, W_v (floats), valid (bool), e, g_depth, g_alpha (float64, (H, W); the gradients not yet rounded
    to float32)."""
    D = np.asarray(depth)
    D = (D[..., 0] if D.ndim == 3 else D)
    al = np.asarray(image)
    al = (al[..., 3] if al.ndim == 3 else al)
    t = np.asarray(target)
    if weight is None:
        w = np.ones(t.shape, dtype=np.float32)
    else:
        w = np.asarray(weight)
        w = np.where(w > 0, np.minimum(w, 1.0), 0.0).astype(w.dtype)  # NaN -> 0
    with np.errstate(invalid="ignore"):
        valid = (w > 0) & np.isfinite(t) & (t > 0) & (al >= np.float32(min_alpha)) & np.isfinite(D) & (D > 0)
    D64, a64, t64, w64 = (x.astype(np.float64) for x in (D, al, t, w))
    e = np.zeros(t.shape)
    with np.errstate(all="ignore"):
        if kind == "l1":
            e[valid] = D64[valid] / a64[valid] - t64[valid]
        elif kind == "inverse":
            e[valid] = a64[valid] / D64[valid] - 1.0 / t64[valid]
        else:
            raise ValueError(kind)
    Wv = math.fsum(w64[valid].tolist())
    gD, gA = np.zeros(t.shape), np.zeros(t.shape)
    if Wv == 0.0:
        return {"L": 0.0, "W_v": 0.0, "valid": valid, "e": e, "g_depth": gD, "g_alpha": gA}
    L = math.fsum((w64[valid] * np.abs(e[valid])).tolist()) / Wv
    s = np.where(valid, scale * np.sign(e) * w64 / Wv, 0.0)
    with np.errstate(all="ignore"):
        if kind == "l1":
            gD[valid] = s[valid] / a64[valid]
            gA[valid] = -s[valid] * D64[valid] / (a64[valid] * a64[valid])
        else:
            gD[valid] = -s[valid] * a64[valid] / (D64[valid] * D64[valid])
            gA[valid] = s[valid] / D64[valid]
    return {"L": L, "W_v": Wv, "valid": valid, "e": e, "g_depth": gD, "g_alpha": gA}


# ---- the loop of "refine images with depth" ------------------------------------------------------------------------

FIT_SEED, FIT_COORD, FIT_W, FIT_H = 6, 6, 40, 36  # the 300-Gaussian SH0 scene; RDF


def torch_depth_loss(D, alpha, target, kind="l1", min_alpha=0.5):
    """The unweighted depth loss of torch tensors D and alpha (in a graph) against a float32 target array: the validity
    is decided from the detached values and held constant.  A 0-d tensor; 0 when no pixel is valid."""
    t = torch.as_tensor(np.asarray(target, dtype=np.float32)).to(D.dtype)
    with torch.no_grad():
        valid = torch.isfinite(t) & (t > 0) & (alpha >= float(np.float32(min_alpha))) & torch.isfinite(D) & (D > 0)
    if not bool(valid.any()):
        return (D * 0.0).sum()
    Dv, av, tv = D[valid], alpha[valid], t[valid]
    e = Dv / av - tv if kind == "l1" else av / Dv - 1.0 / tv
    return torch.abs(e).sum() / float(valid.sum())


def fit_scene(noise):
    """B (the scene), A (B with its positions moved by seeded Gaussian noise of size `noise`), both packed by the CPU
    oracle from the RDF frame, two orbit views at 40 x 36, and per view B's render and its expected depth where alpha >=
    0.5 (+inf elsewhere), float32, both from the float64 references over B's decoded floats."""
    import depth_ref as DR
    import render_ref as RR
    import spz_amd.spz as spz
    from oracle.pyoracle import Oracle
    O = Oracle()
    b = GR.scene(FIT_SEED, 0)
    n = b["alphas"].size
    a = {k: v.copy() for k, v in b.items()}
    rng = np.random.default_rng(21)
    a["positions"] = (a["positions"] + noise * rng.standard_normal(a["positions"].size)).astype(np.float32)
    p = b["positions"].reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    views = spz.orbit_views(2, width=FIT_W, height=FIT_H, fov_y=50.0, center=centre.tolist(), radius=radius)
    s = {"n": n, "a": O.pack(a, n, 0, False, FIT_COORD), "b": O.pack(b, n, 0, False, FIT_COORD), "views": views,
         "oracle": O}
    s["cams"] = [RR.camera(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], FIT_W, FIT_H, 0.2,
                           (0, 0, 0), 3) for v in views]
    _, tb = O.unpack(s["b"], FIT_COORD)
    tb = {k: tb[k] for k in ("positions", "scales", "rotations", "alphas", "colors", "sh")}
    s["images"], s["depths"] = [], []
    for cam in s["cams"]:
        s["images"].append(RR.render(tb, 0, cam).astype(np.float32))
        maps = DR.render_depth(tb, 0, cam)
        s["depths"].append(np.where(maps["alpha"] >= 0.5, DR.expected(maps), np.inf).astype(np.float32))
    return s


def depth_errors(cloud, s):
    """Per view, the unweighted L1 depth loss of the cloud's float64 depth render against the view's map."""
    import depth_ref as DR
    out = []
    for cam, t in zip(s["cams"], s["depths"]):
        maps = DR.render_depth(cloud, 0, cam)
        out.append(depth_loss(maps["accumulated"], maps["alpha"], t)["L"])
    return out


def float32_forward_error(s):
    """Per view, |L32 - L64| / L64 of A's depth error before the loop: forward() in float32 and in float64 with the
    same decisions.  What a float32 blend may be off by through no fault of its own."""
    keys = ("positions", "scales", "rotations", "alphas", "colors", "sh")
    _, cloud = s["oracle"].unpack(s["a"], FIT_COORD)
    cloud = {k: cloud[k] for k in keys}
    out = []
    for cam, t in zip(s["cams"], s["depths"]):
        dec = GR.decisions(cloud, 0, cam)
        L = []
        for dt in (torch.float64, torch.float32):
            with torch.no_grad():
                img, D, _ = forward(GR.as_tensors(cloud, dt, requires_grad=False), 0, cam, dec)
            L.append(depth_loss(D.numpy(), img[..., 3].numpy(), t)["L"])
        out.append(abs(L[1] - L[0]) / L[0])
    return out


def fit_loop(s, iterations, lr_positions, depth_weight, lambda_dssim=0.2):
    """The loop on the CPU from A's decoded floats, positions trained alone: per iteration fresh decisions, forward()
    in float64, loss_ref's image loss plus depth_weight times torch_depth_loss, autograd, loss_ref.adam_step.  Returns a
    dict: history, depth_history, before and after (per view depth errors; after: of the cloud packed and decoded
    again, as the output stream is)."""
    import loss_ref as LR
    O = s["oracle"]
    keys = ("positions", "scales", "rotations", "alphas", "colors", "sh")
    _, cloud = O.unpack(s["a"], FIT_COORD)
    cloud = {k: cloud[k] for k in keys}
    before = depth_errors(cloud, s)
    m, v = np.zeros_like(cloud["positions"]), np.zeros_like(cloud["positions"])
    history, depth_history = [], []
    for i in range(iterations):
        k = i % len(s["cams"])
        cam = s["cams"][k]
        dec = GR.decisions(cloud, 0, cam)
        t = GR.as_tensors(cloud, torch.float64)
        img, D, _ = forward(t, 0, cam, dec)
        photo = LR.loss_terms(img, s["images"][k], lambda_dssim)[0]
        depth = torch_depth_loss(D, img[..., 3], s["depths"][k])
        (photo + depth_weight * depth).backward()
        history.append(float(photo.detach()) + depth_weight * float(depth.detach()))
        depth_history.append(float(depth.detach()))
        g = t["positions"].grad.numpy().astype(np.float32)
        cloud["positions"], m, v, _ = LR.adam_step(cloud["positions"], g, m, v, i + 1, lr_positions)
    _, out = O.unpack(O.pack(cloud, s["n"], 0, False, FIT_COORD), FIT_COORD)
    return {"history": history, "depth_history": depth_history, "before": before,
            "after": depth_errors({k: out[k] for k in keys}, s)}


if __name__ == "__main__":
    # Writes tests/golden/depth_fit_expected.json: the inputs' sizes and what the reference loop gives with the depth
    # term and with weight 0.  Two conditions on the inputs, both checked here, on the CPU, before the file is written.
    # (1) The reference alone brings the mean depth error to at most half of its start within 120 iterations.
    # (2) The device's first losses are asked to be within 1e-6 relative of this float64 reference, and the device
    # blends in float32.  The same forward in float32 is off by 0.5e-7 to 3.1e-7 ABSOLUTE in a view's depth error,
    # whatever the noise (0.25 to 1.0 tried; it does not average out over the view's 720 pixels), so the noise is the
    # smallest of 0.25, 0.3, 0.35, 0.4, 0.5, 0.6, 0.7, 0.85, 1.0 whose depth error, about 0.69 times the noise, leaves
    # 1e-6 of it at least twice that 3.1e-7: 1.0 (0.703 and 0.682).  Asserted below for the noise chosen: the float32
    # forward is within 0.5e-6 relative in both views.
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    noise, iterations, lr = 1.0, 120, 3e-2
    if len(sys.argv) == 4:  # try other inputs: noise, iterations, rate
        noise, iterations, lr = float(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3])
    scene = fit_scene(noise)
    f32_error = float32_forward_error(scene)
    print("float32 forward, relative error of the depth error before:", f32_error)
    assert max(f32_error) <= 0.5e-6
    with_depth = fit_loop(scene, iterations, lr, 1.0)
    without = fit_loop(scene, iterations, lr, 0.0)
    print("with depth:", with_depth["before"], "->", with_depth["after"], "history", with_depth["history"][0], "->",
          with_depth["history"][-1])
    print("weight 0:  ", without["before"], "->", without["after"])
    assert iterations <= 120 and np.mean(with_depth["after"]) <= 0.5 * np.mean(with_depth["before"])
    expected = {"noise": noise, "iterations": iterations, "lr_positions": lr, "depth_weight": 1.0, "depth_kind": "l1",
                "float32_forward_error": f32_error, "with_depth": with_depth, "weight_0": without}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_fit_expected.json")
    with open(path, "w") as f:
        json.dump(expected, f, indent=1)
        f.write("\n")
