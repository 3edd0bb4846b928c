"""The derivative of the render contract on the CPU (include/spz_amd.h "render backward"; DESIGN §8 "Render backward"):
tests/render_ref.py's arithmetic written with torch operations in a chosen dtype, differentiated by autograd.

The discrete decisions are not torch's to make.  decisions() computes them once in float64 with render_ref (the visible
set, the tile rectangles, the depth order and, per pixel, the used pairs up to the stop) and forward() takes them as
constants, whatever its dtype.  The records are rounded to float32 with a straight-through gradient, as the device
stores them.  The clamps (alpha at 0.99, rgb at 0, the quotients of J) are torch.clamp's: no gradient where they clamp.

decisions() also counts the marginal pairs: considered pairs whose float64 value lies within a relative 1e-4 of a
decision threshold, which a float32 blend might decide the other way."""
import numpy as np
import torch

import render_ref as RR

BAND = RR.BAND


def _walk(rec, sel, u, v):
    """render_ref._blend over the Gaussians sel at the pixels (u, v), keeping the decisions: take (pixels, len(sel))
    bool, the used pairs; the marginal pairs per pixel (pixels, int); and the counts (stopped pixels, clamped-alpha
    pairs)."""
    T = np.ones(u.shape)
    live = np.ones(u.shape, dtype=bool)
    mean = rec["mean"].astype(np.float64)
    conic = rec["conic"].astype(np.float64)
    op = rec["opacity"].astype(np.float64)
    take_all = np.zeros(u.shape + (len(sel),), dtype=bool)
    marginal = np.zeros(u.shape, dtype=np.int64)
    clamped = 0
    for k, g in enumerate(sel):
        if not live.any():
            break
        dx, dy = u - mean[g, 0], v - mean[g, 1]
        A, B, Cc = conic[g]
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        raw = op[g] * np.exp(np.minimum(power, 0.0))
        a = np.minimum(0.99, raw)
        neg = live & (power <= 0)
        take = neg & (a >= 1.0 / 255.0)
        Tn = T * (1.0 - a)
        m = live & (np.abs(power) < 1e-6)
        m |= neg & (np.abs(255.0 * a - 1.0) < BAND)
        m |= neg & (np.abs(raw / 0.99 - 1.0) < BAND)
        m |= take & (np.abs(Tn / 1e-4 - 1.0) < BAND)
        marginal += m
        stop = take & (Tn < 1e-4)
        live &= ~stop
        take &= ~stop
        clamped += int((take & (raw > 0.99)).sum())
        take_all[:, k] = take
        T = np.where(take, Tn, T)
    return take_all, marginal, int((~live).sum()), clamped


def _walk_vec(rec, sel, u, v):
    """_walk through render_ref.walk (vectorised over the list as well): the same four results, for long lists."""
    wk = RR.walk(rec, sel, u, v)
    return np.ascontiguousarray(wk["take"].T), wk["marginal"], int(wk["stopped"].sum()), wk["clamped"]


def decisions(cloud, sh_degree, cam, antialiased=False, vectorised=False):
    """The constants of forward(): visible (n bool), and per tile the Gaussians in blend order, the pixels, the used
    pairs and each pixel's number of marginal pairs; plus the scene's counts: entries, used, stopped (pixels), clamped
    (alpha pairs), marginal (pairs), and marginal_mask (H, W bool): the pixels with a marginal pair.  vectorised: walk
    each tile with _walk_vec, which gives the same decisions faster on lists of hundreds of entries."""
    rec = RR.preprocess(cloud, sh_degree, cam, antialiased)
    W, H = cam["width"], cam["height"]
    tw, th = RR.tiles(cam)
    order = RR.depth_order(rec)
    r = rec["rect"][order]
    out = {"visible": rec["visible"].copy(), "tiles": [], "entries": RR.entry_count(rec), "used": 0, "stopped": 0,
           "clamped": 0, "marginal": 0, "marginal_mask": np.zeros((H, W), dtype=bool), "rec": rec}
    for ty in range(th):
        for tx in range(tw):
            sel = order[(r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])]
            vv, uu = np.mgrid[ty * RR.TILE:min(H, ty * RR.TILE + RR.TILE), tx * RR.TILE:min(W, tx * RR.TILE + RR.TILE)]
            uu, vv = uu.ravel(), vv.ravel()
            take, marginal, stopped, clamped = (_walk_vec if vectorised else _walk)(
                rec, sel, uu.astype(np.float64), vv.astype(np.float64))
            out["tiles"].append({"sel": sel, "u": uu, "v": vv, "take": take, "marginal": marginal})
            out["used"] += int(take.sum())
            out["stopped"] += stopped
            out["clamped"] += clamped
            out["marginal"] += int(marginal.sum())
            out["marginal_mask"][vv, uu] = marginal > 0
    return out


def _sh_colour(col, sh, degree, d):
    x, y, z = (d[:, k:k + 1] for k in range(3))
    C1, C2, C3 = RR.C1, RR.C2, RR.C3
    r = RR.C0 * col
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
    return torch.clamp(r + 0.5, min=0.0)


def records(cloud, sh_degree, cam, idx, antialiased=False):
    """render_ref.preprocess for the Gaussians idx (the visible ones) in the dtype of the cloud's tensors: (len(idx), 9)
    = mean 2, conic 3, opacity 1, rgb 3, not rounded."""
    dt = cloud["positions"].dtype
    n = cloud["alphas"].numel()
    idx = torch.as_tensor(idx, dtype=torch.int64)
    R, t = cam["R"], cam["t"]
    P = cloud["positions"].reshape(n, 3)[idx]
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    x = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + t[0]
    y = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + t[1]
    z = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + t[2]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    W, H = float(cam["width"]), float(cam["height"])
    mx = fx * x / z + cx - 0.5
    my = fy * y / z + cy - 0.5
    q = cloud["rotations"].reshape(n, 4)[idx]
    q = q / torch.sqrt((q * q).sum(dim=1))[:, None]
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    Rq = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                      2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                      2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], dim=1)
    Rq = Rq.reshape(-1, 3, 3)
    s = torch.exp(cloud["scales"].reshape(n, 3)[idx])
    M = Rq * s[:, None, :]
    S = M @ M.transpose(1, 2)
    lxp, lxn = (W - cx) / fx + 0.3 * W / fx, cx / fx + 0.3 * W / fx
    lyp, lyn = (H - cy) / fy + 0.3 * H / fy, cy / fy + 0.3 * H / fy
    tx = z * torch.clamp(x / z, -lxn, lxp)
    ty = z * torch.clamp(y / z, -lyn, lyp)
    Rt = torch.as_tensor(R, dtype=dt)
    T0 = (fx / z)[:, None] * Rt[0][None, :] + (-(fx * tx) / (z * z))[:, None] * Rt[2][None, :]
    T1 = (fy / z)[:, None] * Rt[1][None, :] + (-(fy * ty) / (z * z))[:, None] * Rt[2][None, :]
    T = torch.stack([T0, T1], dim=1)
    cov = T @ S @ T.transpose(1, 2)
    a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    det0 = a * c - b * b
    a, c = a + 0.3, c + 0.3
    det = a * c - b * b
    op = 1.0 / (1.0 + torch.exp(-cloud["alphas"][idx]))
    if antialiased:
        pos = det0 > 0  # sqrt(max(0, det0) / det): zero, with a zero derivative, where det0 <= 0
        op = op * torch.where(pos, torch.sqrt(torch.where(pos, det0, torch.ones_like(det0)) / det),
                              torch.zeros_like(det0))
    campos = torch.as_tensor(-(R.T @ t), dtype=dt)
    d = P - campos[None, :]
    d = d / torch.sqrt((d * d).sum(dim=1))[:, None]
    D = RR.SH_DIM[sh_degree]
    sh = cloud["sh"].reshape(n, D, 3)[idx] if D else None
    rgb = _sh_colour(cloud["colors"].reshape(n, 3)[idx], sh, min(sh_degree, cam["max_sh_degree"]), d)
    return torch.cat([mx[:, None], my[:, None], (c / det)[:, None], (-b / det)[:, None], (a / det)[:, None],
                      op[:, None], rgb], dim=1)


def blend(rec9, cam, dec, idx):
    """render_ref's blend of the records rec9 (rows: the Gaussians idx) with the used pairs of dec: (H, W, 4)."""
    dt = rec9.dtype
    W, H = cam["width"], cam["height"]
    row = np.full(dec["visible"].size, -1, dtype=np.int64)
    row[np.asarray(idx)] = np.arange(len(idx))
    bg = torch.as_tensor(cam["background"], dtype=dt)
    img = torch.zeros((H, W, 4), dtype=dt)
    for tile in dec["tiles"]:
        u, v = torch.as_tensor(tile["u"]), torch.as_tensor(tile["v"])
        if len(tile["sel"]) == 0:
            img[v, u] = torch.cat([bg, torch.zeros(1, dtype=dt)])[None, :].expand(u.numel(), 4)
            continue
        m = rec9[torch.as_tensor(row[tile["sel"]])]
        take = torch.as_tensor(tile["take"])
        dx = u.to(dt)[:, None] - m[None, :, 0]
        dy = v.to(dt)[:, None] - m[None, :, 1]
        power = -0.5 * (m[None, :, 2] * dx * dx + m[None, :, 4] * dy * dy) - m[None, :, 3] * dx * dy
        power = torch.where(take, power, torch.zeros_like(power))  # an unused pair's exp may overflow
        a = torch.clamp(m[None, :, 5] * torch.exp(power), max=0.99)
        a = torch.where(take, a, torch.zeros_like(a))
        through = torch.cumprod(1.0 - a, dim=1)
        T = torch.cat([torch.ones_like(through[:, :1]), through[:, :-1]], dim=1)
        C = (T * a) @ m[:, 6:9]
        Tf = through[:, -1]
        img[v, u] = torch.cat([C + Tf[:, None] * bg[None, :], (1.0 - Tf)[:, None]], dim=1)
    return img


def forward(cloud, sh_degree, cam, dec, antialiased=False, round_records=True):
    """(image (H, W, 4), rec9) in the dtype of the cloud's tensors (dict of flat torch tensors).  rec9: the visible
    Gaussians' nine record values as the blend read them, in the graph (retain_grad() gives their gradients)."""
    idx = np.nonzero(dec["visible"])[0]
    rec9 = records(cloud, sh_degree, cam, idx, antialiased)
    if round_records:
        rec9 = rec9 + (rec9.detach().to(torch.float32).to(rec9.dtype) - rec9.detach())  # straight through
    if rec9.requires_grad:
        rec9.retain_grad()
    return blend(rec9, cam, dec, idx), rec9


def as_tensors(cloud_np, dtype, requires_grad=True):
    out = {}
    for k, a in cloud_np.items():
        t = torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype).clone()
        out[k] = t.requires_grad_(requires_grad)
    return out


def gradients(cloud_np, sh_degree, cam, dec, G, antialiased=False, dtype=torch.float64, round_records=True):
    """The gradients of sum(image * G) to the six arrays (flat float64 numpy arrays keyed like the cloud) and, under
    "records", to the nine record values of every Gaussian (n, 9; zero rows for the invisible ones); plus "image"."""
    cloud = as_tensors(cloud_np, dtype)
    img, rec9 = forward(cloud, sh_degree, cam, dec, antialiased, round_records)
    (img * torch.as_tensor(np.asarray(G, dtype=np.float32)).to(dtype)).sum().backward()
    out = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).to(torch.float64).numpy() for k, t in cloud.items()}
    rg = np.zeros((dec["visible"].size, 9))
    if rec9.grad is not None:
        rg[np.nonzero(dec["visible"])[0]] = rec9.grad.to(torch.float64).numpy()
    out["records"] = rg
    out["image"] = img.detach().to(torch.float64).numpy()
    return out


def scene(seed, sh_degree, n=300, clamp_hits=0):
    """The test scene: make_cloud_numpy(n, sh_degree, seed) with scales * 0.25 + 1.5 and alphas * 0.5 + 1.0 (2D sizes of
    a few pixels at 40 x 36, opacities around 0.7).  clamp_hits more Gaussians with alpha = +8 around the centre of the
    view of test_gpu_render.view_of, halfway to its eye (in front of the crowd, where T is still near 1) and about five
    pixels wide, so that a = min(0.99, .) clamps at the pixels next to their centres."""
    from spz_amd.synth import make_cloud_numpy
    c = make_cloud_numpy(n, sh_degree, seed)
    c["scales"] = (c["scales"] * 0.25 + 1.5).astype(np.float32)
    c["alphas"] = (c["alphas"] * 0.5 + 1.0).astype(np.float32)
    if clamp_hits:
        e = make_cloud_numpy(clamp_hits, sh_degree, seed + 1000)
        p = c["positions"].reshape(-1, 3).astype(np.float64)
        lo, hi = np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)
        ext = float(max(hi - lo))
        at = 0.5 * (lo + hi) + 0.5 * ext * np.array([0.3, 0.2, -2.2])
        e["positions"] = (at[None, :] + 0.3 * e["positions"].reshape(-1, 3)).astype(np.float32).reshape(-1)
        e["scales"] = (e["scales"] * 0.05 + 1.4).astype(np.float32)
        e["alphas"] = np.full(clamp_hits, 8.0, np.float32)
        c = {k: np.concatenate([c[k], e[k]]) for k in c}
    return c
