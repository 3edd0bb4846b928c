"""The gradient of a view to its camera and the pose fit on the CPU (include/spz_amd.h "render view backward" and
"locate"; DESIGN §8 "Locate").

The gradient: tests/render_grad_ref.py's forward with the camera's R and t as torch leaves, differentiated by
autograd.  The discrete decisions come from a numpy copy of the same camera (render_grad_ref.decisions) and are
constants, whatever the dtype.  R enters through p_c = R p + t, through T = J R and through the camera centre -R^T t of
the view direction; render_grad_ref.records takes all three from cam["R"] and cam["t"].

The update: numpy restatements of the twist gradient, Adam over the six twist values, Exp of so(3), the step-size
schedule, the level intrinsics and the box mean, as the header words them; locate() runs the whole loop with the
decisions recomputed every iteration."""
import numpy as np
import torch

import loss_ref as LR
import render_grad_ref as GR
import render_ref as RR


def torch_camera(cam, dtype, requires_grad=True):
    """cam with R and t as leaves of `dtype` (the other entries shared)."""
    out = dict(cam)
    out["R"] = torch.as_tensor(np.asarray(cam["R"], dtype=np.float64)).to(dtype).clone().requires_grad_(requires_grad)
    out["t"] = torch.as_tensor(np.asarray(cam["t"], dtype=np.float64)).to(dtype).clone().requires_grad_(requires_grad)
    return out


def pack(gR, gt):
    """[G_R | G_t] as a (3, 4) float64 array."""
    return np.concatenate([gR.to(torch.float64).numpy(), gt.to(torch.float64).numpy()[:, None]], axis=1)


def view_gradient(cloud_np, sh_degree, cam, dec, G, antialiased=False, dtype=torch.float64, round_records=True):
    """The gradients of sum(image * G): "view" (3, 4) = [dL/dR | dL/dt], "records" (n, 9; zero rows for the invisible
    Gaussians) and "image", as float64 numpy arrays."""
    cloud = GR.as_tensors(cloud_np, dtype, requires_grad=False)
    tc = torch_camera(cam, dtype)
    img, rec9 = GR.forward(cloud, sh_degree, tc, dec, antialiased, round_records)
    (img * torch.as_tensor(np.asarray(G, dtype=np.float32)).to(dtype)).sum().backward()
    rg = np.zeros((dec["visible"].size, 9))
    if rec9.grad is not None:
        rg[np.nonzero(dec["visible"])[0]] = rec9.grad.to(torch.float64).numpy()
    return {"view": pack(tc["R"].grad, tc["t"].grad), "records": rg, "image": img.detach().to(torch.float64).numpy()}


def chain(cloud_np, sh_degree, cam, dec, record_grads, antialiased=False, dtype=torch.float64, forward_mode=False):
    """The chain from given record gradients (n, 9) to the camera alone: (n, 3, 4) float64, each Gaussian's 12
    contributions (zero for the invisible ones).  Their sum over n is the view gradient for those record gradients.
    forward_mode: the same derivatives by 12 forward-mode passes, one per camera entry over all the Gaussians at once,
    where one backward pass per Gaussian (n of them, each through all n rows) would take too long."""
    cloud = GR.as_tensors(cloud_np, dtype, requires_grad=False)
    idx = np.nonzero(dec["visible"])[0]
    w = torch.as_tensor(np.asarray(record_grads, dtype=np.float64)[idx]).to(dtype)
    out = np.zeros((dec["visible"].size, 3, 4))
    if forward_mode:
        import torch.autograd.forward_ad as fwd
        base = torch_camera(cam, dtype, requires_grad=False)
        for a in range(3):
            for b in range(4):
                dR, dt = torch.zeros(3, 3, dtype=dtype), torch.zeros(3, dtype=dtype)
                (dR[a] if b < 3 else dt)[b if b < 3 else a] = 1.0
                with fwd.dual_level():
                    tc = dict(base, R=fwd.make_dual(base["R"], dR), t=fwd.make_dual(base["t"], dt))
                    tangent = fwd.unpack_dual(GR.records(cloud, sh_degree, tc, idx, antialiased)).tangent
                    out[idx, a, b] = (tangent * w).sum(dim=1).to(torch.float64).numpy()
        return out
    tc = torch_camera(cam, dtype)
    rec9 = GR.records(cloud, sh_degree, tc, idx, antialiased)
    per = (rec9 * w).sum(dim=1)
    for k, i in enumerate(idx):
        gR, gt = torch.autograd.grad(per[k], (tc["R"], tc["t"]), retain_graph=True)
        out[i] = pack(gR, gt)
    return out


# ---- the update, restated

def so3_exp(w):
    """Exp of so(3) by Rodrigues' formula; below |w| = 1e-4 the series of sin t / t and (1 - cos t) / t^2."""
    w = np.asarray(w, dtype=np.float64)
    t2 = float(w @ w)
    if t2 < 1e-8:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        t = np.sqrt(t2)
        A, B = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * K + B * (K @ K)


def twist_gradient(pose, view_grad):
    """The gradient to (w, v) of L(Exp(w) R, Exp(w) t + v) at 0 from [G_R | G_t]: A = G_R R^T + G_t t^T."""
    pose, g = np.asarray(pose, dtype=np.float64), np.asarray(view_grad, dtype=np.float64)
    A = g[:, :3] @ pose[:, :3].T + np.outer(g[:, 3], pose[:, 3])
    return np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1], g[0, 3], g[1, 3], g[2, 3]])


DEFAULTS = {"iterations": 300, "levels": 1, "lambda_dssim": 0.2, "lr_rotation": 2e-3, "lr_translation": 2e-3,
            "lr_final_factor": 0.1, "beta1": 0.9, "beta2": 0.999, "eps": 1e-15}


def pose_step(opts, i, g, m, v, pose):
    """One update for iteration i: (pose', m', v'), float64."""
    o = dict(DEFAULTS, **opts)
    f = o["lr_final_factor"] ** (i / o["iterations"])
    b1, b2 = o["beta1"], o["beta2"]
    g = np.asarray(g, dtype=np.float64)
    m = b1 * np.asarray(m, dtype=np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, dtype=np.float64) + (1.0 - b2) * g * g
    lr = np.array([o["lr_rotation"]] * 3 + [o["lr_translation"]] * 3) * f
    with np.errstate(all="ignore"):
        d = -lr * (m / (1.0 - b1 ** (i + 1))) / (np.sqrt(v / (1.0 - b2 ** (i + 1))) + o["eps"])
    d = np.where(m == 0.0, 0.0, d)
    E = so3_exp(d[:3])
    pose = np.asarray(pose, dtype=np.float64)
    return np.concatenate([E @ pose[:, :3], (E @ pose[:, 3] + d[3:])[:, None]], axis=1), m, v


def level_camera(cam, k):
    """The camera of level k: the size and fx, fy, cx, cy divided by 2^k."""
    f = 2 ** k
    assert cam["width"] % f == 0 and cam["height"] % f == 0
    out = dict(cam)
    out.update(width=cam["width"] // f, height=cam["height"] // f, fx=cam["fx"] / f, fy=cam["fy"] / f,
               cx=cam["cx"] / f, cy=cam["cy"] / f)
    return out


def box_mean(img):
    """The 2 x 2 box mean of a float32 (H, W, C) image, in float32, in the kernel's order."""
    a = np.asarray(img, dtype=np.float32)
    return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * np.float32(0.25)


def with_pose(cam, pose):
    """cam at the float64 pose rounded to float32, as the params carry it."""
    p = np.asarray(pose, dtype=np.float64).astype(np.float32).astype(np.float64)
    out = dict(cam)
    out["R"], out["t"] = p[:, :3].copy(), p[:, 3].copy()
    return out


def level_schedule(iterations, levels):
    """[(level, first iteration, one past the last)] from the coarsest level down; the remainder goes to level 0."""
    per, out, i = iterations // levels, [], 0
    for k in range(levels - 1, -1, -1):
        until = iterations if k == 0 else i + per
        out.append((k, i, until))
        i = until
    return out


def locate(cloud_np, sh_degree, cam, target, antialiased=False, **opts):
    """The pose fit from cam's pose against target (H, W, 3 or 4, float32): dict(pose (3, 4) float64, history, poses:
    the pose before each step)."""
    o = dict(DEFAULTS, **opts)
    pose = np.concatenate([cam["R"], cam["t"][:, None]], axis=1).astype(np.float64)
    m, v, history, poses = np.zeros(6), np.zeros(6), [], []
    cloud = GR.as_tensors(cloud_np, torch.float64, requires_grad=False)
    targets = [np.asarray(target, dtype=np.float32)]
    for _ in range(1, o["levels"]):
        targets.append(box_mean(targets[-1]))
    for k, first, until in level_schedule(o["iterations"], o["levels"]):
        for i in range(first, until):
            c = with_pose(level_camera(cam, k), pose)
            dec = GR.decisions(cloud_np, sh_degree, c, antialiased)
            tc = torch_camera(c, torch.float64)
            img, _ = GR.forward(cloud, sh_degree, tc, dec, antialiased)
            L = LR.loss_terms(img, targets[k], o["lambda_dssim"])[0]
            L.backward()
            G = pack(tc["R"].grad, tc["t"].grad)
            if not np.isfinite(G).all():
                return {"pose": pose, "history": history, "poses": poses}
            history.append(float(L.detach()))
            poses.append(pose)
            pose, m, v = pose_step(o, i, twist_gradient(pose, G), m, v, pose)
    return {"pose": pose, "history": history, "poses": poses}


def perturbed(m, degrees, fraction, seed=0):
    """The (3, 4) pose m with the camera rotated by `degrees` about a random axis and moved by `fraction` of |t| in a
    random direction: float32, as a params matrix."""
    rng = np.random.default_rng(seed)
    m = np.asarray(m, dtype=np.float64).reshape(3, 4)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    step = rng.standard_normal(3)
    step /= np.linalg.norm(step)
    E = so3_exp(np.deg2rad(degrees) * axis)
    t = E @ m[:, 3] + fraction * np.linalg.norm(m[:, 3]) * step
    return np.concatenate([E @ m[:, :3], t[:, None]], axis=1).astype(np.float32)


def pose_errors(pose, truth):
    """(rotation error in degrees, camera-centre error as a fraction of the true |t|) of two (3, 4) poses."""
    a, b = np.asarray(pose, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    cosang = (np.trace(a[:, :3] @ b[:, :3].T) - 1.0) / 2.0
    ca, cb = -a[:, :3].T @ a[:, 3], -b[:, :3].T @ b[:, 3]
    return float(np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))), float(np.linalg.norm(ca - cb) / np.linalg.norm(b[:, 3]))
