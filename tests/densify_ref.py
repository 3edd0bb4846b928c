"""numpy restatement of the densify primitives (include/spz_amd.h "densify"; DESIGN §8 "Densify"): the thresholds, the
gradient statistic, the plan, the apply with its counter-based normals, and the opacity reset.  float32 where the
contract says float32 (each operation rounded once), float64 for the split children's positions."""
import math

import numpy as np

F = np.float32
M64 = (1 << 64) - 1
KEEP, CLONE, SPLIT, CULL = 0, 1, 2, 3
WIDTHS = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3}
ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")


def width(k, sh_degree):
    return WIDTHS[k] if k != "sh" else 3 * {0: 0, 1: 3, 2: 8, 3: 15}[sh_degree]


def camera_centres(views):
    """c = -R^T t per view (world_to_camera rows as float32 values widened), each sum left to right in float64."""
    out = []
    for w2c in views:
        m = np.asarray(w2c, dtype=np.float32).astype(np.float64).reshape(3, 4)
        out.append([-(m[0, k] * m[0, 3] + m[1, k] * m[1, 3] + m[2, k] * m[2, 3]) for k in range(3)])
    return out


def derived_extent(views):
    """3DGS's cameras_extent: 1.1 max |c_v - mean c|."""
    c = camera_centres(views)
    mean = [0.0, 0.0, 0.0]
    for cv in c:
        for k in range(3):
            mean[k] += cv[k]
    mean = [x / float(len(c)) for x in mean]
    far = 0.0
    for cv in c:
        dx, dy, dz = cv[0] - mean[0], cv[1] - mean[1], cv[2] - mean[2]
        far = max(far, math.sqrt(dx * dx + dy * dy + dz * dz))
    return 1.1 * far


def thresholds(grad_threshold=2e-4, percent_dense=0.01, extent=0.0, min_opacity=0.005, max_scale=0.0, views=()):
    """The limits as float32 (None when the extent cannot be derived): float64 libm values rounded once."""
    if extent == 0.0:
        if not len(views):
            return None
        extent = derived_extent(views)
        if not extent > 0.0:
            return None
    return {"extent": extent, "grad_threshold": F(grad_threshold), "log_dense": F(math.log(percent_dense * extent)),
            "alpha_min": F(math.log(min_opacity / (1.0 - min_opacity))), "use_max_scale": max_scale > 0.0,
            "log_max_scale": F(math.log(max_scale)) if max_scale > 0.0 else F(0.0)}


def accumulate(depth, record_grads, width_px, height_px, accum, denom):
    """New (accum, denom): for finite depth, accum += sqrt((gx W/2)^2 + (gy H/2)^2) in float32 (a non-finite norm adds
    0) and denom += 1."""
    g = np.asarray(record_grads, dtype=F).reshape(-1, 9)
    hw, hh = F(0.5) * F(width_px), F(0.5) * F(height_px)
    with np.errstate(all="ignore"):
        a, b = g[:, 0] * hw, g[:, 1] * hh
        norm = np.sqrt(a * a + b * b)
        vis = np.isfinite(np.asarray(depth, dtype=F))
        add = vis & np.isfinite(norm)
        out = accum.astype(F).copy()
        out[add] = out[add] + norm[add]
    den = denom.copy()
    den[vis] += 1
    return out, den


def plan(accum, denom, scales, alphas, lim, max_points):
    """(action[n], parent[n'], child[n'], counts dict) by the contract's rule."""
    n = int(np.asarray(alphas).size)
    accum, alphas = np.asarray(accum, dtype=F), np.asarray(alphas, dtype=F)
    s = np.asarray(scales, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ms = np.fmax(np.fmax(s[:, 0], s[:, 1]), s[:, 2]) if n else np.zeros(0, F)
        cull = alphas < lim["alpha_min"]
        if lim["use_max_scale"]:
            cull = cull | (ms > lim["log_max_scale"])
        den = np.asarray(denom).astype(np.int64)
        g = np.where(den > 0, accum / np.maximum(den, 1).astype(F), F(0.0)).astype(F)
        g = np.where(np.isnan(g), F(0.0), g)
        cand = ~cull & (g >= lim["grad_threshold"])
    action = np.zeros(n, np.uint8)
    action[cull] = CULL
    action[cand & (ms > lim["log_dense"])] = SPLIT
    action[cand & ~(ms > lim["log_dense"])] = CLONE
    culled = int(cull.sum())
    budget = max(0, int(max_points) - (n - culled))
    idx = np.nonzero(cand)[0]
    ranked = idx[np.argsort(-g[idx].astype(np.float64), kind="stable")]  # descending g, ties to the lower index
    refused = ranked[budget:]
    action[refused] = KEEP
    # input order, each Gaussian replaced by its outputs: keep -> 0; clone -> 0, 1; split -> 2, 3; cull -> nothing
    cnt = np.where(action == CULL, 0, np.where(action == KEEP, 1, 2)).astype(np.int64)
    parent = np.repeat(np.arange(n, dtype=np.int64), cnt)
    nth = np.arange(parent.size, dtype=np.int64) - (np.cumsum(cnt) - cnt)[parent]
    child = np.where(action[parent] == SPLIT, 2 + nth, nth)
    counts = {"num_points": int(parent.size), "cloned": int((action == CLONE).sum()),
              "split": int((action == SPLIT).sum()), "culled": culled, "refused": int(refused.size)}
    return action, parent.astype(np.uint32), child.astype(np.uint8), counts


def sm(x):
    """splitmix64 on a Python int."""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def normals(seed, rnd, i):
    """(z_2, z_3): the three standard normals of each split child of parent i in round rnd."""
    key = sm((sm((seed ^ rnd) & M64) + i) & M64)
    z2, z3 = [], []
    for j in range(3):
        a, b = sm((key + 2 * j + 1) & M64), sm((key + 2 * j + 2) & M64)
        u1, u2 = ((a >> 11) + 1) * 2.0 ** -53, (b >> 11) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        z2.append(r * math.cos(6.283185307179586 * u2))
        z3.append(r * math.sin(6.283185307179586 * u2))
    return z2, z3


def split_offset(scales3, quat4, z):
    """R(q / |q|) (exp(ls) (.) z) in float64 (NaN for a zero quaternion)."""
    q = np.asarray(quat4, dtype=np.float64)
    with np.errstate(all="ignore"):
        qx, qy, qz, qw = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        R = np.array([[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
                      [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
                      [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]])
        sz = np.exp(np.asarray(scales3, dtype=np.float64)) * np.asarray(z, dtype=np.float64)
        return np.array([R[r, 0] * sz[0] + R[r, 1] * sz[1] + R[r, 2] * sz[2] for r in range(3)])


def apply(cloud, m, v, sh_degree, parent, child, seed, rnd):
    """(cloud', m', v', offsets): the gather of the contract; offsets[k] is the float64 offset of a split child (zeros
    elsewhere), for the position margin."""
    n_new = int(parent.size)
    out = [{}, {}, {}]
    for k in ARRAYS:
        w = width(k, sh_degree)
        for j, src in enumerate((cloud, m, v)):
            a = np.asarray(src.get(k, np.zeros(0, F)), dtype=F).reshape(-1, w) if w else np.zeros((0, 0), F)
            out[j][k] = (a[parent].copy() if w else np.zeros((n_new, 0), F))
        if w:
            out[1][k][child != 0] = 0.0
            out[2][k][child != 0] = 0.0
    split = child >= 2
    out[0]["scales"][split] = out[0]["scales"][split] - F(math.log(1.6))
    offsets = np.zeros((n_new, 3))
    pos = np.asarray(cloud["positions"], dtype=F).reshape(-1, 3)
    sc = np.asarray(cloud["scales"], dtype=F).reshape(-1, 3)
    rot = np.asarray(cloud["rotations"], dtype=F).reshape(-1, 4)
    for k in np.nonzero(split)[0]:
        i = int(parent[k])
        z = normals(seed, rnd, i)[int(child[k]) - 2]
        off = split_offset(sc[i], rot[i], z)
        with np.errstate(all="ignore"):
            p = (pos[i].astype(np.float64) + off).astype(F)
        if np.isfinite(p).all():
            out[0]["positions"][k] = p
            offsets[k] = off
    flat = [{k: a.reshape(-1) for k, a in c.items()} for c in out]
    return flat[0], flat[1], flat[2], offsets


def reset_opacity(alphas, m, v):
    ceiling = F(math.log(0.01 / 0.99))
    a = np.asarray(alphas, dtype=F).copy()
    with np.errstate(invalid="ignore"):
        a[a > ceiling] = ceiling
    return a, np.zeros_like(m), np.zeros_like(v)
