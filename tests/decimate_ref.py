"""A float64 numpy restatement of the decimation contract (include/spz_amd.h "decimate", DESIGN §8 "Decimate"): cells,
level counts, parents, the moments of every cell and their encoding to bytes.  A helper module, not a test file:
tests/test_decimate_host.py checks it against the oracle and tests/test_gpu_decimate.py compares the device with it."""
import numpy as np

from test_filter_host import MAGIC, SH_DIM, parse_stream
from test_sort_host import morton_order, position_fields

LEVELS = 25
SCALE_MIN, SCALE_MAX = -10.0, 255.0 / 16.0 - 10.0   # what the scale byte can hold
EIG_FLOOR = np.exp(-20.0)


def round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def cell_u(stream):
    """u_a = stored field ^ 0x800000, (N, 3) int64, in file order."""
    return (position_fields(stream).astype(np.int64) ^ 0x800000)


def leave_bins(us):
    """For sorted u (N, 3): bin_i (i >= 1) = max_a msb(u_a ^ u'_a) = msb(Morton XOR) // 3, 24 when equal."""
    if us.shape[0] < 2:
        return np.zeros(0, np.int64)
    x = np.bitwise_or.reduce(us[1:] ^ us[:-1], axis=1)
    bins = np.full(x.shape, 24, np.int64)
    nz = x != 0
    bins[nz] = np.floor(np.log2(x[nz].astype(np.float64))).astype(np.int64)
    # exact bit length (log2 of a float could round up just below a power of two)
    b = bins[nz]
    b = np.where((np.int64(1) << b) > x[nz], b - 1, b)
    bins[nz] = b
    return bins


def level_counts(stream):
    """cells(L) for L = 0..24 (int64 array of 25)."""
    h = parse_stream(stream)
    n = h["num_points"]
    if n == 0:
        return np.zeros(LEVELS, np.int64)
    us = cell_u(stream)[morton_order(stream)]
    bins = leave_bins(us)
    return np.array([1 + int(np.count_nonzero((bins >= L) & (bins <= 23))) for L in range(LEVELS)], np.int64)


def choose_level(counts, target):
    for L in range(LEVELS):
        if counts[L] <= target:
            return L
    return 24


def cells(stream, level):
    """(order, seg, starts, parents): the sort's order, each sorted point's output index, each cell's first sorted point
    (plus n at the end) and each input point's output index."""
    n = parse_stream(stream)["num_points"]
    order = morton_order(stream)
    if n == 0:
        return order, np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.uint32)
    us = cell_u(stream)[order]
    flag = np.ones(n, bool)
    if n > 1:
        flag[1:] = np.any((us[1:] >> level) != (us[:-1] >> level), axis=1)
    seg = np.cumsum(flag) - 1
    starts = np.concatenate([np.flatnonzero(flag), [n]])
    parents = np.zeros(n, np.uint32)
    parents[order] = seg
    return order, seg, starts, parents


def quat_matrix(q):
    """Rotation matrices of (K, 4) (x, y, z, w) quaternions, normalised first."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def matrix_quat(M):
    """The (x, y, z, w) quaternion of a rotation matrix (the kernel's branches)."""
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    if tr > 0:
        t = np.sqrt(tr + 1.0) * 2.0
        return np.array([(M[2, 1] - M[1, 2]) / t, (M[0, 2] - M[2, 0]) / t, (M[1, 0] - M[0, 1]) / t, 0.25 * t])
    if M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
        t = np.sqrt(1.0 + M[0, 0] - M[1, 1] - M[2, 2]) * 2.0
        return np.array([0.25 * t, (M[0, 1] + M[1, 0]) / t, (M[0, 2] + M[2, 0]) / t, (M[2, 1] - M[1, 2]) / t])
    if M[1, 1] > M[2, 2]:
        t = np.sqrt(1.0 + M[1, 1] - M[0, 0] - M[2, 2]) * 2.0
        return np.array([(M[0, 1] + M[1, 0]) / t, 0.25 * t, (M[1, 2] + M[2, 1]) / t, (M[0, 2] - M[2, 0]) / t])
    t = np.sqrt(1.0 + M[2, 2] - M[0, 0] - M[1, 1]) * 2.0
    return np.array([(M[0, 2] + M[2, 0]) / t, (M[1, 2] + M[2, 1]) / t, 0.25 * t, (M[1, 0] - M[0, 1]) / t])


def cell_moments(pos_w, ls, quats, alpha_bytes, colors, sh):
    """The contract's moments of one cell, two-pass in f64.  pos_w: (k, 3) world offsets from the cell origin; ls: (k, 3)
    log scales; quats (k, 4); colors (k, 3) and sh (k, 3 * dim) decoded floats.  Returns a dict: W, unit (W == 0), mu
    (world, from the origin), cov (world^2), color, sh."""
    a = np.asarray(alpha_bytes, np.float64) / 255.0
    w = a * np.exp(np.sum(np.asarray(ls, np.float64), axis=1))
    W = float(np.sum(w))
    unit = W == 0.0
    if unit:
        w = np.ones_like(w)
    ws = float(np.sum(w))
    p = np.asarray(pos_w, np.float64)
    mu = (w[:, None] * p).sum(0) / ws
    R = quat_matrix(quats)
    s2 = np.exp(2.0 * np.asarray(ls, np.float64))
    own = np.einsum("kab,kb,kcb->kac", R, s2, R)
    d = p - mu
    cov = np.einsum("k,kab->ab", w, own + d[:, :, None] * d[:, None, :]) / ws
    return dict(W=W, unit=unit, mu=mu, cov=cov,
                color=(w[:, None] * np.asarray(colors, np.float64)).sum(0) / ws,
                sh=(w[:, None] * np.asarray(sh, np.float64)).sum(0) / ws if np.asarray(sh).size else np.zeros(0))


def gaussian_of(cov):
    """(log scales (3,), quaternion (4,), eigenvectors (3, 3) det +1) of a covariance: eigenvalues descending, floored."""
    lam, V = np.linalg.eigh(cov)
    lam, V = lam[::-1], V[:, ::-1].copy()
    lam = np.maximum(lam, EIG_FLOOR)
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    return 0.5 * np.log(lam), matrix_quat(V), V


def covariance_of(ls, q):
    """R diag(exp(2 ls)) R^T of (K, 3) log scales and (K, 4) quaternions."""
    R = quat_matrix(q)
    return np.einsum("kab,kb,kcb->kac", R, np.exp(2.0 * np.asarray(ls, np.float64)), R)


def target_covariance(cov):
    """What the encoding aims at: the eigenvalues floored and held inside the scale byte's range."""
    lam, V = np.linalg.eigh(cov)
    lam = np.clip(lam, np.exp(2 * SCALE_MIN), np.exp(2 * SCALE_MAX))
    return (V * lam) @ V.T


def decimate(oracle, stream, level):
    """The decimated v3 stream (bytes) at `level` and a dict of what it was made from: parents, counts, and per output
    point `multi` (bool), plus for the multi-point cells their moments."""
    h = parse_stream(stream)
    n, deg, fb, version = h["num_points"], h["sh_degree"], h["fractional_bits"], h["version"]
    assert version >= 2
    dim = SH_DIM[deg]
    order, seg, starts, parents = cells(stream, level)
    m = len(starts) - 1
    secs = h["sections"]
    head = np.zeros(16, np.uint8)
    head[:12] = np.array([MAGIC, 3, m], "<u4").view(np.uint8)
    head[12], head[13], head[14], head[15] = deg, fb, h["flags"] & 1, 0
    info = dict(parents=parents, counts=level_counts(stream), multi=np.zeros(m, bool), moments={})
    if m == 0:
        return bytes(head), info
    out = [np.zeros((m, b), np.uint8) for b in (9, 1, 3, 3, 4, 3 * dim)]
    rc, full = oracle.unpack(np.frombuffer(bytes(stream), np.uint8))
    assert rc == 0
    if version >= 3:
        rot_v3 = secs[4]
    else:   # the rotations re-encoded with the smallest-three encoder (as mergeSpz does)
        re = parse_stream(oracle.pack(full, n, deg, False, 0, 3).tobytes())
        rot_v3 = re["sections"][4]
    us_all = cell_u(stream)
    scales = full["scales"].reshape(n, 3)
    quats = full["rotations"].reshape(n, 4)
    colors = full["colors"].reshape(n, 3)
    sh = full["sh"].reshape(n, 3 * dim) if dim else np.zeros((n, 0), np.float32)
    alpha_b = secs[1][:, 0]
    multi_idx, multi_g = [], []
    for c in range(m):
        idx = order[starts[c]:starts[c + 1]]
        if idx.size == 1:
            i = idx[0]
            out[0][c], out[1][c], out[2][c], out[3][c], out[5][c] = secs[0][i], secs[1][i], secs[2][i], secs[3][i], secs[5][i]
            out[4][c] = rot_v3[i]
            continue
        u = us_all[idx]
        origin = (u[0] >> level) << level
        mo = cell_moments((u - origin) * 2.0 ** -fb, scales[idx], quats[idx], alpha_b[idx], colors[idx], sh[idx])
        ls, q, _ = gaussian_of(mo["cov"])
        alpha = 0.0 if mo["unit"] else min(1.0, mo["W"] / np.exp(np.sum(ls)))
        out[1][c] = np.clip(round_half_away(255.0 * alpha), 0, 255)
        r = np.clip(round_half_away(mo["mu"] * 2.0 ** fb), 0, (1 << level) - 1).astype(np.int64)
        f = ((origin + r) ^ 0x800000) & 0xFFFFFF
        out[0][c] = np.stack([(f >> s) & 0xFF for s in (0, 8, 16)], axis=1).reshape(-1)
        info["multi"][c] = True
        mo.update(ls=ls, q=q, origin=origin)
        info["moments"][c] = mo
        multi_idx.append(c)
        multi_g.append((ls, q, mo["color"], mo["sh"]))
    if multi_idx:
        k = len(multi_idx)
        cloud = {
            "positions": np.zeros(3 * k, np.float32),
            "scales": np.array([g[0] for g in multi_g], np.float32).reshape(-1),
            "rotations": np.array([g[1] for g in multi_g], np.float32).reshape(-1),
            "alphas": np.zeros(k, np.float32),
            "colors": np.array([g[2] for g in multi_g], np.float32).reshape(-1),
            "sh": np.array([g[3] for g in multi_g], np.float32).reshape(-1) if dim else np.zeros(0, np.float32),
        }
        enc = parse_stream(oracle.pack(cloud, k, deg, False, 0, 3).tobytes())["sections"]
        mi = np.array(multi_idx)
        out[2][mi], out[3][mi], out[4][mi], out[5][mi] = enc[2], enc[3], enc[4], enc[5]
    parts = [head] + [np.ascontiguousarray(o).reshape(-1) for o in out]
    return np.concatenate(parts).tobytes(), info
