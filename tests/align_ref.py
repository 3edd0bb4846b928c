"""A numpy restatement of the align contract (include/spz_amd.h "align", DESIGN §8 "Align"): the mapped and rounded
queries, the exact nearest target point on int64 with ties to the smallest index, the trimming by an exact rank on
(d2, source index), the moments, the solve by numpy's SVD and the run.  A helper module, not a test file:
tests/test_align_host.py checks it against an independent O(n^2) loop and the library's solve against it, and
tests/test_gpu_align.py compares the device with it.

Two routes to the nearest neighbour: chunked brute force (exact int64), and for large n a scipy cKDTree over the
distinct target points (each standing for its smallest input index), whose candidates' d2 are recomputed in int64; a
query whose candidates do not settle the answer (a tie beyond them, or distances f64 cannot tell apart) is redone by
brute force."""
import math

import numpy as np

from clean_ref import radius_r2, stored_positions
from test_filter_host import parse_stream

BRUTE_MAX_PAIRS = 50_000_000
NONE = -1
SAT = 1 << 26
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def queries(P_src, f_s, f_t, m, stride=1):
    """Steps 1-2: (Q (n_s, 3) int64, valid (n_s,) bool).  Points not taking part are not valid."""
    m = np.asarray(m, np.float64)
    x = P_src.astype(np.float64) * np.float64(2.0 ** -int(f_s))
    n = P_src.shape[0]
    Q = np.zeros((n, 3), np.int64)
    valid = (np.arange(n) % stride) == 0
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            y = ((m[3 * a] * x[:, 0] + m[3 * a + 1] * x[:, 1]) + m[3 * a + 2] * x[:, 2]) + m[9 + a]
            valid &= np.isfinite(y)
            r = np.rint(y * np.float64(2.0 ** int(f_t)))
            Q[:, a] = np.where(np.isfinite(y), np.clip(np.nan_to_num(r, nan=0.0), -SAT, SAT), 0).astype(np.int64)
    Q[~valid] = 0
    return Q, valid


def _nearest_brute(Q, T, chunk=None):
    n = T.shape[0]
    chunk = chunk or max(1, min(4096, 8_000_000 // max(n, 1)))
    idx = np.empty(Q.shape[0], np.int64)
    d2 = np.empty(Q.shape[0], np.int64)
    for s in range(0, Q.shape[0], chunk):
        e = min(Q.shape[0], s + chunk)
        d = Q[s:e, None, :] - T[None, :, :]
        dd = np.einsum("ijk,ijk->ij", d, d)
        j = np.argmin(dd, axis=1)          # the first minimum: the smallest index
        idx[s:e] = j
        d2[s:e] = dd[np.arange(e - s), j]
    return idx, d2


def _nearest_tree(Q, T, k=4):
    import pytest
    spatial = pytest.importorskip("scipy.spatial")
    U, first = np.unique(T, axis=0, return_index=True)   # first: the smallest input index of each distinct point
    k = min(k, U.shape[0])
    tree = spatial.cKDTree(U.astype(np.float64))
    _, cand = tree.query(Q.astype(np.float64), k=k, workers=16)
    cand = cand.reshape(Q.shape[0], k)
    d = U[cand] - Q[:, None, :]
    dd = np.einsum("ijk,ijk->ij", d, d)
    orig = first[cand]
    # the smallest (d2, input index) among the candidates
    best = dd.min(axis=1)
    tied = dd == best[:, None]
    idx = np.where(tied, orig, np.iinfo(np.int64).max).min(axis=1)
    d2 = best
    if k < U.shape[0]:
        # unsettled: the farthest candidate is no farther than the best by more than f64 can tell
        far = dd.max(axis=1)
        redo = np.nonzero((far - best).astype(np.float64) <= best.astype(np.float64) * 2.0 ** -48)[0]
        if redo.size:
            idx[redo], d2[redo] = _nearest_brute(Q[redo], T)
    return idx, d2


def nearest(Q, T, valid=None, limit=None, method=None):
    """Step 3 (+ the limit of step 4): (index, d2) int64, NONE for queries that are not valid or have no target point
    with d2 <= limit."""
    n = Q.shape[0]
    valid = np.ones(n, bool) if valid is None else valid
    idx = np.full(n, NONE, np.int64)
    d2 = np.full(n, NONE, np.int64)
    sel = np.nonzero(valid)[0]
    if sel.size and T.shape[0]:
        method = method or ("brute" if sel.size * T.shape[0] <= BRUTE_MAX_PAIRS else "tree")
        i, d = (_nearest_brute if method == "brute" else _nearest_tree)(Q[sel], T)
        idx[sel], d2[sel] = i, d
    if limit is not None:
        out = (idx != NONE) & (d2 > limit)
        idx[out] = NONE
        d2[out] = NONE
    return idx, d2


def keep_count(c, overlap):
    return min(c, int(math.ceil(float(overlap) * float(c))))


def step(P_src, f_s, P_tgt, f_t, m, stride=1, max_distance=None, overlap=1.0, method=None, terms=False):
    """Steps 1-5: dict(index, d2, inlier, count, taking_part, candidates, sum_d2 (python int), sum_a, sum_b, sum_ab
    (9, row-major a_r b_c), sum_aa, sum_bb); with terms=True also `terms`, the (K, 17) array whose columns are summed."""
    limit = None if max_distance is None else radius_r2(max_distance, f_t)
    Q, valid = queries(P_src, f_s, f_t, m, stride)
    idx, d2 = nearest(Q, P_tgt, valid, limit, method)
    cand = np.nonzero(idx != NONE)[0]
    K = keep_count(cand.size, overlap)
    order = cand[np.lexsort((cand, d2[cand]))][:K]
    inlier = np.zeros(P_src.shape[0], bool)
    inlier[order] = True
    sel = np.nonzero(inlier)[0]
    a = P_src[sel].astype(np.float64) * np.float64(2.0 ** -int(f_s))
    b = P_tgt[idx[sel]].astype(np.float64) * np.float64(2.0 ** -int(f_t))
    t = np.empty((sel.size, 17), np.float64)
    t[:, 0:3] = a
    t[:, 3:6] = b
    for r in range(3):
        for c in range(3):
            t[:, 6 + 3 * r + c] = a[:, r] * b[:, c]
    t[:, 15] = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    t[:, 16] = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    s = t.sum(axis=0)
    out = dict(index=idx, d2=d2, inlier=inlier, count=int(sel.size), taking_part=(P_src.shape[0] + stride - 1) // stride,
               candidates=int(cand.size), sum_d2=int(sum(int(v) for v in d2[sel])), sum_a=s[0:3], sum_b=s[3:6],
               sum_ab=s[6:15], sum_aa=float(s[15]), sum_bb=float(s[16]))
    if terms:
        out["terms"] = t
    return out


def solve(mom, estimate_scale, scale_in):
    """Step 6 with numpy's SVD: (map (12,), scale) or None when degenerate."""
    K = mom["count"]
    if K < 3:
        return None
    ma = np.asarray(mom["sum_a"], np.float64) / K
    mb = np.asarray(mom["sum_b"], np.float64) / K
    var_a = mom["sum_aa"] / K - float((ma[0] * ma[0] + ma[1] * ma[1]) + ma[2] * ma[2])
    if not var_a > 0.0 or not math.isfinite(var_a):
        return None
    H = np.asarray(mom["sum_ab"], np.float64).reshape(3, 3).T / K - np.outer(mb, ma)
    if not np.all(np.isfinite(H)):
        return None
    U, D, Vt = np.linalg.svd(H)
    if not D[0] > 0.0 or not D[1] > 1e-12 * D[0]:
        return None
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = (U * S) @ Vt
    s = float((D * S).sum() / var_a) if estimate_scale else float(scale_in)
    t = mb - s * (R @ ma)
    return np.concatenate([(s * R).reshape(-1), t]), s


def fitness_rmse(mom, f_t):
    fit = mom["count"] / mom["taking_part"] if mom["taking_part"] else 0.0
    rmse = math.sqrt(float(mom["sum_d2"]) / mom["count"]) * 2.0 ** -int(f_t) if mom["count"] else 0.0
    return fit, rmse


def run(P_src, f_s, P_tgt, f_t, m0=IDENTITY, scale0=1.0, estimate_scale=False, stride=1, max_distance=None, overlap=1.0,
        max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, method=None):
    """The run from a map in the stored frame: dict(map, scale, fitness, inlier_rmse, inliers, iterations, converged,
    degenerate, history)."""
    m, scale = np.asarray(m0, np.float64), float(scale0)
    res = dict(converged=False, degenerate=False, history=[])
    prev = None
    for it in range(max_iterations):
        mom = step(P_src, f_s, P_tgt, f_t, m, stride, max_distance, overlap, method)
        fit, rmse = fitness_rmse(mom, f_t)
        res["history"].append((fit, rmse, mom["count"]))
        res.update(map=m.copy(), scale=scale, fitness=fit, inlier_rmse=rmse, inliers=mom["count"], iterations=it + 1)
        if prev is not None and abs(fit - prev[0]) <= relative_fitness * max(fit, prev[0]) and \
                abs(rmse - prev[1]) <= relative_rmse * max(rmse, prev[1]):
            res["converged"] = True
            break
        prev = (fit, rmse)
        if it + 1 == max_iterations:
            break
        nxt = solve(mom, estimate_scale, scale)
        if nxt is None:
            res["degenerate"] = True
            break
        m, scale = nxt
    return res


def initial_map(rotation=(0.0, 0.0, 0.0, 1.0), translation=(0.0, 0.0, 0.0), scale=1.0, coord=0):
    """The map (12,) in the stored RUB frame of a placement stated in `coord` (0: unspecified, no flips; 1..8 = LDB, RDB,
    LUB, RUB, LDF, RDF, LUF, RUF): R = F R_c F, t = F t_c with F the axis flips between coord and RUB."""
    f = np.ones(3)
    if coord:
        f = np.array([1.0 if ((coord - 1) >> a) & 1 == (3 >> a) & 1 else -1.0 for a in range(3)])
    Rm = quat_to_matrix(rotation) * f[:, None] * f[None, :]
    return np.concatenate([(float(scale) * Rm).reshape(-1), f * np.asarray(translation, np.float64)])


def centroid_map(P_src, f_s, P_tgt, f_t, m, stride=1):
    """init_centroids: m with its translation replaced so that the centroid of the taking-part source points lands on
    the centroid of all target points."""
    m = np.asarray(m, np.float64).copy()
    cs = (P_src[::stride].astype(np.float64) * 2.0 ** -int(f_s)).mean(axis=0)
    ct = (P_tgt.astype(np.float64) * 2.0 ** -int(f_t)).mean(axis=0)
    m[9:] = ct - m[:9].reshape(3, 3) @ cs
    return m


def quat_to_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def axis_angle_quat(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return tuple(a * math.sin(angle / 2)) + (math.cos(angle / 2),)


def map_errors(m, scale, R_true, t_true, s_true):
    """(rotation angle in rad, translation distance, |scale difference|) between a map (12,) and a known placement."""
    m = np.asarray(m, np.float64)
    R = m[:9].reshape(3, 3) / scale
    c = (np.trace(R.T @ R_true) - 1.0) / 2.0
    dR = R - R_true
    ang = math.acos(max(-1.0, min(1.0, c))) if c < 1 - 1e-9 else float(np.linalg.norm(dR) / math.sqrt(2.0))
    return ang, float(np.linalg.norm(m[9:] - np.asarray(t_true))), abs(scale - s_true)


def positions_of(stream):
    h = parse_stream(stream)
    return stored_positions(stream), h["fractional_bits"]
