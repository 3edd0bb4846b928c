"""A numpy / Python-int restatement of the plane contract (include/spz_amd.h "plane", DESIGN §8 "Level"): the prepared
points, the seeded hypotheses, the integer score, the exact moments, the solve (exact integers, then the same cyclic
Jacobi in Python floats, which are IEEE doubles without fused multiply-add) and the run with its orientation, labels and
levelling placement.  A helper module, not a test file: tests/test_plane_host.py checks the library's host functions
against it and tests/test_gpu_plane.py the device."""
import math

import numpy as np

from clean_ref import stored_positions
from test_filter_host import parse_stream

MASK64 = (1 << 64) - 1
MAX_T = 1 << 36
# coordinate systems 1..8: the bits of coord - 1 say R, U, F
UNSPECIFIED, RUB = 0, 4


def mix64(z):
    """splitmix64's finaliser."""
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def threshold(tau, f):
    """T = floor(tau 2^(f+16)), or None where the library refuses it."""
    if not math.isfinite(tau) or tau < 0:
        return None
    t = math.floor(math.ldexp(tau, f + 16))
    return t if t <= MAX_T else None


def flips(coord):
    """The axis signs between coord and the stored RUB frame."""
    if coord == 0:
        return (1.0, 1.0, 1.0)
    a, b = coord - 1, RUB - 1
    return tuple(-1.0 if ((a >> k) & 1) != ((b >> k) & 1) else 1.0 for k in range(3))


def prepare(P, stride=1, labels=None):
    """(prepared points (m, 3) int64, their input indices)."""
    n = P.shape[0]
    take = (np.arange(n) % stride) == 0
    if labels is not None:
        take &= np.asarray(labels) == 0
    idx = np.nonzero(take)[0]
    return P[idx], idx


def sample_indices(seed, r, H, m):
    return [[mix64(seed + (r << 48) + 3 * h + k) % m for k in range(3)] for h in range(H)]


def hypothesis(idx, P0, P1, P2, axis=None, max_tilt=90.0):
    """One plane (a, b, c, e) of three prepared points with their indices; (0, 0, 0, 0) is invalid."""
    if idx[0] == idx[1] or idx[0] == idx[2] or idx[1] == idx[2]:
        return (0, 0, 0, 0)
    u = [int(P1[k]) - int(P0[k]) for k in range(3)]
    v = [int(P2[k]) - int(P0[k]) for k in range(3)]
    N = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    if N == (0, 0, 0):
        return (0, 0, 0, 0)
    nx, ny, nz = float(N[0]), float(N[1]), float(N[2])
    L = math.sqrt((nx * nx + ny * ny) + nz * nz)
    a, b, c = (int(np.rint(65536.0 * t / L)) for t in (nx, ny, nz))
    e = a * int(P0[0]) + b * int(P0[1]) + c * int(P0[2])
    if axis is not None:
        norm = math.sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])
        ux, uy, uz = (t / norm for t in axis)
        if abs((float(a) * ux + float(b) * uy) + float(c) * uz) < 65536.0 * math.cos(max_tilt * (math.pi / 180.0)):
            return (0, 0, 0, 0)
    return (a, b, c, e)


def hypotheses(Q, seed, r, H, axis=None, max_tilt=90.0):
    """(planes, indices) of round r over the prepared points Q."""
    idx = sample_indices(seed, r, H, Q.shape[0])
    return [hypothesis(t, Q[t[0]], Q[t[1]], Q[t[2]], axis, max_tilt) for t in idx], idx


def distances(Q, plane):
    a, b, c, e = plane
    return Q[:, 0] * a + Q[:, 1] * b + Q[:, 2] * c - e      # int64: |d| < 2^43


def valid(plane):
    """a, b, c not all zero, and in range: a, b, c in [-2^16, 2^16], |e| <= 2^42."""
    return any(plane[:3]) and all(abs(v) <= 65536 for v in plane[:3]) and abs(plane[3]) <= 1 << 42


def score(Q, planes, T):
    """[(K, S, cost)] per plane."""
    m = Q.shape[0]
    out = []
    for p in planes:
        if not valid(p):
            out.append((0, 0, MASK64))
            continue
        ad = np.abs(distances(Q, p))
        inl = ad <= T
        K, S = int(inl.sum()), int(ad[inl].sum())
        out.append((K, S, S + T * (m - K)))
    return out


def moments(Q, plane, T):
    """The exact sums as Python ints."""
    d = distances(Q, plane)
    inl = np.abs(d) <= T
    I = [[int(v) for v in row] for row in Q[inl]]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return {"count": len(I), "sum_abs": int(np.abs(d[inl]).sum()), "above": int((d > T).sum()),
            "below": int((d < -T).sum()), "points": int(Q.shape[0]),
            "sum_p": [sum(p[k] for p in I) for k in range(3)],
            "sum_pp": [sum(p[i] * p[j] for p in I) for i, j in pairs]}


def jacobi3(A):
    """Cyclic Jacobi on the symmetric A (lists, changed in place); returns V whose columns are the eigenvectors."""
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(64):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[p][q]
                if apq == 0.0 or abs(apq) <= 1e-17 * math.sqrt(abs(A[p][p])) * math.sqrt(abs(A[q][q])):
                    continue
                rotated = True
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(1.0 + theta * theta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for k in range(3):
                    x, y = A[k][p], A[k][q]
                    A[k][p] = c * x - s * y
                    A[k][q] = s * x + c * y
                for k in range(3):
                    x, y = A[p][k], A[q][k]
                    A[p][k] = c * x - s * y
                    A[q][k] = s * x + c * y
                for k in range(3):
                    x, y = V[k][p], V[k][q]
                    V[k][p] = c * x - s * y
                    V[k][q] = s * x + c * y
        if not rotated:
            break
    return V


def div_round(num, den):
    """num / den to the nearest integer, ties to even, in exact integers (den > 0)."""
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    return q


def moment_matrix(mo):
    """M = K sum P P^T - sum P sum P^T as exact ints."""
    pair = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    return [[mo["count"] * mo["sum_pp"][pair[i][j]] - mo["sum_p"][i] * mo["sum_p"][j] for j in range(3)]
            for i in range(3)]


def solve(mo):
    """(plane, normal, eigenvalues descending), or None when degenerate."""
    K = mo["count"]
    if K < 3:
        return None
    A = [[float(v) for v in row] for row in moment_matrix(mo)]
    V = jacobi3(A)
    order = [0, 1, 2]
    for a in range(2):
        for b in range(a + 1, 3):
            if A[order[b]][order[b]] > A[order[a]][order[a]]:
                order[a], order[b] = order[b], order[a]
    l0, l1 = A[order[0]][order[0]], A[order[1]][order[1]]
    if not (l0 > 0.0) or not math.isfinite(l0) or not (l1 > 1e-12 * l0):
        return None
    s = order[2]
    n = [V[k][s] for k in range(3)]
    a, b, c = (int(np.rint(65536.0 * t)) for t in n)
    if not (a or b or c):
        return None
    e = div_round(a * mo["sum_p"][0] + b * mo["sum_p"][1] + c * mo["sum_p"][2], K)
    return (a, b, c, e), n, [A[k][k] for k in order]


def placement(plane, f, coord=0, no_translate=False):
    """(normal in coord, offset, rotation (x, y, z, w) in coord, translation in coord) of an oriented plane."""
    a, b, c, e = (float(v) for v in plane)
    L = math.sqrt((a * a + b * b) + c * c)
    n = (a / L, b / L, c / L)
    d = math.ldexp(e / L, -f)
    fl = flips(coord)
    det = fl[0] * fl[1] * fl[2]
    q = [-n[2], 0.0, n[0], (n[0] * n[0] + n[2] * n[2]) / (1.0 - n[1]) if n[1] < 0.0 else 1.0 + n[1]]
    if q[3] < 1e-12:
        q = [1.0, 0.0, 0.0, 0.0]
    qn = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    rot = [det * fl[k] * q[k] / qn for k in range(3)] + [q[3] / qn]
    return ([fl[k] * n[k] for k in range(3)], d, rot, [0.0, 0.0 if no_translate else fl[1] * -d, 0.0])


def run(P, f, tau, hypotheses_count=4096, seed=0, stride=1, refine=3, max_planes=1, min_inliers=0, axis=None,
        max_tilt=90.0, up_hint=None, coord=0, no_translate=False):
    """Definition 7 over the stored integers P (N, 3) int64.  axis and up_hint are stated in coord.  Returns
    (list of plane dicts, labels uint8)."""
    T = threshold(tau, f)
    fl = flips(coord)
    axis_s = None if axis is None else [fl[k] * axis[k] for k in range(3)]
    hint_s = None if up_hint is None else [fl[k] * up_hint[k] for k in range(3)]
    labels = np.zeros(P.shape[0], np.uint8)
    found = []
    for r in range(max_planes):
        Q, index = prepare(P, stride, labels)
        m = Q.shape[0]
        if m < 3:
            break
        planes, idx = hypotheses(Q, seed, r, hypotheses_count, axis_s, max_tilt)
        sc = score(Q, planes, T)
        best = min(range(len(planes)), key=lambda h: (sc[h][2], h))
        cost = sc[best][2]
        if cost == MASK64:
            break
        cur, accepted = planes[best], 0
        for _ in range(refine):
            got = solve(moments(Q, cur, T))
            if got is None:
                break
            s1 = score(Q, [got[0]], T)[0]
            if not s1[2] < cost:
                break
            cost, cur, accepted = s1[2], got[0], accepted + 1
        mo = moments(Q, cur, T)
        if mo["count"] < min_inliers:
            break
        if hint_s is not None:
            negate = (float(cur[0]) * hint_s[0] + float(cur[1]) * hint_s[1]) + float(cur[2]) * hint_s[2] < 0.0
        elif mo["above"] != mo["below"]:
            negate = mo["below"] > mo["above"]
        else:
            negate = cur[1] < 0
        if negate:
            cur = tuple(-v for v in cur)
            mo["above"], mo["below"] = mo["below"], mo["above"]
        inl = np.abs(distances(Q, cur)) <= T
        labels[index[inl]] = r + 1
        normal, offset, rot, tr = placement(cur, f, coord, no_translate)
        found.append({"plane": cur, "inliers": mo["count"], "sum_abs": mo["sum_abs"], "points": m,
                      "above": mo["above"], "below": mo["below"], "best_hypothesis": best, "refinements": accepted,
                      "fitness": mo["count"] / m,
                      "mean_distance": math.ldexp(mo["sum_abs"] / mo["count"], -(f + 16)) if mo["count"] else 0.0,
                      "normal": normal, "offset": offset, "rotation": rot, "translation": tr,
                      "triple": idx[best]})
    return found, labels


def run_stream(raw, tau, **kw):
    """run() over a raw (inflated) v2/v3 stream."""
    return run(stored_positions(raw), parse_stream(raw)["fractional_bits"], tau, **kw)
