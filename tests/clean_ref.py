"""A numpy restatement of the clean contract (include/spz_amd.h "clean", DESIGN §8 "Clean"): exact squared distances on
the sign-extended stored integers, the k_eff smallest per point, the statistical scores and threshold, the radius
counts and the keep mask.  A helper module, not a test file: tests/test_clean_host.py checks it against an independent
O(n^2) loop and tests/test_gpu_clean.py compares the device with it.

Two routes to the k smallest d2: chunked brute force (exact int64), and for large n a scipy cKDTree on the float64
integer coordinates, whose squared distances are exact (< 2^50), with every returned neighbour's d2 recomputed in
int64."""
import numpy as np

from test_filter_host import parse_stream
from test_sort_host import position_fields

BRUTE_MAX = 20_000


def stored_positions(stream):
    """(N, 3) int64: the sign-extended stored 24-bit integers."""
    f = position_fields(stream).astype(np.int64)
    return np.where(f >= 1 << 23, f - (1 << 24), f)


def k_eff(n, k):
    return max(0, min(k, n - 1))


def radius_r2(radius, fractional_bits):
    """R2 = floor(fl((radius * 2^f)^2)), in f64 (python floats are IEEE doubles)."""
    q = float(radius) * 2.0 ** int(fractional_bits)
    return int(np.floor(q * q))


def _knn_d2_brute(P, keff, chunk=512):
    n = P.shape[0]
    out = np.empty((n, keff), np.int64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        d = P[s:e, None, :] - P[None, :, :]
        d2 = np.einsum("ijk,ijk->ij", d, d)
        d2[np.arange(e - s), np.arange(s, e)] = np.iinfo(np.int64).max   # the point itself, by index
        part = np.partition(d2, keff - 1, axis=1)[:, :keff]
        out[s:e] = np.sort(part, axis=1)
    return out


def _knn_d2_tree(P, keff):
    import pytest
    spatial = pytest.importorskip("scipy.spatial")
    tree = spatial.cKDTree(P.astype(np.float64))
    _, idx = tree.query(P.astype(np.float64), k=keff + 1, workers=16)
    idx = idx.reshape(P.shape[0], keff + 1)
    d = P[idx] - P[:, None, :]
    d2 = np.sort(np.einsum("ijk,ijk->ij", d, d), axis=1)
    # the k_eff + 1 nearest including the point itself (distance 0, the smallest); drop one 0
    assert np.all(d2[:, 0] == 0)
    return d2[:, 1:]


def knn_d2(stream_or_positions, k, method=None):
    """(N, k_eff) int64: the k_eff smallest d2 to other points, ascending."""
    P = stream_or_positions if isinstance(stream_or_positions, np.ndarray) else stored_positions(stream_or_positions)
    n = P.shape[0]
    keff = k_eff(n, k)
    if keff == 0:
        return np.zeros((n, 0), np.int64)
    method = method or ("brute" if n <= BRUTE_MAX else "tree")
    return _knn_d2_brute(P, keff) if method == "brute" else _knn_d2_tree(P, keff)


def scores_of(d2, fractional_bits):
    """score_i = (sum of sqrt(d2) in ascending order) / k_eff * 2^-f, f64; 0 when k_eff == 0."""
    n, keff = d2.shape
    if keff == 0:
        return np.zeros(n, np.float64)
    s = np.zeros(n, np.float64)
    for j in range(keff):
        s = s + np.sqrt(d2[:, j].astype(np.float64))
    return s / np.float64(keff) * np.float64(2.0 ** -int(fractional_bits))


def threshold_of(scores, std_ratio):
    n = scores.size
    if n == 0:
        return 0.0
    mean = scores.sum() / n
    std = np.sqrt(np.sum((scores - mean) ** 2) / (n - 1)) if n > 1 else 0.0
    return float(mean + std_ratio * std)


def radius_counts(stream_or_positions, r2, min_neighbors, chunk=512):
    """count_i = min(#{j != i : d2 <= R2}, min_neighbors), int64, by chunked brute force."""
    P = stream_or_positions if isinstance(stream_or_positions, np.ndarray) else stored_positions(stream_or_positions)
    n = P.shape[0]
    out = np.empty(n, np.int64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        d = P[s:e, None, :] - P[None, :, :]
        d2 = np.einsum("ijk,ijk->ij", d, d)
        within = d2 <= r2
        within[np.arange(e - s), np.arange(s, e)] = False
        out[s:e] = np.minimum(within.sum(axis=1), min_neighbors)
    return out


def clean(stream, k=None, std_ratio=2.0, radius=None, min_neighbors=None):
    """dict(scores, kth_d2, threshold, counts, keep) of the contract (None for a rule not given)."""
    h = parse_stream(stream)
    n, fb = h["num_points"], h["fractional_bits"]
    P = stored_positions(stream)
    r = dict(scores=None, kth_d2=None, threshold=None, counts=None)
    keep = np.ones(n, bool)
    if k is not None:
        d2 = knn_d2(P, k)
        r["scores"] = scores_of(d2, fb)
        r["kth_d2"] = d2[:, -1] if d2.shape[1] else np.zeros(n, np.int64)
        r["threshold"] = threshold_of(r["scores"], std_ratio)
        keep &= r["scores"] <= r["threshold"]
    if radius is not None:
        r["counts"] = radius_counts(P, radius_r2(radius, fb), min_neighbors)
        keep &= r["counts"] >= min_neighbors
    if n <= 1:
        keep[:] = True
    r["keep"] = keep
    return r
