"""Densify on the GPU (include/spz_amd.h "densify"; DESIGN §8 "Densify"), against tests/densify_ref.py.

Primitives.  accumulate, plan, the copied arrays and moments of apply, the split children's log scales and reset are
compared bit for bit.  A split child's position is p + R (exp(ls) (.) z) in f64 rounded once to f32; the device's f64
log, sin, cos and exp may differ from numpy's in the last f64 bits, far below one f32 rounding of a value of size |p| +
|offset|: the margin is one f32 ulp of |p| + |offset| per axis (derived, not measured).  plan runs on planted accum,
denom, scales and alphas, so nothing rests on the backward's atomics.  The plan's scan has two levels from 257 Gaussians
on (every workgroup scans its 256, one workgroup scans the workgroups' sums); that second level gives each of its 1024
threads a run of more than one sum only above 262 144 Gaussians, which the 300 001 case reaches.

Refine end to end.  The scene is render_grad_ref.scene(SCENE_SEED, 1): 300 Gaussians, SH1, three 48 x 40 orbit views in
the RDF frame.  B is the scene; A is every third Gaussian of B (100), both packed by the CPU oracle.  Before the inputs
below were fixed the loop was run on the CPU alone (reference_loop(): render_grad_ref's forward and autograd in float64,
loss_ref's loss and Adam, densify_ref's accumulate, plan and apply), once with densify and once without:
the mean PSNR of the three views on the floats went from 17.54 dB to 27.14 dB without densify and to 29.23 dB with it, a
margin of 2.09 dB (the condition was 0.5 dB); the rounds cloned 43 (43 % of A; the condition was 5 % to 50 %), 47 and 42
Gaussians, 100 -> 143 -> 190 -> 232 (above A's 100, under B's 300); with percent_dense = 1 every candidate's largest
scale is under the extent, so all are clones (splits run end to end in the colour test below, at percent_dense = 0.01).
Shorter runs did not meet the condition: at 45 and 150 iterations the reference gained nothing from the new Gaussians
(45: 21.06 dB without, 20.04 dB with; 150: 25.72 dB and 25.76 dB), because they need steps to move apart.  On the
device the margin asked for is half the reference's, 1.04 dB, and it is of the written files, quantisation included: the
backward's f32 atomics can move a Gaussian across the threshold, so the counts are not compared with the reference's
either."""
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_ref as DR
import loss_ref as LR
import metrics_ref as MR
import render_grad_ref as GR
import render_ref as RR
from conftest import ROOT, assert_bytes_equal

pytestmark = pytest.mark.gpu

ARRAYS = DR.ARRAYS
THR = 2.0 ** -12   # a gradient threshold float32 holds exactly


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == np.asarray(want).shape, (what, got.shape, np.asarray(want).shape)
    assert np.array_equal(bits(got), bits(np.asarray(want, dtype=got.dtype))), what


def limits(**kw):
    from spz_amd import abi
    kw.setdefault("extent", 1.0)
    kw.setdefault("grad_threshold", THR)
    return abi.densify_thresholds(abi.densify_options(interval=1, **kw)), DR.thresholds(**kw)


# ---- accumulate ----------------------------------------------------------------------------------------------------

def raw_records(depth):
    """n raw 48-byte render records with the given depths (the other fields are not read)."""
    rec = np.zeros(depth.size, dtype=[("f", "<f4", 10), ("rect", "<u2", 4)])
    rec["f"][:, :9] = 0.25
    rec["f"][:, 9] = depth
    return rec.view(np.uint8).reshape(-1)


@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_accumulate_is_the_f32_restatement_bit_for_bit(cuda, n):
    from spz_amd import device as D
    rng = np.random.default_rng(100 + n)
    w, h = 48, 40
    accum, denom = np.zeros(n, np.float32), np.zeros(n, np.int32)
    a_t, d_t = torch.as_tensor(accum).to(cuda), torch.as_tensor(denom).to(cuda)
    for call in range(2):   # two successive calls accumulate
        rg = (rng.standard_normal((n, 9)) * 10.0 ** rng.uniform(-6, -2, (n, 1))).astype(np.float32)
        depth = rng.uniform(0.5, 9.0, n).astype(np.float32)
        if n > 1:
            depth[rng.permutation(n)[:max(1, n // 5)]] = np.inf   # invisible
            k = rng.permutation(n)[:4]
            depth[k] = 3.0
            rg[k[0], 0], rg[k[1], 1], rg[k[2], 0], rg[k[3], 1] = np.nan, np.inf, 3e30, -np.inf
        elif call == 1:
            rg[0, 1] = np.nan
        D.densify_accumulate(torch.as_tensor(raw_records(depth)).to(cuda), torch.as_tensor(rg).to(cuda), w, h, a_t, d_t)
        accum, denom = DR.accumulate(depth, rg, w, h, accum, denom)
        same_bits(a_t, accum, f"accum after call {call}")
        same_bits(d_t, denom, f"denom after call {call}")
    assert np.isfinite(accum).all() and denom.max() == 2
    if n > 1:
        assert (denom == 0).any() and (accum[denom == 2] > 0).any()


# ---- plan ----------------------------------------------------------------------------------------------------------

def run_plan(cuda, accum, denom, scales, alphas, max_points, **lim_kw):
    from spz_amd import device as D
    lim, want_lim = limits(**lim_kw)
    got = D.densify_plan(torch.as_tensor(np.asarray(accum, np.float32)).to(cuda),
                         torch.as_tensor(np.asarray(denom, np.int32)).to(cuda),
                         torch.as_tensor(np.asarray(scales, np.float32).reshape(-1)).to(cuda),
                         torch.as_tensor(np.asarray(alphas, np.float32)).to(cuda), lim, max_points)
    action, parent, child, counts = DR.plan(accum, denom, scales, alphas, want_lim, max_points)
    same_bits(got["action"], action, "action")
    assert {k: got[k] for k in counts} == counts
    same_bits(got["parent"], parent.astype(np.int32), "parent")
    same_bits(got["child"], child, "child")
    return action, counts


def test_plan_of_nothing(cuda):
    _, counts = run_plan(cuda, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), 5)
    assert counts == {"num_points": 0, "cloned": 0, "split": 0, "culled": 0, "refused": 0}


@pytest.mark.parametrize("case,want", [("keep", 0), ("clone", 1), ("split", 2), ("cull", 3)])
def test_plan_of_one_gaussian(cuda, case, want):
    _, ref = limits(percent_dense=0.1)
    small, big = float(ref["log_dense"]) - 1.0, float(ref["log_dense"]) + 1.0
    accum = [0.5 * THR] if case == "keep" else [4.0 * THR]
    scales = [small, big if case == "split" else small, small]
    alphas = [-9.0] if case == "cull" else [0.3]
    action, counts = run_plan(cuda, accum, [1], scales, alphas, 2, percent_dense=0.1)
    assert action.tolist() == [want] and counts["num_points"] == (0, 1, 2, 2)[(3, 0, 1, 2).index(want)]


def planted_mix(n, seed, ref_lim):
    """A random mix of all four actions with the edge cases planted: alphas of -inf, +inf and NaN; denom == 0; g exactly
    the threshold; max(log scale) exactly log_dense; a NaN log scale; NaN and +inf in accum; a group of equal g."""
    rng = np.random.default_rng(seed)
    denom = rng.integers(0, 5, n).astype(np.int32)
    accum = (rng.uniform(0.0, 2.5 * THR, n) * np.maximum(denom, 1)).astype(np.float32)
    scales = rng.normal(float(ref_lim["log_dense"]), 1.0, (n, 3)).astype(np.float32)
    alphas = rng.normal(0.0, 4.0, n).astype(np.float32)
    k = rng.permutation(n)[:60]
    alphas[k[0:2]], alphas[k[2:4]], alphas[k[4:6]] = -np.inf, np.inf, np.nan
    denom[k[6:9]], accum[k[6:9]] = 0, 1.0                                   # never seen: g = 0
    denom[k[9:12]], accum[k[9:12]], alphas[k[9:12]] = 4, np.float32(4 * THR), 1.0   # g == threshold: a candidate
    scales[k[12:15], :] = ref_lim["log_dense"] - np.float32(0.5)
    scales[k[12:15], 1] = ref_lim["log_dense"]                              # not above log_dense: a clone
    accum[k[12:15]], denom[k[12:15]], alphas[k[12:15]] = 8 * THR, 2, 1.0
    scales[k[15], 0] = np.nan
    accum[k[16]], accum[k[17]] = np.nan, np.inf
    denom[k[16:18]], alphas[k[16:18]] = 1, 1.0
    ties = k[20:60]
    accum[ties], denom[ties], alphas[ties] = np.float32(3 * THR * 1.25), 3, 1.0   # forty equal g in mid-range
    return accum, denom, scales, alphas, ties


ODD_RUNS_N = 262_145   # 1025 tiles of 256 Gaussians for the 1024 threads of the second level: runs of two sums, the last
                       # owning thread holds one, half the block holds none


@pytest.mark.parametrize("n", [257, 70001, ODD_RUNS_N, 300001])
def test_plan_of_a_planted_mix(cuda, n):
    if n == ODD_RUNS_N:
        tiles = -(-n // 256)
        assert tiles % 2 == 1 and 1024 < tiles < 2 * 1024
    _, ref = limits(percent_dense=0.05)
    accum, denom, scales, alphas, ties = planted_mix(n, n, ref)
    action, counts = run_plan(cuda, accum, denom, scales, alphas, 2 * n, percent_dense=0.05)   # every candidate granted
    assert counts["refused"] == 0 and min(counts["cloned"], counts["split"], counts["culled"]) > n // 20
    assert (action == 0).sum() > n // 20
    _, off = run_plan(cuda, accum, denom, scales, alphas, 0, percent_dense=0.05)               # budget 0
    assert off["cloned"] == off["split"] == 0 and off["refused"] == counts["cloned"] + counts["split"]
    assert off["culled"] == counts["culled"] and off["num_points"] == n - counts["culled"]
    # a budget that cuts through the group of equal g: the lower indices of the group are granted
    g = np.where(denom > 0, accum / np.maximum(denom, 1).astype(np.float32), 0).astype(np.float32)
    cand = (action == 1) | (action == 2)
    assert cand[ties].all()
    above = int((cand & (g > g[ties[0]])).sum())
    cut, c = run_plan(cuda, accum, denom, scales, alphas, (n - counts["culled"]) + above + 17, percent_dense=0.05)
    assert c["cloned"] + c["split"] == above + 17 and c["num_points"] == (n - counts["culled"]) + above + 17
    granted = np.sort(ties)[(cut[np.sort(ties)] != 0)]
    assert granted.size == 17 and np.array_equal(granted, np.sort(ties)[:17])
    # max_scale on: more culls, and they come before the gradient rule
    _, on = run_plan(cuda, accum, denom, scales, alphas, 2 * n, percent_dense=0.05,
                     max_scale=float(np.exp(ref["log_dense"] + 1.0)))
    assert on["culled"] > counts["culled"] and on["split"] < counts["split"]


# ---- apply ---------------------------------------------------------------------------------------------------------

def float_state(n, deg, seed):
    from spz_amd.synth import make_cloud_numpy
    rng = np.random.default_rng(seed)
    p = make_cloud_numpy(n, deg, seed)
    p = {k: p[k] for k in ARRAYS}
    p["scales"] = (p["scales"] * 0.3 - 2.0).astype(np.float32)
    m = {k: (0.1 * rng.standard_normal(x.size)).astype(np.float32) for k, x in p.items()}
    v = {k: (0.01 * rng.standard_normal(x.size) ** 2).astype(np.float32) for k, x in p.items()}
    return p, m, v


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("n_new", [1, 3, 1025])
def test_apply_is_the_restatement(cuda, n_new, deg):
    from spz_amd import device as D
    n = max(2, (2 * n_new) // 3)
    rng = np.random.default_rng(7 * n_new + deg)
    p, m, v = float_state(n, deg, 50 + n_new)
    p["rotations"].reshape(-1, 4)[1] = 0.0   # a zero quaternion: its split children stay at the parent
    dev = [D.to_device(x, cuda) for x in (p, m, v)]
    if deg == 0:
        for c in dev:
            del c["sh"]   # sh may be absent at degree 0
    lists = [(np.sort(rng.integers(0, n, n_new)), rng.integers(0, 4, n_new))]
    if n_new == 1:
        lists = [(np.array([k % n]), np.array([k])) for k in range(4)]
    if n_new == 3:
        lists.append((np.array([1, 1, 1]), np.array([0, 2, 3])))
    for parent, child in lists:
        parent, child = parent.astype(np.int32), child.astype(np.uint8)
        p_t, c_t = torch.as_tensor(parent).to(cuda), torch.as_tensor(child).to(cuda)
        got = D.densify_apply(*dev, n, deg, p_t, c_t, seed=11, round=2)
        want = DR.apply(p, m, v, deg, parent.astype(np.int64), child, 11, 2)
        split = child >= 2
        for j, name in enumerate(("params", "m", "v")):
            for k in ARRAYS:
                w = DR.width(k, deg)
                if w == 0:
                    assert got[j][k].numel() == 0
                    continue
                g = got[j][k].cpu().numpy().reshape(-1, w)
                r = want[j][k].reshape(-1, w)
                if j == 0 and k == "positions":
                    same_bits(g[~split], r[~split], "copied positions")
                    continue
                same_bits(g, r, (name, k))   # split log scales and zeroed moments included
                if j:
                    assert not g[child != 0].any() and not np.signbit(g[child != 0]).any()
        pos = got[0]["positions"].cpu().numpy().reshape(-1, 3)
        src = p["positions"].reshape(-1, 3)[parent]
        off = want[3]
        margin = np.spacing((np.abs(src.astype(np.float64)) + np.abs(off)).astype(np.float32)).astype(np.float64)
        err = np.abs(pos.astype(np.float64) - (src.astype(np.float64) + off))
        if split.any():
            print(f"n' {n_new} deg {deg}: {int(split.sum())} split children, worst |pos - f64| / margin "
                  f"{(err[split] / margin[split]).max():.3f}, largest offset {np.abs(off).max():.3e}")
        assert (err[split] <= margin[split]).all()
        zero_q = split & (parent == 1)
        same_bits(pos[zero_q], src[zero_q], "children of a zero quaternion take the parent's position")
        moved = split & (parent != 1)
        assert (np.abs(off[moved]).max(axis=1) > 0).all() and (pos[moved] != src[moved]).any(axis=1).all()
        # the same seed and round give the same bits; another seed or round gives other children
        again = D.densify_apply(*dev, n, deg, p_t, c_t, seed=11, round=2)[0]["positions"]
        assert torch.equal(again.view(torch.int32), got[0]["positions"].view(torch.int32))
        if moved.any():
            for kw in (dict(seed=12, round=2), dict(seed=11, round=3)):
                other = D.densify_apply(*dev, n, deg, p_t, c_t, **kw)[0]["positions"].cpu().numpy().reshape(-1, 3)
                assert (other[moved] != pos[moved]).any(axis=1).all(), kw
                same_bits(other[~moved], pos[~moved], "everything but the split children")


def test_apply_and_plan_refuse_bad_arguments_with_nothing_launched(cuda):
    import ctypes as C
    from spz_amd import abi, device as D
    L = abi.load_library()
    n, deg = 40, 1
    p, m, v = float_state(n, deg, 3)
    src = [D.to_device(x, cuda) for x in (p, m, v)]
    dst = [{k: torch.full((8 * DR.width(k, deg),), -7.0, device=cuda) for k in p} for _ in range(3)]
    parent = torch.arange(8, dtype=torch.int32, device=cuda)
    child = torch.zeros(8, dtype=torch.uint8, device=cuda)
    sp = [D._ptrs(c, deg, n, cuda) for c in src]
    dp = [D._ptrs(c, deg, 8, cuda) for c in dst]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(s0=sp[0], d2=dp[2], par=parent.data_ptr(), n_new=8, cap=8, degree=deg):
        return L.spz_amd_densify_apply_device(C.byref(s0) if s0 is not None else None, C.byref(sp[1]), C.byref(sp[2]),
                                              C.byref(dp[0]), C.byref(dp[1]), C.byref(d2), par, child.data_ptr(), n,
                                              n_new, cap, degree, 0, 0, st)

    no_pos = abi.CloudPtrs.from_buffer_copy(dp[2])
    no_pos.positions = None
    assert call(s0=None) == abi.ERR_INVALID_ARG and call(par=None) == abi.ERR_INVALID_ARG
    assert call(d2=no_pos) == abi.ERR_INVALID_ARG
    assert call(degree=4) == abi.ERR_SH_DEGREE
    assert call(n_new=9, cap=8) == abi.ERR_CAPACITY
    torch.cuda.synchronize()
    for c in dst:
        for k, t in c.items():
            assert bool((t == -7.0).all()), k
    assert call() == abi.OK
    torch.cuda.synchronize()
    assert torch.equal(dst[0]["colors"], src[0]["colors"][:24])
    with pytest.raises(ValueError):
        D.densify_apply(*src, n, 4, parent, child)
    with pytest.raises(ValueError):
        D.densify_apply(*src, n, deg, parent.to(torch.int64), child)
    lim, _ = limits()
    with pytest.raises(ValueError):
        D.densify_plan(src[0]["alphas"], torch.zeros(n, dtype=torch.int64, device=cuda), src[0]["scales"],
                       src[0]["alphas"], lim, 50)
    with pytest.raises(ValueError):
        D.densify_plan(src[0]["alphas"], torch.zeros(n, dtype=torch.int32, device=cuda), src[0]["scales"],
                       src[0]["alphas"], lim, -1)


def test_reset_opacity_bit_for_bit(cuda):
    from spz_amd import device as D
    rng = np.random.default_rng(8)
    a = rng.normal(-4.0, 3.0, 1025).astype(np.float32)
    a[:6] = (np.inf, -np.inf, np.nan, np.log(0.01 / 0.99), -4.59, -4.6)
    m, v = rng.standard_normal(1025).astype(np.float32), rng.standard_normal(1025).astype(np.float32) ** 2
    a_t, m_t, v_t = (torch.as_tensor(x).to(cuda) for x in (a, m, v))
    D.reset_opacity(a_t, m_t, v_t)
    wa, wm, wv = DR.reset_opacity(a, m, v)
    same_bits(a_t, wa, "alphas")
    same_bits(m_t, wm, "m")
    same_bits(v_t, wv, "v")
    got = a_t.cpu().numpy()
    assert got[0] == np.float32(np.log(0.01 / 0.99)) and got[1] == -np.inf and np.isnan(got[2])
    assert (a > wa).sum() > 100 and (a == wa).sum() > 100
    only = torch.as_tensor(a).to(cuda)
    D.reset_opacity(only)   # a user whose optimiser is not ours
    same_bits(only, wa, "alphas alone")


# ---- refine with densify -------------------------------------------------------------------------------------------

SCENE_SEED, RW, RH, COORD = 4, 48, 40, 6   # RDF
ITERATIONS = 300
DENSIFY = {"interval": 20, "from_iter": 0, "until_iter": 61, "grad_threshold": 5e-3, "percent_dense": 1.0, "seed": 3}
REFERENCE_MARGIN_DB = 2.09   # what the CPU loop showed (it had to show 0.5); halved for the device (see the docstring)


@functools.lru_cache(maxsize=None)
def densify_scene():
    """B (the scene), A (every third Gaussian of B), both packed by the CPU oracle from the RDF frame, the three orbit
    views as dicts, and the position rate (1.6e-4 times the bounding-sphere radius)."""
    import spz_amd.spz as spz
    from oracle.pyoracle import Oracle
    O = Oracle()
    b = GR.scene(SCENE_SEED, 1)
    n = b["alphas"].size
    keep = np.arange(0, n, 3)
    a = {k: np.ascontiguousarray(v.reshape(n, -1)[keep]).reshape(-1) for k, v in b.items()}
    p = b["positions"].reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    views = spz.orbit_views(3, width=RW, height=RH, fov_y=50.0, center=centre.tolist(), radius=radius)
    return {"n_a": keep.size, "n_b": n, "deg": 1, "a": O.pack(a, keep.size, 1, False, COORD),
            "b": O.pack(b, n, 1, False, COORD), "views": views, "lrs": {"positions": 1.6e-4 * radius}, "oracle": O}


def view_params(v, coord=COORD):
    from spz_amd import abi
    return abi.render_params(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                             v["height"], 0.2, (0.0, 0.0, 0.0), 3, coord)


def reference_loop(densify=None, iterations=ITERATIONS):
    """The loop on the CPU, from A's decoded floats: render_grad_ref's forward and autograd in float64, loss_ref's loss
    and Adam with refine's default rates, and with `densify` (a dict as DENSIFY) densify_ref's accumulate, plan and
    apply where refine has them.  Returns (mean PSNR before, mean PSNR after, rounds, final count); what it gave is in
    this module's docstring.  Not run by the tests."""
    from spz_amd import abi
    s = densify_scene()
    O = s["oracle"]
    _, cloud = O.unpack(s["a"], COORD)
    _, target = O.unpack(s["b"], COORD)
    cloud = {k: cloud[k] for k in ARRAYS}
    cams = [RR.camera(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], RW, RH, 0.2, (0, 0, 0), 3)
            for v in s["views"]]
    targets = [RR.render({k: target[k] for k in ARRAYS}, 1, cam) for cam in cams]
    o = abi.refine_options(iterations, lrs=s["lrs"])
    psnr = lambda c: float(np.mean([MR.metrics(RR.render(c, 1, cam), t)[0]["psnr"]  # noqa: E731
                                    for cam, t in zip(cams, targets)]))
    before = psnr(cloud)
    m = {k: np.zeros_like(x) for k, x in cloud.items()}
    v = {k: np.zeros_like(x) for k, x in cloud.items()}
    n = s["n_a"]
    accum, denom = np.zeros(n, np.float32), np.zeros(n, np.int32)
    lim = None
    if densify:
        kw = {k: densify[k] for k in ("grad_threshold", "percent_dense", "extent", "min_opacity", "max_scale")
              if k in densify}
        lim = DR.thresholds(views=[x["world_to_camera"] for x in s["views"]], **kw)
    rounds = []
    for i in range(iterations):
        cam, tgt = cams[i % 3], targets[i % 3]
        dec = GR.decisions(cloud, 1, cam)
        t = GR.as_tensors(cloud, torch.float64)
        img, rec9 = GR.forward(t, 1, cam, dec)
        LR.loss_terms(img, tgt, o.lambda_dssim)[0].backward()
        in_range = densify and densify["from_iter"] <= i < densify["until_iter"]
        if in_range:
            rg = np.zeros((n, 9), np.float32)
            if rec9.grad is not None:
                rg[np.nonzero(dec["visible"])[0]] = rec9.grad.numpy().astype(np.float32)
            depth = np.where(dec["visible"], 1.0, np.inf).astype(np.float32)
            accum, denom = DR.accumulate(depth, rg, RW, RH, accum, denom)
        for j, k in enumerate(ARRAYS):
            g = (t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])).numpy().astype(np.float32)
            cloud[k], m[k], v[k], _ = LR.adam_step(cloud[k], g, m[k], v[k], i + 1, o.lr[j])
        if in_range and (i + 1) % densify["interval"] == 0:
            _, parent, child, counts = DR.plan(accum, denom, cloud["scales"], cloud["alphas"], lim,
                                               densify.get("max_points") or s["n_b"])
            cloud, m, v, _ = DR.apply(cloud, m, v, 1, parent.astype(np.int64), child, densify.get("seed", 0), len(rounds))
            n = counts["num_points"]
            accum, denom = np.zeros(n, np.float32), np.zeros(n, np.int32)
            rounds.append(dict(counts, iteration=i))
    return before, psnr(cloud), rounds, n


@functools.lru_cache(maxsize=None)
def resident(cuda_index):
    from spz_amd import abi
    s = densify_scene()
    dev = torch.device("cuda", cuda_index)
    a_t, b_t = torch.as_tensor(s["a"]).to(dev), torch.as_tensor(s["b"]).to(dev)
    rc, ha = abi.peek_header(s["a"].tobytes())
    assert rc == 0
    rc, hb = abi.peek_header(s["b"].tobytes())
    assert rc == 0
    return a_t, ha, b_t, hb, [view_params(v) for v in s["views"]]


@functools.lru_cache(maxsize=None)
def device_runs(cuda_index):
    """The two runs the assertions share: with DENSIFY and without, their reports and output bytes."""
    from spz_amd import device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda_index)
    out = {}
    for name, dn in (("densify", DENSIFY), ("plain", None)):
        with D.refine_packed(a_t, ha, b_t, hb, views, ITERATIONS, lrs=s["lrs"], densify=dn) as res:
            out[name] = (res.report, res.fetch().copy())
    return out


def sections(stream, n, deg):
    from spz_amd import abi
    lay = abi.stream_layout(n, deg, 3)
    s = np.asarray(stream)
    return {"header": s[:16], **{name: s[lay.offset[k]:lay.offset[k] + lay.bytes[k]] for k, name in
                                 enumerate(("positions", "alphas", "colors", "scales", "rotations", "sh"))}}


def mean_psnr(ms):
    return float(np.mean([m["psnr"] for m in ms]))


def test_refine_with_densify_grows_the_cloud_and_fits_better(cuda):
    from spz_amd import abi, device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    runs = device_runs(cuda.index)
    rep, out = runs["densify"]
    plain, _ = runs["plain"]
    n_new = rep["num_points"]
    print(f"rounds {rep['rounds']}; points {s['n_a']} -> {n_new} (B has {s['n_b']}); mean PSNR before "
          f"{mean_psnr(rep['before']):.3f} dB, after with densify {mean_psnr(rep['after']):.3f} dB, without "
          f"{mean_psnr(plain['after']):.3f} dB; ms {rep['ms']}")
    assert s["n_a"] < n_new <= s["n_b"]
    # the rounds add up
    n = s["n_a"]
    assert [r["iteration"] for r in rep["rounds"]] == [19, 39, 59]
    for r in rep["rounds"]:
        n = n - r["culled"] + r["cloned"] + r["split"]
        assert r["num_points"] == n
    assert n == n_new and plain["num_points"] == s["n_a"] and plain["rounds"] == []
    # the header is A's but for the count, and the stream has the layout's length
    rc, ho = abi.peek_header(out.tobytes())
    assert rc == 0 and ho.num_points == n_new
    assert (ho.version, ho.sh_degree, ho.fractional_bits, ho.flags) == (ha.version, ha.sh_degree, ha.fractional_bits,
                                                                         ha.flags)
    assert_bytes_equal(out[:4], s["a"][:4], "magic")
    assert out.size == rep["out_bytes"] == abi.stream_layout(n_new, s["deg"], 3).total_bytes
    assert rep["origin"].size == n_new and rep["origin"].max() < s["n_a"]
    # after: the metrics of the written stream, rendered with the packed path, bit for bit
    out_t = torch.as_tensor(out).to(cuda)
    for k, p in enumerate(views):
        m = D.image_metrics(D.render_packed(out_t, ho, p), D.render_packed(b_t, hb, p)).cpu().numpy()
        assert rep["after"][k] == dict(zip(("mse", "psnr", "ssim", "l1", "max_abs"), m.tolist())), k
    # before and history[0] come before any step or round: the same bits with and without
    assert rep["before"] == plain["before"] and rep["history"][0] == plain["history"][0]
    assert len(rep["history"]) == ITERATIONS
    assert mean_psnr(rep["after"]) > mean_psnr(rep["before"])
    assert mean_psnr(rep["after"]) >= mean_psnr(plain["after"]) + 0.5 * REFERENCE_MARGIN_DB


def test_refine_densify_off_through_the_new_entry_is_refine_packed(cuda):
    from spz_amd import device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    plain, _ = device_runs(cuda.index)["plain"]
    with D.refine_packed(a_t, ha, b_t, hb, views, 3, lrs=s["lrs"], densify={"interval": 0}) as res:
        assert res.report["before"] == plain["before"] and res.report["history"][0] == plain["history"][0]
        assert res.report["num_points"] == s["n_a"] and res.report["rounds"] == []
        assert np.array_equal(res.report["origin"], np.arange(s["n_a"]))
    for dn in ({"interval": 0}, {"interval": 4}):
        with D.refine_packed(a_t, ha, b_t, hb, views, 0, densify=dn) as res:
            assert_bytes_equal(res.fetch(), s["a"], f"iterations = 0 with {dn}")
            assert res.report["after"] == res.report["before"] == plain["before"]


def test_refine_densify_keeps_untrained_colour_bytes_through_the_origin(cuda):
    from spz_amd import device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    dn = dict(DENSIFY, percent_dense=0.01)   # every candidate is larger than 1 % of the extent: splits
    with D.refine_packed(a_t, ha, b_t, hb, views, 45, lrs=s["lrs"], train=("positions", "scales", "rotations", "alphas",
                                                                            "sh"), densify=dn) as res:
        rep, out = res.report, res.fetch()
    n_new = rep["num_points"]
    assert n_new > s["n_a"] and len(rep["rounds"]) == 2 and sum(r["split"] for r in rep["rounds"]) > 0
    got = sections(out, n_new, s["deg"])
    want = sections(s["a"], s["n_a"], s["deg"])
    assert_bytes_equal(got["colors"].reshape(-1, 3), want["colors"].reshape(-1, 3)[rep["origin"]],
                       "colours gathered through the origin")
    assert not np.array_equal(got["alphas"], want["alphas"][rep["origin"]])
    assert (np.diff(rep["origin"].astype(np.int64)) >= 0).all(), "output order is input order"


def test_refine_densify_at_capacity_does_not_grow_and_still_culls(cuda):
    from spz_amd import device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    dn = dict(DENSIFY, max_points=s["n_a"], min_opacity=0.6)
    with D.refine_packed(a_t, ha, b_t, hb, views, 45, lrs=s["lrs"], densify=dn) as res:
        rep = res.report
    print(f"at capacity: rounds {rep['rounds']}")
    assert all(r["num_points"] <= s["n_a"] for r in rep["rounds"]) and rep["num_points"] <= s["n_a"]
    assert sum(r["culled"] for r in rep["rounds"]) > 0


def test_refine_densify_refusals(cuda):
    from spz_amd import abi, device as D
    s = densify_scene()
    a_t, ha, b_t, hb, views = resident(cuda.index)
    for kw in (dict(train=("scales", "colors")), dict(train=("positions", "colors")),
               dict(densify=dict(DENSIFY, max_points=s["n_a"] - 1)), dict(views=views[:1]),
               dict(train=("positions", "scales"), densify=dict(DENSIFY, opacity_reset_interval=5))):
        args = dict(views=views, densify=DENSIFY)
        args.update(kw)
        with pytest.raises(abi.SpzAmdError) as e:
            D.refine_packed(a_t, ha, b_t, hb, args.pop("views"), 4, **args)
        assert e.value.status == abi.ERR_INVALID_ARG, kw
    with pytest.raises(abi.SpzAmdError) as e:
        D.refine_packed(a_t, ha, b_t, hb, views, 4, densify=dict(DENSIFY, max_points=2 ** 31))
    assert e.value.status == abi.ERR_TOO_MANY_POINTS
    # one view with an explicit extent runs, and an opacity reset lowers the alphas it is due for
    with D.refine_packed(a_t, ha, b_t, hb, views[:1], 4, densify=dict(DENSIFY, interval=2, extent=3.0,
                                                                      opacity_reset_interval=4)) as res:
        assert len(res.report["rounds"]) == 2
        lay = abi.stream_layout(res.report["num_points"], s["deg"], 3)
        alphas = res.fetch()[lay.offset[abi.SEC_ALPHAS]:lay.offset[abi.SEC_ALPHAS] + lay.bytes[abi.SEC_ALPHAS]]
        assert alphas.max() <= 3   # sigmoid(logit(0.01)) * 255 = 2.55


def test_densify_through_the_file_layers(cuda, tmp_path):
    import spz_amd.spz as spz
    from spz_amd import abi
    s = densify_scene()
    rep, _ = device_runs(cuda.index)["densify"]
    fa, fb, fo, fc = (str(tmp_path / x) for x in ("a.spz", "b.spz", "out.spz", "cli.spz"))
    for path, stream in ((fa, s["a"]), (fb, s["b"])):
        with open(path, "wb") as f:
            f.write(gzip.compress(stream.tobytes(), 6))
    r = spz.refine_spz(fa, fb, fo, s["views"], iterations=ITERATIONS, coord=spz.RDF, lrs=s["lrs"], densify=DENSIFY)
    assert r["history"][0] == rep["history"][0] and [m["psnr"] for m in r["before"]] == [m["psnr"] for m in rep["before"]]
    assert s["n_a"] < r["num_points"] <= s["n_b"] and len(r["rounds"]) == 3
    assert r["rounds"][-1]["num_points"] == r["num_points"]
    with gzip.open(fo, "rb") as f:
        written = f.read()
    rc, ho = abi.peek_header(written)
    assert rc == 0 and ho.num_points == r["num_points"]
    again = spz.compare_spz(fo, fb, s["views"], coord=spz.RDF)
    assert [m["psnr"] for m in again] == [m["psnr"] for m in r["after"]], "the report's after is the written file's"
    assert np.mean([m["psnr"] for m in r["after"]]) > np.mean([m["psnr"] for m in r["before"]])
    views_file = tmp_path / "views.txt"
    views_file.write_text("".join(
        " ".join([str(v["width"]), str(v["height"])] + [repr(float(x)) for x in (v["fx"], v["fy"], v["cx"], v["cy"])]
                 + [repr(float(x)) for x in np.asarray(v["world_to_camera"]).reshape(-1)]) + "\n" for v in s["views"]))
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_refine")
    run = subprocess.run([tool, fa, fb, fc, "--views", str(views_file), "--iters", str(ITERATIONS), "--coord", "RDF",
                          "--lr-positions", repr(s["lrs"]["positions"]), "--densify-interval", str(DENSIFY["interval"]),
                          "--densify-from", str(DENSIFY["from_iter"]), "--densify-until", str(DENSIFY["until_iter"]),
                          "--grad-threshold", repr(DENSIFY["grad_threshold"]), "--seed", str(DENSIFY["seed"])],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.strip().split("\n")
    rounds = [ln for ln in lines if ln.startswith("densify iteration ")]
    assert len(rounds) == 3 and lines[-1].startswith("points ")
    count = int(lines[-1].split()[1])
    assert int(rounds[-1].split()[-1]) == count and s["n_a"] < count <= s["n_b"]
    with gzip.open(fc, "rb") as f:
        rc, hc = abi.peek_header(f.read())
    assert rc == 0 and hc.num_points == count
    after = float([ln for ln in lines if ln.startswith("mean psnr ")][0].split()[4])
    assert float(np.mean([m["psnr"] for m in spz.compare_spz(fc, fb, s["views"], coord=spz.RDF)])) == after
