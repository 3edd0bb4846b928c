"""Densify without a GPU (DESIGN §8 "Densify"; include/spz_amd.h "densify"): the option checks, the thresholds against
tests/densify_ref.py bit for bit (the derived extent of three orbit views included, and its refusal for one view), the
restatement's own plan rule on a hand-worked case, the argument checks of the new C entries (every refusal comes before
the first HIP call), spz.refine_spz's densify argument and spz_refine's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_ref as DR
import render_ref as RR
from conftest import ROOT


def lib():
    from spz_amd import abi
    return abi, abi.load_library()


def orbit(k, width=48, height=40):
    import spz_amd.spz as spz
    return spz.orbit_views(k, width=width, height=height, fov_y=50.0, center=[0.1, -0.2, 0.3], radius=2.5)


def params_of(v, coord=6):
    from spz_amd import abi
    return abi.render_params(np.asarray(v["world_to_camera"]), v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                             v["height"], 0.2, (0.0, 0.0, 0.0), 3, coord)


def test_signatures_resolve_and_structs_have_the_headers_sizes():
    abi, L = lib()
    for name, restype, nargs in (("spz_amd_densify_default_options", C.c_int, 1), ("spz_amd_densify_check", C.c_int, 1),
                                 ("spz_amd_densify_thresholds", C.c_int, 4),
                                 ("spz_amd_densify_accumulate_device", C.c_int, 8),
                                 ("spz_amd_densify_plan_workspace_bytes", C.c_uint64, 1),
                                 ("spz_amd_densify_plan_device", C.c_int, 14), ("spz_amd_densify_plan_host", C.c_int, 15),
                                 ("spz_amd_densify_apply_device", C.c_int, 15),
                                 ("spz_amd_densify_reset_opacity_device", C.c_int, 5),
                                 ("spz_amd_refine_densify_open", C.c_int, 24)):
        assert name in abi.EXPORTS
        f = getattr(L, name)
        assert f.restype is restype and len(f.argtypes) == nargs, name
    assert C.sizeof(abi.DensifyOptions) == 72 and C.sizeof(abi.DensifyLimits) == 32 and C.sizeof(abi.DensifyRound) == 48
    assert L.spz_amd_abi_version() == 1
    assert L.spz_amd_densify_plan_workspace_bytes(0) > 0 and L.spz_amd_densify_plan_workspace_bytes(2 ** 31) == 0
    assert L.spz_amd_densify_plan_workspace_bytes(1000) >= 2 * 4 * 1000


def test_defaults_are_the_published_values_with_densify_off():
    abi, _ = lib()
    o = abi.densify_options()
    assert (o.interval, o.from_iter, o.until_iter, o.opacity_reset_interval) == (0, 500, 15000, 0)
    assert (o.grad_threshold, o.percent_dense, o.extent, o.min_opacity, o.max_scale) == (2e-4, 0.01, 0.0, 0.005, 0.0)
    assert (o.max_points, o.seed) == (0, 0)
    o = abi.densify_options({"interval": 10, "seed": 2 ** 63}, max_points=77)
    assert (o.interval, o.seed, o.max_points) == (10, 2 ** 63, 77)
    assert abi.densify_options(o).interval == 10


def test_densify_check_refusals():
    abi, L = lib()
    assert L.spz_amd_densify_check(None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_densify_default_options(None) == abi.ERR_INVALID_ARG
    for field, value in (("interval", -1), ("from_iter", -1), ("until_iter", -5), ("opacity_reset_interval", -1),
                         ("grad_threshold", -1e-9), ("percent_dense", -0.01), ("extent", -1.0), ("max_scale", -2.0),
                         ("min_opacity", -0.1), ("min_opacity", 0.0), ("min_opacity", 1.0), ("min_opacity", 1.5),
                         ("grad_threshold", float("nan")), ("percent_dense", float("nan")), ("extent", float("nan")),
                         ("min_opacity", float("nan")), ("max_scale", float("nan"))):
        o = abi.densify_options(interval=5)
        setattr(o, field, value)
        assert L.spz_amd_densify_check(C.byref(o)) == abi.ERR_INVALID_ARG, (field, value)
    o = abi.densify_options(interval=5, from_iter=10, until_iter=10)
    assert L.spz_amd_densify_check(C.byref(o)) == abi.OK
    o.until_iter = 9
    assert L.spz_amd_densify_check(C.byref(o)) == abi.ERR_INVALID_ARG
    o = abi.densify_options(interval=0, percent_dense=0.0)          # off: percent_dense is not looked at
    assert L.spz_amd_densify_check(C.byref(o)) == abi.OK
    o.interval = 1
    assert L.spz_amd_densify_check(C.byref(o)) == abi.ERR_INVALID_ARG
    for kw in (dict(interval=-1), dict(interval=2.5), dict(interval=True), dict(intervall=3), dict(min_opacity=2.0),
               dict(grad_threshold=float("nan")), dict(max_points=-1), dict(from_iter=9, until_iter=3)):
        with pytest.raises(ValueError):
            abi.densify_options(**kw)
    with pytest.raises(ValueError):
        abi.densify_options([1, 2, 3])


@pytest.mark.parametrize("kw", [dict(), dict(extent=3.7), dict(max_scale=0.25, min_opacity=0.02),
                                dict(grad_threshold=1.3e-5, percent_dense=0.037), dict(extent=1e-3, max_scale=1e3)])
def test_thresholds_equal_the_restatement_bit_for_bit(kw):
    abi, _ = lib()
    views = orbit(3)
    o = abi.densify_options(interval=1, **kw)
    lim = abi.densify_thresholds(o, [params_of(v) for v in views])
    want = DR.thresholds(views=[v["world_to_camera"] for v in views], **kw)
    print(f"extent {lim.extent!r} (restated {want['extent']!r}), log_dense {lim.log_dense!r}, alpha_min {lim.alpha_min!r}")
    assert lim.extent == want["extent"] and lim.extent > 0.0
    for k in ("grad_threshold", "log_dense", "alpha_min", "log_max_scale"):
        assert np.float32(getattr(lim, k)).view(np.uint32) == want[k].view(np.uint32), k
    assert bool(lim.use_max_scale) == want["use_max_scale"]
    if "extent" not in kw:
        # the same by numpy's matrix product
        m = [np.asarray(v["world_to_camera"], np.float64) for v in views]
        c = np.array([-(w[:, :3].T @ w[:, 3]) for w in m])
        d = np.linalg.norm(c - c.mean(axis=0), axis=1)
        assert abs(lim.extent - 1.1 * d.max()) < 1e-5 * d.max()


def test_one_view_or_coincident_cameras_give_no_extent():
    abi, L = lib()
    o = abi.densify_options(interval=1)
    one = [params_of(orbit(1)[0])]
    assert DR.thresholds(views=[orbit(1)[0]["world_to_camera"]]) is None
    for views in (one, one * 3, []):
        with pytest.raises(abi.SpzAmdError) as e:
            abi.densify_thresholds(o, views)
        assert e.value.status == abi.ERR_INVALID_ARG
    # an explicit extent needs no views
    o.extent = 2.0
    lim = abi.densify_thresholds(o, [])
    assert np.float32(lim.log_dense) == DR.thresholds(extent=2.0)["log_dense"]
    assert L.spz_amd_densify_thresholds(C.byref(o), None, 0, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_densify_thresholds(None, None, 0, C.byref(lim)) == abi.ERR_INVALID_ARG


def test_the_restated_plan_on_a_case_worked_by_hand():
    """Six Gaussians: a cull by opacity, a clone, a split, a refused candidate (budget 2 of 3, the tie in g goes to the
    lower index), a keep by gradient, and a keep whose denom is 0."""
    lim = DR.thresholds(extent=1.0, percent_dense=0.1)   # log_dense = log 0.1
    big, small = np.log(0.5), np.log(0.01)
    scales = np.float32([[small] * 3, [small] * 3, [small, big, small], [small] * 3, [big] * 3, [big] * 3])
    alphas = np.float32([-10.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    accum = np.float32([9.0, 6e-4, 9e-4, 6e-4, 1e-4, 7.0])
    denom = np.int32([1, 3, 3, 3, 1, 0])
    action, parent, child, counts = DR.plan(accum, denom, scales, alphas, lim, 7)
    assert action.tolist() == [3, 1, 2, 0, 0, 0]
    assert parent.tolist() == [1, 1, 2, 2, 3, 4, 5] and child.tolist() == [0, 1, 2, 3, 0, 0, 0]
    assert counts == {"num_points": 7, "cloned": 1, "split": 1, "culled": 1, "refused": 1}
    z2, z3 = DR.normals(5, 0, 3)
    assert DR.normals(5, 0, 3) == (z2, z3) and DR.normals(6, 0, 3) != (z2, z3) and DR.normals(5, 1, 3) != (z2, z3)
    assert DR.sm(0) == 0xE220A8397B1DCDAF   # splitmix64's first output from state 0


def test_device_entries_refuse_bad_arguments_before_any_device_work():
    abi, L = lib()
    p = C.c_void_p(4096)
    odd = C.c_void_p(4098)
    lim = abi.densify_thresholds(abi.densify_options(interval=1, extent=1.0))
    nan_lim = abi.DensifyLimits.from_buffer_copy(lim)
    nan_lim.log_dense = float("nan")

    def acc(rec=p, rg=p, n=10, w=48, h=40, a=p, d=p):
        return L.spz_amd_densify_accumulate_device(rec, rg, n, w, h, a, d, None)

    for kw in (dict(rec=None), dict(rg=None), dict(a=None), dict(d=None), dict(w=0), dict(h=16385), dict(a=odd)):
        assert acc(**kw) == abi.ERR_INVALID_ARG, kw
    assert acc(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert acc(n=0, rec=None, rg=None, a=None, d=None) == abi.OK

    def plan(acc_=p, den=p, sc=p, al=p, n=10, lm=lim, mp=20, cap=20, act=p, par=p, ch=p, cnt=p, ws=p):
        return L.spz_amd_densify_plan_device(acc_, den, sc, al, n, C.byref(lm) if lm is not None else None, mp, cap, act,
                                             par, ch, cnt, ws, None)

    for kw in (dict(acc_=None), dict(den=None), dict(sc=None), dict(al=None), dict(lm=None), dict(act=None),
               dict(par=None), dict(ch=None), dict(cnt=None), dict(ws=None), dict(par=odd), dict(cnt=C.c_void_p(4100)),
               dict(lm=nan_lim)):
        assert plan(**kw) == abi.ERR_INVALID_ARG, kw
    assert plan(n=2 ** 31) == abi.ERR_TOO_MANY_POINTS and plan(mp=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert plan(cap=19) == abi.ERR_CAPACITY          # n' can reach min(2 n, max(max_points, n)) = 20
    assert plan(mp=5, cap=9) == abi.ERR_CAPACITY     # culls only: up to n
    h = (C.c_uint64 * 5)()
    assert L.spz_amd_densify_plan_host(p, p, p, p, 10, C.byref(lim), 20, 20, p, p, p, p, p, None, None) \
        == abi.ERR_INVALID_ARG
    assert L.spz_amd_densify_plan_host(p, p, p, p, 10, C.byref(lim), 20, 19, p, p, p, p, p, h, None) == abi.ERR_CAPACITY

    cl = abi.CloudPtrs(*([4096] * 6))
    no_sh = abi.CloudPtrs(*([4096] * 5), None)
    odd_cl = abi.CloudPtrs(*([4098] * 6))

    def apply(sp=cl, sm=cl, sv=cl, dp=cl, dm=cl, dv=cl, par=p, ch=p, n=10, m=12, cap=12, deg=1):
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        return L.spz_amd_densify_apply_device(ref(sp), ref(sm), ref(sv), ref(dp), ref(dm), ref(dv), par, ch, n, m, cap,
                                              deg, 1, 0, None)

    for kw in (dict(sp=None), dict(sm=None), dict(sv=None), dict(dp=None), dict(dm=None), dict(dv=None), dict(par=None),
               dict(ch=None), dict(sp=no_sh), dict(dv=no_sh), dict(dm=odd_cl), dict(n=0), dict(par=odd)):
        assert apply(**kw) == abi.ERR_INVALID_ARG, kw
    assert apply(deg=4) == abi.ERR_SH_DEGREE and apply(deg=-1) == abi.ERR_SH_DEGREE
    assert apply(m=13) == abi.ERR_CAPACITY
    assert apply(m=2 ** 31, cap=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert apply(m=0, cap=0, par=None, ch=None) == abi.OK
    assert L.spz_amd_densify_reset_opacity_device(None, p, p, 4, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_densify_reset_opacity_device(odd, p, p, 4, None) == abi.ERR_INVALID_ARG
    assert L.spz_amd_densify_reset_opacity_device(p, p, p, 2 ** 31, None) == abi.ERR_TOO_MANY_POINTS
    assert L.spz_amd_densify_reset_opacity_device(None, None, None, 0, None) == abi.OK
    if not torch.cuda.is_available():
        assert acc() == abi.ERR_NO_DEVICE and plan() == abi.ERR_NO_DEVICE and apply() == abi.ERR_NO_DEVICE
        assert apply(sp=no_sh, sm=no_sh, sv=no_sh, dp=no_sh, dm=no_sh, dv=no_sh, deg=0) == abi.ERR_NO_DEVICE
        assert L.spz_amd_densify_reset_opacity_device(p, None, None, 4, None) == abi.ERR_NO_DEVICE


def test_refine_densify_open_refuses_bad_arguments_and_no_device_is_an_error():
    abi, L = lib()
    ha, hb = abi.Header(), abi.Header()
    ha.num_points, ha.sh_degree, ha.version, ha.fractional_bits = 10, 1, 3, 12
    hb.num_points, hb.sh_degree, hb.version, hb.fractional_bits = 30, 1, 3, 12
    buf = (C.c_uint8 * 4096)()
    views = [params_of(v) for v in orbit(3)]
    history = (C.c_double * 8)()

    def call(vs=views, d="default", train=None, a_hdr=ha, b_hdr=hb, rounds_cap=4, **dkw):
        o = abi.refine_options(4, train=train)
        dn = abi.densify_options(interval=2, from_iter=0, until_iter=4, **dkw) if d == "default" else d
        arr = (abi.RenderParams * len(vs))(*vs)
        ctx, nbytes, bad, n_out, n_rounds = C.c_void_p(), C.c_uint64(), C.c_int32(7), C.c_uint64(9), C.c_int32(9)
        rounds = (abi.DensifyRound * 4)()
        rc = L.spz_amd_refine_densify_open(buf, 4096, C.byref(a_hdr), buf, 4096, C.byref(b_hdr), arr, len(vs), C.byref(o),
                                           C.byref(dn) if dn is not None else None, 0, C.byref(ctx), C.byref(nbytes),
                                           history, None, None, None, None, C.byref(bad), C.byref(n_out), rounds,
                                           rounds_cap, C.byref(n_rounds), None)
        assert not ctx.value and nbytes.value == 0
        return rc

    assert call(train=("scales", "colors")) == abi.ERR_INVALID_ARG            # positions untrained
    assert call(train=("positions", "colors")) == abi.ERR_INVALID_ARG         # scales untrained
    assert call(train=("positions", "scales"), opacity_reset_interval=3) == abi.ERR_INVALID_ARG   # alphas untrained
    assert call(max_points=9) == abi.ERR_INVALID_ARG                          # below A's count
    small = abi.Header.from_buffer_copy(hb)
    small.num_points = 5
    assert call(b_hdr=small) == abi.ERR_INVALID_ARG                           # max_points 0 = B's count, below A's
    assert call(max_points=2 ** 31) == abi.ERR_TOO_MANY_POINTS
    assert call(vs=views[:1]) == abi.ERR_INVALID_ARG                          # one view gives no extent
    assert call(rounds_cap=-1) == abi.ERR_INVALID_ARG
    bad = abi.densify_options(interval=2)
    bad.min_opacity = 2.0
    assert call(d=bad) == abi.ERR_INVALID_ARG
    if not torch.cuda.is_available():
        assert call() == abi.ERR_NO_DEVICE
        assert call(vs=views[:1], extent=2.0) == abi.ERR_NO_DEVICE
        assert call(train=("positions", "scales")) == abi.ERR_NO_DEVICE
        assert call(d=None, train=("colors",)) == abi.ERR_NO_DEVICE           # off: refine_open's rules alone
        assert call(d=abi.densify_options(interval=0), train=("colors",)) == abi.ERR_NO_DEVICE


def a_view(**kw):
    v = {"world_to_camera": RR.look_at([0, 0, -5], [0, 0, 0], [0, 1, 0]), "fx": 50.0, "fy": 50.0, "cx": 32.0,
         "cy": 24.0, "width": 64, "height": 48}
    v.update(kw)
    return v


def test_refine_spz_checks_its_densify_argument_first(tmp_path):
    import spz_amd.spz as spz
    from spz_amd import abi
    out = str(tmp_path / "out.spz")
    args = ("missing.spz", "missing_target.spz", out, [a_view()])
    for dn, kw, msg in [({"interval": -1}, {}, "wrong type or is out of range"), ({"interval": 2.5}, {}, "wrong type"),
                        ({"intervall": 3}, {}, "unknown field"), ({"min_opacity": 1.0}, {}, "min_opacity"),
                        ({"grad_threshold": float("nan")}, {}, "finite"), ({"extent": -1.0}, {}, "finite and >= 0"),
                        ({"from_iter": 5, "until_iter": 4}, {}, "until_iter"),
                        ({"interval": 3, "percent_dense": 0.0}, {}, "percent_dense"),
                        ({"interval": 3}, dict(train=["colors"]), "positions and scales"),
                        ({"interval": 3, "opacity_reset_interval": 9}, dict(train=["positions", "scales"]), "alphas"),
                        ([3], {}, "dict or a densify options object")]:
        with pytest.raises(ValueError, match=msg):
            spz.refine_spz(*args, densify=dn, **kw)
    # past the argument checks the missing file is what fails, with a dict and with an options object
    for dn in ({"interval": 3, "max_points": 100, "seed": 7}, abi.densify_options(interval=3), {"interval": 0}):
        with pytest.raises(RuntimeError):
            spz.refine_spz(*args, densify=dn)
    assert not os.path.exists(out)


def test_cli_densify_usage_errors(tmp_path):
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_refine")
    views = tmp_path / "v.txt"
    views.write_text("64 48 50 50 32 24 1 0 0 0 0 1 0 0 0 0 1 5\n")
    base = ["in.spz", "target.spz", str(tmp_path / "out.spz"), "--views", str(views)]
    for extra in [["--densify-interval"], ["--densify-interval", "-2"], ["--densify-interval", "1.5"],
                  ["--densify-interval", "5", "--densify-interval", "6"], ["--densify-from", "3"],
                  ["--grad-threshold", "1e-4"], ["--max-points", "10"], ["--seed", "1"],
                  ["--densify-interval", "5", "--grad-threshold", "-1"],
                  ["--densify-interval", "5", "--grad-threshold", "nan"],
                  ["--densify-interval", "5", "--percent-dense", "0"],
                  ["--densify-interval", "5", "--min-opacity", "1"], ["--densify-interval", "5", "--min-opacity", "0"],
                  ["--densify-interval", "5", "--max-points", "2.5"], ["--densify-interval", "5", "--max-points", "-1"],
                  ["--densify-interval", "5", "--seed", "x"], ["--densify-interval", "5", "--extent", "inf"],
                  ["--densify-interval", "5", "--densify-from", "9", "--densify-until", "3"],
                  ["--densify-interval", "5", "--opacity-reset-interval", "-1"]]:
        r = subprocess.run([tool, *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (extra, r.stdout, r.stderr)
        assert "Usage: spz_refine" in r.stderr and "--densify-interval" in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "out.spz").exists()
    # well-formed densify flags get as far as the missing input (no usage line), and trained arrays are checked first
    r = subprocess.run([tool, *base, "--densify-interval", "5", "--max-points", "100"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "Usage" not in r.stderr
    r = subprocess.run([tool, *base, "--densify-interval", "5", "--train", "colors"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "positions and scales" in r.stdout + r.stderr and "Usage" not in r.stderr
