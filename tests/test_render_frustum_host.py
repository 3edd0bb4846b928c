"""The frustum scenes (tests/frustum_ref.py: a view from inside the cloud) without a GPU: the scenes' own assertions, the
reference's rows for invisible and non-finite Gaussians, a central-difference check of the reference where the quotients
of J clamp, and the CPU build of the two per-Gaussian chains of the render backward (preprocess_backward_one and
view_backward_one, the functions the device kernels call; tests/cpp/render_chain_host.cpp) against the reference.

The central differences.  Float64, records not rounded, the decisions held, L = sum(G * image).  For
each perturbed value the two steps h = 1e-5 and 1e-6 give two quotients; their difference d measures what a central
difference is worth there (rounding eps |L| / h against truncation h^2 |L'''| / 6), and autograd's value must lie
within 10 d + 1e-9 max|array| of both.  Nothing is fixed in advance.  L is summed exactly (math.fsum) and rounded once:
with a blocked float64 sum the two quotients of one alpha came out equal to the last bit, d = 0, while both were 1.9e-9
off (the rounding of |L| = 44 at h = 1e-6, eps |L| / 2h = 3.5e-9).  Observed: over the 44 cloud values of the four
perturbed Gaussians (one past lim_x_pos, one past lim_y_neg, the corner, one cut at the left edge) the worst error is
0.150 (plain) and 0.104 (antialiased) of its allowance, over the 12 pose entries 0.121 and 0.110.

Observed for the CPU build (error as a fraction of its bound, the worst array; all / clamped / cut): plain 0.035 /
0.050 / 0.044, antialiased 0.051 / 0.041 / 0.054, strip 0.049 / 0.049 / 0.041; the view sums agree to below 5e-4 of
their 1e-12.  The clamped class carries 0.11, 0.10 and 0.07 of a pose entry's sum |contribution|.  With free_x set to
1.0 in preprocess_backward_one the positions are off by 2.6 where 2.9e-5 is allowed; in view_backward_one the view sums
by 10.2 where 1.2e-9 is allowed; without the zero-fill of the invisible branch the NaN the output was filled with shows.

The CPU build.  preprocess_backward_one from the reference's float64 record gradients rounded to float32: per array
within 1e-6 of the reference's largest value (test_render_grad_host's rule: the chain runs in f64 and rounds its result
to f32 once, 6e-8), over all Gaussians and then over the clamped class and the cut-rect class alone, each against its
own largest value, so a small class cannot hide under the crowd's maximum; every entry of an invisible Gaussian is an
exact 0 (the output is filled with NaN before the run).  view_backward_one: the sums of the 12 contributions within
1e-12 of the largest sum of magnitudes (test_locate_host's rule for the chain), again over all and per class."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import depth_grad_ref as DG
import frustum_ref as F
import render_grad_ref as GR
import render_ref as RR
import view_grad_ref as VR
from conftest import ROOT

ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")
SMALL = ("plain", "aa")


def image_gradient(s, seed=41):
    cam = s["cam"]
    return np.random.default_rng(seed).standard_normal((cam["height"], cam["width"], 4)).astype(np.float32)


@pytest.mark.parametrize("variant", list(F.VARIANTS))
def test_the_scene_reaches_every_arm(variant):
    """scene() asserts the class table and the conditions on the whole scene from the reference; here also what the
    builder promises about the camera and the order."""
    s = F.scene(variant)
    print(f"{variant}: seed {F.SEEDS[variant]}, classes {s['counts']}, scene {s['facts']}")
    cam = s["cam"]
    p = s["cloud"]["positions"].reshape(-1, 3).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    eye = -(cam["R"].T @ cam["t"])
    assert (p.min(axis=0) < eye).all() and (eye < p.max(axis=0)).all(), "the eye lies inside the cloud's box"
    R = cam["R"]
    assert np.abs(R).max() < 0.999 and np.abs(R - np.eye(3)).max() > 0.05, "the camera is not axis-aligned"
    assert cam["fx"] != cam["fy"] and len(set(np.round(F.limits(cam), 6))) == 4, "the four lim values differ"
    assert s["dec"]["visible"].sum() == s["counts"]["visible"]
    if variant != "strip":
        assert s["n"] <= 500 and cam["width"] == 40 and cam["height"] == 36


@pytest.mark.parametrize("variant", list(F.VARIANTS))
def test_the_seed_is_the_first_that_meets_the_conditions(variant):
    assert F.first_seed(variant) == F.SEEDS[variant]


@pytest.mark.parametrize("variant", SMALL)
def test_the_packed_scene_keeps_its_classes(variant):
    """The finite classes through a v3 stream (the CPU oracle's pack and unpack, which the device's encode and decode
    equal bit for bit): the class table holds on the decoded floats, no r3 lies near an integer, and the visible set
    is the float scene's."""
    from oracle.pyoracle import Oracle
    from spz_amd import abi
    s = F.scene(variant)
    f = F.finite_part(s)
    O = Oracle()
    rc, w = O.unpack(O.pack(f["cloud"], f["n"], f["deg"], s["aa"], abi.RUB), abi.RUB)
    assert rc == 0
    decoded = {k: np.asarray(w[k], dtype=np.float32).reshape(-1) for k in f["cloud"]}
    rec = RR.preprocess(decoded, f["deg"], f["cam"], s["aa"])
    print(f"{variant} packed: {F.check_classes(f, rec)}")
    r3 = rec["r3"][rec["visible"]]
    assert (np.abs(r3 - np.round(r3)) >= 1e-4).all()
    assert np.array_equal(rec["visible"], s["dec"]["rec"]["visible"][f["kept"]])


@pytest.mark.parametrize("variant", SMALL)
def test_the_references_give_exact_zero_rows_to_invisible_gaussians(variant):
    """render_grad_ref, depth_grad_ref and view_grad_ref index the visible Gaussians out before any arithmetic: every
    row of an invisible Gaussian, the non-finite ones included, is an exact 0 and every value is finite, in float64
    and in float32."""
    s = F.scene(variant)
    cloud, deg, cam, dec, aa, n = s["cloud"], s["deg"], s["cam"], s["dec"], s["aa"], s["n"]
    hidden = ~dec["visible"]
    assert hidden[F.members(s["labels"], "nonfinite")].all()
    G = image_gradient(s)
    GD = np.random.default_rng(43).standard_normal((cam["height"], cam["width"])).astype(np.float32)
    for dtype in (torch.float64, torch.float32):
        g = GR.gradients(cloud, deg, cam, dec, G, aa, dtype)
        d = DG.gradients(cloud, deg, cam, dec, G, GD, aa, dtype)
        for name, ref, keys in (("render", g, ARRAYS + ("records",)), ("depth", d, ARRAYS + ("records", "depth"))):
            for k in keys:
                a = F.rows_of(ref[k], n)
                assert np.isfinite(a).all(), (name, k)
                assert not a[hidden].any(), (name, k)
            assert np.isfinite(ref["image"]).all()
        v = VR.view_gradient(cloud, deg, cam, dec, G, aa, dtype)
        assert np.isfinite(v["view"]).all() and not v["records"][hidden].any()
    rg = g["records"].astype(np.float32)
    per = VR.chain(cloud, deg, cam, dec, rg, aa, forward_mode=True)
    assert np.isfinite(per).all() and not per[hidden].any()
    c = F.chain_to_cloud(cloud, deg, cam, dec, rg, aa)
    for k in ARRAYS:
        a = F.rows_of(c[k], n)
        assert np.isfinite(a).all() and not a[hidden].any(), k
    if aa:
        disc = F.members(s["labels"], "disc")
        flat = dec["rec"]["det0"][disc] <= 0
        assert not F.rows_of(g["alphas"], n)[disc][flat].any(), "a disc with det0 <= 0 has an alpha gradient"


def perturbed_gaussians(s):
    """One past an x limit, one past a y limit, the corner, one cut rect."""
    L = s["labels"]
    return {"clamp_x_pos": int(F.members(L, "clamp_x_pos")[0]), "clamp_y_neg": int(F.members(L, "clamp_y_neg")[0]),
            "corner": int(F.members(L, "corner")[0]), "cut_x_neg": int(F.members(L, "cut_x_neg")[0])}


@pytest.mark.parametrize("variant", SMALL)
def test_the_reference_equals_central_differences_where_it_clamps(variant):
    """The reference defines "no gradient where the quotient clamps": its autograd values against central differences
    of its own forward at two step sizes (the module's docstring has the rule and the observed ratios)."""
    s = F.scene(variant)
    c, deg, cam, dec, aa = s["cloud"], s["deg"], s["cam"], s["dec"], s["aa"]
    G = image_gradient(s)
    g = GR.gradients(c, deg, cam, dec, G, aa, round_records=False)
    Gt = torch.as_tensor(G).to(torch.float64)
    cloud = GR.as_tensors(c, torch.float64, requires_grad=False)

    def loss(cam_now=cam):
        with torch.no_grad():
            img = GR.forward(cloud, deg, cam_now, dec, aa, round_records=False)[0]
            return math.fsum((img * Gt).reshape(-1).tolist())  # rounded once: a blocked sum's rounding moves with h

    def quotient(move, h):
        move(h)
        up = loss()
        move(-h)
        down = loss()
        move(0.0)
        return (up - down) / (2.0 * h)

    worst = 0.0
    width = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1}
    for label, i in perturbed_gaussians(s).items():
        for k, wd in width.items():
            scale = np.abs(g[k]).max()
            for e in range(i * wd, i * wd + wd):
                x = float(cloud[k][e])

                def move(step, k=k, e=e, x=x):
                    cloud[k][e] = x + step

                q5, q6 = quotient(move, 1e-5), quotient(move, 1e-6)
                d = abs(q5 - q6)
                allowed = 10.0 * d + 1e-9 * scale
                err = max(abs(q5 - g[k][e]), abs(q6 - g[k][e]))
                worst = max(worst, err / allowed)
                assert err <= allowed, (label, k, e, g[k][e], q5, q6)
            assert np.abs(g[k][i * wd:i * wd + wd]).max() > 0.0, (label, k)
        print(f"{variant} {label}: autograd within {worst:.3f} of 10 |q(1e-5) - q(1e-6)| + 1e-9 max|array| so far")
    # the clamp itself: a position gradient that took free_x = 1 would differ by the J02 term, which is not small
    v = VR.view_gradient(c, deg, cam, dec, G, aa, round_records=False)["view"]
    pose = np.concatenate([cam["R"], cam["t"][:, None]], axis=1)
    worst_v = 0.0
    for r in range(3):
        for k in range(4):
            def at(step):
                m = pose.copy()
                m[r, k] += step
                cm = dict(cam)
                cm["R"], cm["t"] = torch.as_tensor(m[:, :3].copy()), torch.as_tensor(m[:, 3].copy())
                return loss(cm)
            q5 = (at(1e-5) - at(-1e-5)) / 2e-5
            q6 = (at(1e-6) - at(-1e-6)) / 2e-6
            allowed = 10.0 * abs(q5 - q6) + 1e-9 * np.abs(v).max()
            err = max(abs(q5 - v[r, k]), abs(q6 - v[r, k]))
            worst_v = max(worst_v, err / allowed)
            assert err <= allowed, (r, k, v[r, k], q5, q6)
    print(f"{variant}: cloud values within {worst:.3f} of their allowance, pose entries within {worst_v:.3f}")


def write_scene(path, s, record_grads):
    """The scene file of tests/cpp/render_chain_host.cpp, with the reference's records."""
    from spz_amd import abi
    m, fx, fy, cx, cy = s["view"]
    cam = s["cam"]
    params = abi.render_params(m, fx, fy, cx, cy, cam["width"], cam["height"], F.NEAR, F.BG, 3, 0)
    rec, n = s["dec"]["rec"], s["n"]
    records = np.zeros((n, 12), dtype=np.float32)
    records[:, 0:2], records[:, 2:5], records[:, 5] = rec["mean"], rec["conic"], rec["opacity"]
    records[:, 6:9], records[:, 9] = rec["rgb"], rec["depth"]
    records[:, 10:12] = rec["rect"].astype(np.uint16).view(np.float32)
    with open(path, "wb") as f:
        f.write(np.array([n, s["deg"], 1 if s["aa"] else 0, 0], dtype=np.int32).tobytes())
        f.write(bytes(params))
        for k in ARRAYS:
            f.write(np.asarray(s["cloud"][k], dtype=np.float32).tobytes())
        f.write(records.tobytes())
        f.write(np.asarray(record_grads, dtype=np.float32).tobytes())


def read_result(path, n, dim):
    raw = np.fromfile(path, dtype=np.uint8)
    out, at = {}, 0
    for k, per in zip(ARRAYS, (3, 3, 4, 1, 3, 3 * dim)):
        out[k] = raw[at:at + 4 * n * per].view(np.float32).astype(np.float64).reshape(n, per)
        at += 4 * n * per
    out["view"] = raw[at:at + 8 * n * 12].view(np.float64).reshape(n, 3, 4)
    assert at + 8 * n * 12 == raw.size
    return out


@pytest.mark.parametrize("variant", list(F.VARIANTS))
def test_the_cpu_build_of_the_two_chains(variant, tmp_path):
    """preprocess_backward_one and view_backward_one, compiled for the host, over the scene with the reference's
    record gradients (rounded to float32, as the device's are) against autograd of the reference's records."""
    s = F.scene(variant)
    cloud, deg, cam, dec, aa, n = s["cloud"], s["deg"], s["cam"], s["dec"], s["aa"], s["n"]
    G = image_gradient(s)
    rg = GR.gradients(cloud, deg, cam, dec, G, aa)["records"].astype(np.float32)
    write_scene(tmp_path / "scene.bin", s, rg)
    tool = os.path.join(ROOT, "spz_amd", "bin", "render_chain_host")
    done = subprocess.run([tool, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                          timeout=60)
    assert done.returncode == 0 and not done.stderr.strip(), done.stderr
    got = read_result(tmp_path / "out.bin", n, RR.SH_DIM[deg])
    want = F.chain_to_cloud(cloud, deg, cam, dec, rg, aa)
    per = VR.chain(cloud, deg, cam, dec, rg, aa, forward_mode=True)
    hidden = ~dec["visible"]
    classes = {"all": np.arange(n), "clamped": F.members(s["labels"], "clamp"), "cut": F.members(s["labels"], "cut")}
    for k in ARRAYS + ("view",):
        assert np.isfinite(got[k]).all(), f"{k}: an entry is not finite (NaN: never written)"
        assert not got[k][hidden].any(), f"{k}: an invisible Gaussian's entry is not an exact 0"
    for name, rows in classes.items():
        line = []
        for k in ARRAYS:
            w = F.rows_of(want[k], n)[rows]
            scale = np.abs(w).max()
            err = np.abs(got[k][rows] - w).max()
            line.append(f"{k} {err / (1e-6 * scale):.3f}")
            assert scale > 0.0 and err <= 1e-6 * scale, (name, k, err, scale)
        mag = np.abs(per[rows]).sum(axis=0)
        err = np.abs(got["view"][rows].sum(axis=0) - per[rows].sum(axis=0)).max()
        line.append(f"view {err / (1e-12 * mag.max()):.1e}")
        assert err <= 1e-12 * mag.max(), (name, "view", err, mag.max())
        print(f"{variant} {name} ({rows.size} Gaussians), error as a fraction of its bound: " + ", ".join(line))
    # the clamped class is no bystander: in some entry it carries a twentieth of the pose gradient's magnitude
    share = np.abs(per[classes["clamped"]]).sum(axis=0) / np.abs(per).sum(axis=0)
    print(f"{variant}: the clamped class carries up to {share.max():.3f} of sum |contribution| of a pose entry")
    assert share.max() >= 0.05
