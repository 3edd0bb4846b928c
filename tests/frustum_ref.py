"""The frustum scene: a view from inside a cloud, for the arms of the rasteriser's per-Gaussian chain that only an
interior camera reaches (DESIGN §8 "Render", "Render backward", "Locate"): culling (behind the camera, inside near, off
the image, non-finite), the clamp of x / z and y / z at the four lim values, a tile rectangle cut at the edge of the
tile grid, and max(0, det0) under antialiasing.  Shared by tests/test_render_frustum_host.py and
tests/test_gpu_render_frustum.py.

The Gaussians are placed by inverse projection (as test_gpu_render_scale.unproject places them) under a camera that is
not axis-aligned: render_ref.look_at from an eye inside the cloud's box with a tilted up, fx = 0.9 H and fy = 1.1 H,
the principal point off the middle (so the four lim values differ), near = 0.2.  Each Gaussian carries the label of
the class it was built for, and check_classes() asserts every class's membership from render_ref.preprocess and the
camera alone: a scene that stops reaching an arm fails there.  check_scene() asserts the conditions on the whole scene
from render_grad_ref.decisions.

The seeds.  SEEDS holds, per variant, the first seed from 0 on whose scene meets check_classes() and check_scene()
(first_seed() is the search, run on the CPU; scene() asserts the conditions again), as test_gpu_render_scale.DEEP_CASES
records its seeds.

Non-finite inputs.  Seven of the eight non-finite Gaussians fail the preprocess's own finiteness tests.  The eighth, a
NaN alpha on a Gaussian that is otherwise visible, did not: its opacity is not among them, the record carried a NaN
opacity, and the blends read min(0.99, NaN) each in their own way (numpy: NaN, so the pair is dropped; fminf: 0.99, so
the Gaussian blended as an opaque one and its record gradients were NaN).  The rule is the maintainers' "non-finite
inputs become invisible Gaussians": render_ref.preprocess and spz_render_preprocess_kernel now test the opacity too,
and the tests assert that Gaussian invisible, with exact zero gradients."""
import functools

import numpy as np

import render_grad_ref as GR
import render_ref as RR

W, H = 40, 36
NEAR = 0.2
BG = (0.1, 0.2, 0.3)
DEG = 3
SIDES = ("x_pos", "x_neg", "y_pos", "y_neg")
NONFINITE = ("nan_x", "inf_y", "ninf_z", "inf_scale", "nan_scale", "zero_quat", "nan_quat", "nan_alpha")
# variant: (seed, antialiased, width, height).  The seeds: see the module's docstring.
SEEDS = {"plain": 22, "aa": 3, "strip": 7}
VARIANTS = {"plain": (False, W, H), "aa": (True, W, H), "strip": (False, W, 292)}
# the least members of each class (the "at least" column of the class table); per side where the class has sides
AT_LEAST = {"interior": 150, "clamp": 4, "corner": 2, "cut": 4, "behind": 30, "near": 10, "off": 30, "nonfinite": 8}


def frustum_camera(width=W, height=H, max_sh=3):
    """(world_to_camera (3, 4) float32, fx, fy, cx, cy) and the render_ref camera."""
    m = RR.look_at((0.3, -0.2, 0.1), (0.9, 0.5, 4.0), (0.15, 1.0, 0.1))
    fx, fy, cx, cy = 0.9 * height, 1.1 * height, 0.5 * width + 3.25, 0.5 * height - 2.5
    return (m, fx, fy, cx, cy), RR.camera(m, fx, fy, cx, cy, width, height, NEAR, BG, max_sh)


def limits(cam):
    """(lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg) as render_ref.preprocess and make_cam compute them."""
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    Wf, Hf = float(cam["width"]), float(cam["height"])
    return ((Wf - cx) / fx + 0.3 * Wf / fx, cx / fx + 0.3 * Wf / fx,
            (Hf - cy) / fy + 0.3 * Hf / fy, cy / fy + 0.3 * Hf / fy)


def unproject(cam, u, v, z):
    """The camera-frame points that project to the pixel centres (u, v) at depth z, as
    test_gpu_render_scale.unproject."""
    return np.stack([(u + 0.5 - cam["cx"]) * z / cam["fx"], (v + 0.5 - cam["cy"]) * z / cam["fy"], z], axis=1)


def _quat_of(m):
    """The unit quaternion (x, y, z, w) of a rotation matrix."""
    t = np.trace(m)
    if t > 0.0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(m)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k])
        q = [0.0, 0.0, 0.0, (m[k, j] - m[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (m[j, i] + m[i, j]) / s, (m[k, i] + m[i, k]) / s
    return np.asarray(q)


def _place(rng, cam, u, v, z, sigma_px, alpha, colour_lo=-1.5):
    """Gaussians at the pixels (u, v) and depths z, about sigma_px wide on the image: (k, .) float64 arrays.  The world
    size allows for the growth of the footprint off the axis, (1 + qx^2 + qy^2)^(1/2) with the clamped quotients."""
    k = u.size
    pc = unproject(cam, u, v, z)
    pw = (pc - cam["t"][None, :]) @ cam["R"]  # R^T (p_c - t)
    lxp, lxn, lyp, lyn = limits(cam)
    qx, qy = np.clip(pc[:, 0] / pc[:, 2], -lxn, lxp), np.clip(pc[:, 1] / pc[:, 2], -lyn, lyp)
    world = sigma_px * np.abs(z) / (np.sqrt(cam["fx"] * cam["fy"]) * np.sqrt(1.0 + qx * qx + qy * qy))
    q = rng.standard_normal((k, 4))
    return {"positions": pw, "scales": np.log(world)[:, None] + rng.uniform(-0.2, 0.2, (k, 3)),
            "rotations": q / np.linalg.norm(q, axis=1, keepdims=True), "alphas": np.asarray(alpha, dtype=np.float64),
            "colors": rng.uniform(colour_lo, 1.5, (k, 3)),
            "sh": 0.3 * rng.standard_normal((k, RR.SH_DIM[DEG] * 3))}


def _past(rng, side, k, lo, hi, cam):
    """(u, v) of k means lo to hi (fractions of the image's width or height, or pixels when above 1) past `side`, the
    other coordinate inside the image."""
    Wf, Hf = float(cam["width"]), float(cam["height"])
    span = Wf if side[0] == "x" else Hf
    d = rng.uniform(lo, hi, k) * (span if hi <= 1.0 else 1.0)
    u, v = rng.uniform(4.0, Wf - 5.0, k), rng.uniform(4.0, Hf - 5.0, k)
    if side == "x_pos":
        u = Wf - 0.5 + d
    elif side == "x_neg":
        u = -0.5 - d
    elif side == "y_pos":
        v = Hf - 0.5 + d
    else:
        v = -0.5 - d
    return u, v, d


def build(seed, antialiased=False, width=W, height=H, nonfinite=True):
    """The scene of `seed`: dict(cloud (flat float32 arrays), n, deg, aa, labels (n strings: the class each Gaussian was
    built for, "clamp_x_pos", "cut_y_neg", "nan_alpha", ... for the classes with members of their own), view (the
    arguments of abi.render_params), cam).  nonfinite False: without the non-finite class (a packed stream holds none).
    Nothing is asserted here: check_classes() and check_scene() do that."""
    rng = np.random.default_rng(seed)
    view, cam = frustum_camera(width, height)
    Wf, Hf = float(width), float(height)
    parts, labels = [], []

    def add(label, part):
        parts.append(part)
        labels.extend([label] * part["alphas"].size)

    strip = height > 2 * H
    k = 330 if strip else 290  # the crowd: a few pixels wide, inside the image, behind the clamped ones
    add("interior", _place(rng, cam, rng.uniform(1.0, Wf - 2.0, k), rng.uniform(1.0, Hf - 2.0, k),
                           rng.uniform(2.5, 8.0, k), rng.uniform(1.2, 3.3, k), rng.uniform(-0.5, 2.5, k)))
    for side in SIDES:  # past a lim: 0.35 to 0.6 of the width (height) past the edge, wide enough to reach the image
        u, v, d = _past(rng, side, 5, 0.35, 0.6, cam)
        sigma = np.clip(d / 1.8, 8.0, np.inf if strip else 12.0)  # 8 to 12 px; the strip's limits lie further out
        add("clamp_" + side, _place(rng, cam, u, v, rng.uniform(1.0, 1.8, 5), sigma, rng.uniform(0.6, 1.4, 5), -2.5))
    # the corner: past lim_x_pos and lim_y_pos at once
    du, dv = rng.uniform(0.35, 0.42, 3) * Wf, rng.uniform(0.35, 0.42, 3) * Hf
    add("corner", _place(rng, cam, Wf - 0.5 + du, Hf - 0.5 + dv, rng.uniform(1.0, 1.8, 3),
                         np.maximum(12.0, np.hypot(du, dv) / 1.8), rng.uniform(0.6, 1.4, 3), -2.5))
    for side in SIDES:  # 2 to 10 px outside an edge, a few px wide: the rectangle is cut at the grid's edge
        u, v, d = _past(rng, side, 5, 2.0, 10.0, cam)
        sigma = rng.uniform(1.05, 1.4, 5) * (d + 3.0) / 3.0
        add("cut_" + side, _place(rng, cam, u, v, rng.uniform(1.5, 6.0, 5), sigma, rng.uniform(0.0, 2.0, 5)))
    k = 40
    add("behind", _place(rng, cam, rng.uniform(-Wf, 2.0 * Wf, k), rng.uniform(-Hf, 2.0 * Hf, k),
                         -rng.uniform(0.15, 6.0, k), rng.uniform(1.0, 8.0, k), rng.uniform(-0.5, 2.5, k)))
    k = 12
    add("near", _place(rng, cam, rng.uniform(1.0, Wf - 2.0, k), rng.uniform(1.0, Hf - 2.0, k),
                       rng.uniform(0.02, NEAR - 5e-3, k), rng.uniform(1.0, 8.0, k), rng.uniform(-0.5, 2.5, k)))
    # off the image with an empty rectangle: far out on any side (past a lim as well), and 8 to 10.5 px outside the left
    # or the top edge with a radius too small to reach tile 0 (inside every lim)
    k = 24
    far, low = rng.uniform(60.0, 300.0, (2, k)), rng.integers(0, 2, (2, k)) == 0
    pick = rng.integers(0, 3, k)  # far in x, in y, or in both
    u = np.where(pick != 1, np.where(low[0], -far[0], Wf + far[0]), rng.uniform(0.0, Wf, k))
    v = np.where(pick != 0, np.where(low[1], -far[1], Hf + far[1]), rng.uniform(0.0, Hf, k))
    add("off", _place(rng, cam, u, v, rng.uniform(0.5, 8.0, k), rng.uniform(1.0, 3.0, k), rng.uniform(-0.5, 2.5, k)))
    k = 16
    d = rng.uniform(8.0, 10.5, k)
    left = np.arange(k) % 2 == 0
    u = np.where(left, -0.5 - d, rng.uniform(4.0, Wf - 5.0, k))
    v = np.where(left, rng.uniform(4.0, Hf - 5.0, k), -0.5 - d)
    add("off", _place(rng, cam, u, v, rng.uniform(1.0, 8.0, k), rng.uniform(0.5, 1.1, k), rng.uniform(-0.5, 2.5, k)))
    if nonfinite:  # one each, on a Gaussian that would be visible in the middle of the image
        k = len(NONFINITE)
        p = _place(rng, cam, rng.uniform(8.0, Wf - 9.0, k), rng.uniform(8.0, Hf - 9.0, k), rng.uniform(1.9, 2.4, k),
                   rng.uniform(2.0, 3.0, k), np.full(k, 1.0))
        p["positions"][0, 0] = np.nan
        p["positions"][1, 1] = np.inf
        p["positions"][2, 2] = -np.inf
        p["scales"][3, 1] = np.inf
        p["scales"][4, 2] = np.nan
        p["rotations"][5, :] = 0.0
        p["rotations"][6, 3] = np.nan
        p["alphas"][7] = np.nan
        parts.append(p)
        labels.extend(NONFINITE)
    if antialiased:
        # six discs: one log scale of -10 and two of about -2, the thin axis turned from the view direction by a sweep
        # of angles that ends within 2 degrees of edge-on (90), about a seeded axis
        k = 6
        p = _place(rng, cam, rng.uniform(6.0, Wf - 7.0, k), rng.uniform(6.0, Hf - 7.0, k), rng.uniform(2.0, 2.4, k),
                   np.full(k, 2.0), rng.uniform(0.5, 2.0, k))
        campos = -(cam["R"].T @ cam["t"])
        for i, theta in enumerate(np.deg2rad([0.0, 60.0, 85.0, 88.5, 89.5, 89.9])):
            d = p["positions"][i] - campos
            d /= np.linalg.norm(d)
            e = np.cross(d, rng.standard_normal(3))
            e /= np.linalg.norm(e)
            e2 = np.cross(d, e)
            normal = np.cos(theta) * d + np.sin(theta) * e
            p["rotations"][i] = _quat_of(np.stack([normal, e2, np.cross(normal, e2)], axis=1))
            p["scales"][i] = [-10.0, -2.0 + rng.uniform(-0.2, 0.2), -2.0 + rng.uniform(-0.2, 0.2)]
        add("disc", p)
    order = rng.permutation(len(labels))  # shuffled: every wave of the per-Gaussian kernels mixes the classes
    cloud = {key: np.concatenate([q[key] for q in parts])[order].astype(np.float32).reshape(-1) for key in parts[0]}
    return {"cloud": cloud, "n": len(labels), "deg": DEG, "aa": bool(antialiased),
            "labels": np.asarray(labels)[order], "view": view, "cam": cam}


def members(labels, name):
    """The indices of the Gaussians built for class `name` ("clamp": all sides and the corner; "clamp_x_pos": one side;
    "nonfinite": the eight)."""
    labels = np.asarray(labels)
    if name == "nonfinite":
        return np.nonzero(np.isin(labels, NONFINITE))[0]
    if name == "clamp":
        return np.nonzero(np.char.startswith(labels, "clamp_") | (labels == "corner"))[0]
    if name == "cut":
        return np.nonzero(np.char.startswith(labels, "cut_"))[0]
    return np.nonzero(labels == name)[0]


def quotients(rec, cam):
    """Per Gaussian, what the clamp of J does: (past (n, 4) bool: x / z above lim_x_pos, below -lim_x_neg, y / z above
    lim_y_pos, below -lim_y_neg, each by more than 1e-6 relative; free_x, free_y (n) bool: inside both limits of that
    axis by more than 1e-6 relative).  A quotient that is neither lies within 1e-6 of a lim."""
    p = rec["camera_xyz"]
    with np.errstate(all="ignore"):
        qx, qy = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        lxp, lxn, lyp, lyn = limits(cam)
        hi, lo = 1.0 + 1e-6, 1.0 - 1e-6
        past = np.stack([qx > lxp * hi, qx < -lxn * hi, qy > lyp * hi, qy < -lyn * hi], axis=1)
        free_x = (qx < lxp * lo) & (qx > -lxn * lo)
        free_y = (qy < lyp * lo) & (qy > -lyn * lo)
    return past, free_x, free_y


def pixels_used(dec):
    """Per Gaussian, the number of pixels whose blend uses it."""
    used = np.zeros(dec["visible"].size, dtype=np.int64)
    for tile in dec["tiles"]:
        if len(tile["sel"]):
            np.add.at(used, tile["sel"], tile["take"].sum(axis=0))
    return used


def check_classes(s, rec, dec=None):
    """The class table, from the reference's records `rec` (render_ref.preprocess of s["cloud"], or of a cloud decoded
    from its packed form) and the camera.  dec: the decisions, for the classes that must be used by pixels (None: that
    column is not checked).  Returns the class counts."""
    cam, labels = s["cam"], s["labels"]
    vis = rec["visible"]
    past, free_x, free_y = quotients(rec, cam)
    z = rec["camera_xyz"][:, 2]
    mean = rec["mean"].astype(np.float64)
    tw, th = RR.tiles(cam)
    rect = rec["rect"]
    used = pixels_used(dec) if dec is not None else None
    counts = {}

    def count(name, idx, least):
        counts[name] = int(idx.size)
        assert idx.size >= least, f"{name}: {idx.size} members, {least} wanted"

    i = members(labels, "interior")
    count("interior", i, AT_LEAST["interior"])
    assert vis[i].all() and free_x[i].all() and free_y[i].all(), "interior: visible with both quotients free"
    assert ((mean[i, 0] > -0.5) & (mean[i, 0] < cam["width"] - 0.5) & (mean[i, 1] > -0.5)
            & (mean[i, 1] < cam["height"] - 0.5)).all(), "interior: the mean lies inside the image"
    for k, side in enumerate(SIDES):
        i = members(labels, "clamp_" + side)
        count("clamp_" + side, i, AT_LEAST["clamp"])
        assert vis[i].all(), f"clamp_{side}: visible"
        assert past[i, k].all(), f"clamp_{side}: the quotient lies past its own lim"
        other_free = free_y if side[0] == "x" else free_x
        assert other_free[i].all(), f"clamp_{side}: the other quotient is free"
        if used is not None:
            assert (used[i] >= 20).all(), f"clamp_{side}: used by {used[i]} pixels, 20 each wanted"
        i = members(labels, "cut_" + side)
        count("cut_" + side, i, AT_LEAST["cut"])
        assert vis[i].all() and free_x[i].all() and free_y[i].all(), f"cut_{side}: visible with free quotients"
        at_edge = (rect[i, 2] == tw, rect[i, 0] == 0, rect[i, 3] == th, rect[i, 1] == 0)[k]
        outside = (mean[i, 0] > cam["width"] - 0.5, mean[i, 0] < -0.5, mean[i, 1] > cam["height"] - 0.5,
                   mean[i, 1] < -0.5)[k]
        assert at_edge.all() and outside.all(), f"cut_{side}: the mean lies outside and the rectangle ends at the edge"
    assert sum(counts["clamp_" + side] for side in SIDES) >= 16
    i = members(labels, "corner")
    count("corner", i, AT_LEAST["corner"])
    assert vis[i].all() and past[i, 0].all() and past[i, 2].all(), "corner: visible, both quotients clamped"
    if used is not None:
        assert (used[i] >= 1).all(), f"corner: used by {used[i]} pixels"
    i = members(labels, "behind")
    count("behind", i, AT_LEAST["behind"])
    assert (z[i] < -0.1).all() and not vis[i].any(), "behind: z < -0.1, invisible"
    i = members(labels, "near")
    count("near", i, AT_LEAST["near"])
    assert ((z[i] > 0.01) & (z[i] < cam["near"] - 1e-3)).all() and not vis[i].any(), "near: 0.01 < z < near, invisible"
    i = members(labels, "off")
    count("off", i, AT_LEAST["off"])
    assert (z[i] > cam["near"]).all() and not vis[i].any(), "off: in front of near, invisible"
    with np.errstate(all="ignore"):
        finite = np.isfinite(rec["r3"][i]).all() and (rec["det0"][i] + 0.3 > 0).all()
    assert finite, "off: nothing but the empty rectangle hides them"
    n_past, n_free = int(past[i].any(axis=1).sum()), int((free_x[i] & free_y[i]).sum())
    assert n_past >= 5 and n_free >= 5, f"off: {n_past} past a lim and {n_free} inside every lim, 5 each wanted"
    counts["off_past_a_lim"], counts["off_inside_the_lims"] = n_past, n_free
    i = members(labels, "nonfinite")
    if i.size:
        count("nonfinite", i, AT_LEAST["nonfinite"])
        assert not vis[i].any(), f"non-finite: {labels[i][vis[i]]} visible; non-finite inputs are invisible Gaussians"
    i = members(labels, "disc")
    if i.size:
        counts["disc"] = int(i.size)
        assert vis[i].all(), "disc: visible"
    counts["visible"], counts["n"] = int(vis.sum()), int(vis.size)
    return counts


def check_scene(s, dec, whole=True):
    """The conditions on the whole scene, from the reference.  whole False (the strip): those on the records only; the
    blend's counts (stopped pixels) are the small scene's business."""
    rec, cam, labels = dec["rec"], s["cam"], s["labels"]
    vis = rec["visible"]
    n = s["n"]
    assert dec["marginal"] == 0, f"{dec['marginal']} marginal pairs: choose another seed"
    r3 = rec["r3"][vis]
    assert (np.abs(r3 - np.round(r3)) >= 1e-4).all(), "a visible Gaussian's r3 lies within 1e-4 of an integer"
    z = rec["camera_xyz"][:, 2]
    assert not (np.abs(z - cam["near"]) < 1e-3).any(), "a z lies within 1e-3 of near"
    past, free_x, free_y = quotients(rec, cam)
    fin = np.isfinite(rec["camera_xyz"]).all(axis=1) & (z > 0)
    assert (past[fin, :2].any(axis=1) | free_x[fin]).all() and (past[fin, 2:].any(axis=1) | free_y[fin]).all(), \
        "a quotient lies within 1e-6 relative of its lim"
    if whole:
        assert 256 < n <= 500, f"n = {n}: two workgroups of the per-Gaussian kernels, the second one partial, wanted"
    assert n % 64 != 0, "n is a multiple of the wave size"
    for a in range(0, n - 63):  # every 64 consecutive indices, whole waves among them
        w = vis[a:a + 64]
        assert w.any() and not w.all(), f"the Gaussians {a} to {a + 63} are all visible or all invisible"
    c = members(labels, "clamp")
    assert (rec["rgb"][c] == 0.0).any(), "no rgb channel of a clamped-quotient Gaussian is clamped at 0"
    if whole:
        assert dec["stopped"] >= 150, f"{dec['stopped']} pixels reach the stop, 150 wanted"
    if s["aa"]:
        d = members(labels, "disc")
        det0, a0c0 = rec["det0"][d], rec["a0c0"][d]
        assert (np.abs(det0) >= 1e-12 * a0c0).all(), "a disc's det0 is below 1e-12 of a0 c0: leave it out"
        pos = det0[det0 > 0]
        assert pos.size >= 2 and pos.max() / pos.min() >= 1e4, f"the discs' det0 span {pos.max() / pos.min():.3g}"
        assert (rec["opacity"][d][det0 <= 0] == 0.0).all(), "a disc with det0 <= 0 has an opacity"
    return {"marginal": dec["marginal"], "stopped": dec["stopped"], "entries": dec["entries"], "used": dec["used"],
            "clamped_alpha_pairs": dec["clamped"]}


def first_seed(variant, start=0, tries=200):
    """The first seed from `start` on whose scene meets check_classes() and check_scene(): how SEEDS was chosen."""
    aa, width, height = VARIANTS[variant]
    for seed in range(start, start + tries):
        s = build(seed, aa, width, height)
        try:
            dec = GR.decisions(s["cloud"], s["deg"], s["cam"], aa, vectorised=True)
            check_classes(s, dec["rec"], dec)
            check_scene(s, dec, whole=variant != "strip")
        except AssertionError:
            continue
        return seed
    raise AssertionError(f"no seed in [{start}, {start + tries}) gives a {variant} scene")


@functools.lru_cache(maxsize=None)
def scene(variant):
    """The variant's scene with its decisions ("dec"), class counts ("counts") and scene facts ("facts"), asserted;
    computed once and shared (nothing changes it)."""
    aa, width, height = VARIANTS[variant]
    s = build(SEEDS[variant], aa, width, height)
    dec = GR.decisions(s["cloud"], s["deg"], s["cam"], aa, vectorised=True)
    s["dec"] = dec
    s["counts"] = check_classes(s, dec["rec"], dec)
    s["facts"] = check_scene(s, dec, whole=variant != "strip")
    return s


def finite_part(s):
    """The scene without its non-finite class, in the same order (what a packed stream can hold): a scene dict with
    "kept", the indices into s."""
    keep = np.nonzero(~np.isin(s["labels"], NONFINITE))[0]
    n = s["n"]
    cloud = {k: v.reshape(n, -1)[keep].reshape(-1) for k, v in s["cloud"].items()}
    out = dict(s, cloud=cloud, n=int(keep.size), labels=s["labels"][keep], kept=keep)
    for k in ("dec", "counts", "facts"):
        out.pop(k, None)
    return out


def chain_to_cloud(cloud_np, sh_degree, cam, dec, record_grads, antialiased=False, dtype=None):
    """The chain from given record gradients (n, 9) to the cloud's six arrays, by autograd of
    render_grad_ref.records (float64): what preprocess_backward_one computes.  Flat float64 arrays keyed like the cloud,
    exact zero rows for the invisible Gaussians (they are indexed out before any arithmetic, so nothing non-finite in
    them reaches a product)."""
    import torch
    dtype = dtype or torch.float64
    cloud = GR.as_tensors(cloud_np, dtype)
    idx = np.nonzero(dec["visible"])[0]
    w = torch.as_tensor(np.asarray(record_grads, dtype=np.float64)[idx]).to(dtype)
    (GR.records(cloud, sh_degree, cam, idx, antialiased) * w).sum().backward()
    return {k: (t.grad if t.grad is not None else torch.zeros_like(t)).to(torch.float64).numpy()
            for k, t in cloud.items()}


def rows_of(a, n):
    """A gradient array (flat, or (n, .)) as float64 rows per Gaussian."""
    return np.asarray(a, dtype=np.float64).reshape(n, -1)
