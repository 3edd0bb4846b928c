"""A float64 numpy restatement of the seed contract (include/spz_amd.h "seed"; DESIGN §8 "Seed"): the sample lattice, the
validity tests, the cover test against a rendered alpha and accumulated depth, the selection with its capacity cut, and
the Gaussian each selected sample becomes.  Every operation is written in the contract's order; numpy does not
contract a product and a sum, so each is rounded on its own as the device rounds it.

A view is a dict: world_to_camera (3, 4) float32, fx, fy, cx, cy, width, height, near (the float32 values the device
reads).  opts is a dict: stride, scale_factor, alpha (pre-sigmoid), cover_alpha, cover_tolerance, cover, sh_degree."""
import numpy as np

C0 = 0.28209479177387814
SH_DIM = {0: 0, 1: 3, 2: 8, 3: 15}
VALID, SELECTED = 1, 2
FIELDS = ("positions", "scales", "rotations", "alphas", "colors", "sh")


def options(stride=1, scale_factor=1.0, opacity=0.5, cover_alpha=0.5, cover_tolerance=0.05, cover=True, sh_degree=0):
    """The options as the device reads them: the floats rounded to float32, opacity turned into alpha once."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    return {"stride": int(stride), "scale_factor": f(scale_factor), "alpha": f(np.log(opacity / (1.0 - opacity))),
            "cover_alpha": f(cover_alpha), "cover_tolerance": f(cover_tolerance), "cover": bool(cover),
            "sh_degree": int(sh_degree)}


def view(world_to_camera, fx, fy, cx, cy, width, height, near=0.2):
    f = lambda v: float(np.float32(v))  # noqa: E731
    return {"world_to_camera": np.asarray(world_to_camera, np.float32).reshape(3, 4), "fx": f(fx), "fy": f(fy),
            "cx": f(cx), "cy": f(cy), "width": int(width), "height": int(height), "near": f(near)}


def lattice(width, height, stride):
    """The sample pixels (u, v) in lattice order (row-major in (j, i)) and the lattice's size (lw, lh)."""
    us = np.arange(stride // 2, width, stride, dtype=np.int64)
    vs = np.arange(stride // 2, height, stride, dtype=np.int64)
    vv, uu = np.meshgrid(vs, us, indexing="ij")
    return uu.ravel(), vv.ravel(), (len(us), len(vs))


def samples(width, height, stride):
    return len(range(stride // 2, width, stride)) * len(range(stride // 2, height, stride))


def empty_cloud(capacity, sh_degree):
    per = {"positions": 3, "scales": 3, "rotations": 4, "alphas": 1, "colors": 3, "sh": 3 * SH_DIM[sh_degree]}
    return {k: np.zeros(capacity * per[k], np.float32) for k in FIELDS}


def select(vw, image, depth, weights, cover_image, cover_depth, opts, room=None, why=None):
    """flags (one uint8 per lattice sample: bit 0 valid, bit 1 selected) and counts (valid, appended, refused) with
    `room` places left (None: no limit).  cover_image (H, W, 4) and cover_depth (H, W, 2), float32, or None for no
    cover test.  why (a dict, optional) gets the number of samples that left at each test."""
    u, v, _ = lattice(vw["width"], vw["height"], opts["stride"])
    image, depth = np.asarray(image, np.float32), np.asarray(depth, np.float32)
    d = depth[v, u]
    with np.errstate(invalid="ignore"):
        measured = np.isfinite(d) & (d > np.float32(vw["near"]))
        counted = np.ones_like(measured) if weights is None else np.asarray(weights, np.float32)[v, u] > np.float32(0.5)
        coloured = np.isfinite(image[v, u, :3]).all(axis=1)
        valid = measured & counted & coloured
        covered = np.zeros_like(valid)
        if cover_image is not None:
            A = np.asarray(cover_image, np.float32)[v, u, 3]
            acc = np.asarray(cover_depth, np.float32)[v, u, 0]
            opaque = A >= np.float32(opts["cover_alpha"])
            with np.errstate(divide="ignore"):
                e = (acc / A).astype(np.float32)  # the f32 division of expected_depth()
            near = np.abs(e.astype(np.float64) - d.astype(np.float64)) <= opts["cover_tolerance"] * d.astype(np.float64)
            covered = valid & opaque & near
            if why is not None:
                why["alpha_low"] = int((valid & ~opaque).sum())
                why["depth_in_front"] = int((valid & opaque & ~near & (e < d)).sum())
                why["depth_behind"] = int((valid & opaque & ~near & (e > d) & np.isfinite(e)).sum())
                why["depth_not_finite"] = int((valid & opaque & ~np.isfinite(e)).sum())
                why["covered"] = int(covered.sum())
    if why is not None:
        why["no_depth"] = int((~measured).sum())
        why["no_weight"] = int((measured & ~counted).sum())
        why["no_colour"] = int((measured & counted & ~coloured).sum())
        why["selected"] = int((valid & ~covered).sum())
    selected = valid & ~covered
    flags = (valid * VALID + selected * SELECTED).astype(np.uint8)
    total = int(selected.sum())
    appended = total if room is None else min(total, int(room))
    return flags, (int(valid.sum()), appended, total - appended)


def emit(vw, image, depth, flags, opts, cloud, n, appended):
    """Write the first `appended` selected samples, in lattice order, into the six arrays of `cloud` at n + rank."""
    u, v, _ = lattice(vw["width"], vw["height"], opts["stride"])
    take = np.nonzero(flags & SELECTED)[0][:appended]
    u, v = u[take], v[take]
    M = vw["world_to_camera"].astype(np.float64)
    R, t = M[:, :3], M[:, 3]
    fx, fy, cx, cy = (np.float64(vw[k]) for k in ("fx", "fy", "cx", "cy"))
    z = np.asarray(depth, np.float32)[v, u].astype(np.float64)
    qx = ((u.astype(np.float64) + 0.5 - cx) / fx) * z - t[0]
    qy = ((v.astype(np.float64) + 0.5 - cy) / fy) * z - t[1]
    qz = z - t[2]
    pos = np.stack([(qx * R[0, k] + qy * R[1, k]) + qz * R[2, k] for k in range(3)], axis=1).astype(np.float32)
    ls = np.log((((np.float64(opts["scale_factor"]) * np.float64(opts["stride"])) * z) * 0.5) * (1.0 / fx + 1.0 / fy))
    rgb = np.asarray(image, np.float32)[v, u, :3].astype(np.float64)
    col = ((rgb - 0.5) / C0).astype(np.float32)
    k = len(take)
    sh3 = 3 * SH_DIM[opts["sh_degree"]]
    cloud["positions"][3 * n: 3 * (n + k)] = pos.ravel()
    cloud["scales"][3 * n: 3 * (n + k)] = np.repeat(ls.astype(np.float32), 3)
    cloud["rotations"][4 * n: 4 * (n + k)] = np.tile(np.array([0, 0, 0, 1], np.float32), k)
    cloud["alphas"][n: n + k] = np.float32(opts["alpha"])
    cloud["colors"][3 * n: 3 * (n + k)] = col.ravel()
    cloud["sh"][sh3 * n: sh3 * (n + k)] = 0.0
    return n + k


def seed_loop(views, images, depths, weights, opts, capacity, render_depth, cloud=None, n=0):
    """The loop: per view, with cover set and n > 0, render_depth(cloud, n, view) -> (cover_image (H, W, 4), cover_depth
    (H, W, 2)) float32 of the first n Gaussians; select; emit.  Returns (cloud, n, counts per view)."""
    if cloud is None:
        cloud = empty_cloud(capacity, opts["sh_degree"])
    counts = []
    for k, vw in enumerate(views):
        ci = cd = None
        if opts["cover"] and n > 0:
            ci, cd = render_depth(cloud, n, vw)
        w = None if weights is None else weights[k]
        flags, got = select(vw, images[k], depths[k], w, ci, cd, opts, room=capacity - n)
        n = emit(vw, images[k], depths[k], flags, opts, cloud, n, got[1])
        counts.append(got)
    return cloud, n, counts


def ulp_distance(a, b):
    """The distance in float32 steps between two arrays of finite floats of one sign."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64)
                  - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


# ---- files as the tools read them ------------------------------------------------------------------------------------
def write_pfm(path, pixels, magic):
    """A PFM as spz_render writes it (little-endian, rows bottom to top): magic b"Pf" (pixels (h, w)) or b"PF"
    ((h, w, 3))."""
    h, w = pixels.shape[:2]
    with open(path, "wb") as f:
        f.write(magic + b"\n" + f"{w} {h}\n".encode() + b"-1.0\n")
        f.write(np.ascontiguousarray(pixels[::-1]).astype("<f4").tobytes())


def write_views(path, views):
    """A views file (spz::loadViewsFile): width height fx fy cx cy and the 3x4 matrix, one view per line."""
    with open(path, "w") as f:
        for v in views:
            m = np.asarray(v["world_to_camera"], np.float32).reshape(-1)
            f.write(" ".join([str(v["width"]), str(v["height"])] + [repr(float(np.float32(v[k]))) for k in
                                                                     ("fx", "fy", "cx", "cy")]
                             + [repr(float(x)) for x in m]) + "\n")
