"""Readers of camera sets for prune_spz (DESIGN §8 "Prune") and the back-projection of depth maps (DESIGN §8 "Render"):
plain Python, no device work."""
import json

import numpy as np

_KEYS = ("width", "height", "fx", "fy", "position", "rotation")


def load_3dgs_cameras(path):
    """The views of the cameras.json that the original 3DGS training writes, as prune_spz's view dicts.

    Each entry has width, height, fx, fy, position (the camera centre) and rotation (the camera-to-world 3x3, OpenCV
    axes); so R = rotation^T, t = -rotation^T position, and cx, cy = width / 2, height / 2.  Those cameras live in the
    frame of the training .ply, so the views are meant for coord=RDF (prune_spz(..., coord=spz.RDF)).  ValueError on an
    entry without those fields or of the wrong shape."""
    with open(path, "r", encoding="utf-8") as f:
        data = json.load(f)
    if not isinstance(data, list):
        raise ValueError(f"{path}: expected a JSON list of cameras")
    views = []
    for k, e in enumerate(data):
        if not isinstance(e, dict) or any(key not in e for key in _KEYS):
            raise ValueError(f"{path}: camera {k} lacks one of {', '.join(_KEYS)}")
        rot = np.asarray(e["rotation"], dtype=np.float64)
        pos = np.asarray(e["position"], dtype=np.float64).reshape(-1)
        if rot.shape != (3, 3) or pos.shape != (3,):
            raise ValueError(f"{path}: camera {k}: rotation must be 3x3 and position three values")
        R = rot.T
        t = -R @ pos
        m = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
        width, height = int(e["width"]), int(e["height"])
        views.append({"world_to_camera": m, "fx": float(e["fx"]), "fy": float(e["fy"]), "cx": width / 2.0,
                      "cy": height / 2.0, "width": width, "height": height})
    return views


def unproject_depth(depth, world_to_camera, fx, fy, cx, cy):
    """The world points of a depth map (render_depth_spz's expected or median): (K, 3) float64, one per finite pixel in
    row-major order, in the frame of world_to_camera (the render's `coord` frame).

    depth: (height, width), the camera-space z of each pixel.  Pixel (u, v) is centred at (u + 0.5, v + 0.5), as in the
    render contract, so its ray is ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1) and the point is R^T (z ray - t).
    ValueError when depth is not two-dimensional or world_to_camera is not 3x4."""
    d = np.asarray(depth, dtype=np.float64)
    m = np.asarray(world_to_camera, dtype=np.float64)
    if d.ndim != 2:
        raise ValueError(f"depth must be (height, width), got shape {d.shape}")
    if m.shape != (3, 4):
        raise ValueError(f"world_to_camera must be 3x4, got shape {m.shape}")
    v, u = np.nonzero(np.isfinite(d))
    z = d[v, u]
    cam = np.stack([(u + 0.5 - cx) / fx * z, (v + 0.5 - cy) / fy * z, z], axis=1)
    return (cam - m[:, 3]) @ m[:, :3]
