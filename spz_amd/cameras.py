"""Readers of camera sets for prune_spz (DESIGN §8 "Prune"): plain Python, no device work."""
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
