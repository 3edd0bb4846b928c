"""The per-view step that prune, compare and refine share (spz_amd/csrc/spz_view_pass.hpp) on the GPU: the two places
where it allocates the render workspace again.

Growing totals within one call: one camera at 16 x 16, 48 x 32 and 128 x 96 (intrinsics scaled) behind a view turned
away from the scene, so the entry totals are 0 and then strictly increasing (asserted from single-view renders): in this
order the workspace grows at every view, in the reverse order never after the first.  A 2000-point SH3 scene and its SH0
copy.

A prepare part that grows between sources: a 300-point file against a 3000-point file over the turned-away view and an
ordinary one.  The small file's first view has no entries, so the workspace it leaves is smaller than the large file's
prepare part (asserted from spz_amd_render_workspace_bytes) and is freed and allocated again while the stream is live.

Everything is compared bit for bit: compare_spz against compare_images of the single-view renders, prune's sums and
maxima against the single-view calls', refine's "before" metrics against compare_spz's."""
import functools
import gzip

import numpy as np
import pytest
import torch

import render_ref as RR
from test_gpu_compare import as_vec, check_views
from test_gpu_prune import gz, scene

pytestmark = pytest.mark.gpu

COORD = 4  # RUB (spz.RUB in the file layer), the frame the scenes are encoded from
SIZES = ((16, 16), (48, 32), (128, 96))


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def camera_views(positions, sizes, away_size=(48, 32)):
    """A view turned away from the positions, then one camera looking at them at every size (fx, fy, cx, cy scaled from
    the largest).  The eye is outside the positions' box, so the first view has every point behind it."""
    p = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in positions])
    lo, hi = p.min(axis=0), p.max(axis=0)
    c, ext = 0.5 * (lo + hi), float(max(hi - lo))
    eye = c + 2.2 * ext * np.array([np.sin(0.4), 0.2, -np.cos(0.4)])
    W, H = max(sizes)
    f = 4.0 * H  # a long lens: the splats span several tiles at the largest size, so the totals grow with the size

    def view(m, w, h):
        return {"world_to_camera": m, "fx": f * w / W, "fy": f * h / H, "cx": 0.5 * w, "cy": 0.5 * h, "width": w,
                "height": h}

    toward, away = RR.look_at(eye, c, [0, 1, 0]), RR.look_at(eye, 2 * eye - c, [0, 1, 0])
    return [view(away, *away_size)] + [view(toward, w, h) for w, h in sizes]


def params_of(v):
    from spz_amd import abi
    return abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"], 0.2,
                             (0.0, 0.0, 0.0), 3, COORD)


def entry_totals(stream, hdr, views):
    from spz_amd import device as D
    return [int(D.render_packed(stream, hdr, params_of(v), return_info=True)[1].cpu()[0]) for v in views]


def resident(path, cuda):
    """A written file's stream on the device, with its header."""
    from spz_amd import abi
    raw = gzip.decompress(path.read_bytes())
    rc, h = abi.peek_header(raw)
    assert rc == 0
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(cuda), h, raw


@pytest.fixture(scope="module")
def growing(cuda, spz, tmp_path_factory):
    """The scene's file, its SH0 copy, and the four views whose totals are 0 and then strictly increasing."""
    d = tmp_path_factory.mktemp("view_pass")
    c, (stream, hdr) = scene(cuda, 2000, 3, 23, False)
    full, sh0 = d / "full.spz", d / "sh0.spz"
    full.write_bytes(gz(stream.cpu().numpy().tobytes()))
    spz.filter_spz(str(full), str(sh0), sh_degree=0)
    views = camera_views([c["positions"]], SIZES)
    totals = entry_totals(stream, hdr, views)
    print("entry totals", totals)
    assert totals[0] == 0 and all(a < b for a, b in zip(totals, totals[1:])), totals
    return {"full": full, "sh0": sh0, "views": views, "n": 2000, "dir": d}


def test_compare_over_growing_totals(cuda, spz, growing):
    g = growing
    for views in (g["views"], g["views"][::-1]):
        got = check_views(spz, g["sh0"], g["full"], views, spz.RUB, reference=False)
        assert all(m["mse"] > 0.0 for m, v in zip(got, views) if v is not g["views"][0])


def test_prune_over_growing_totals(cuda, spz, growing):
    g = growing
    out = str(g["dir"] / "pruned.spz")

    def scores(views):
        _, _, s, x = spz.prune_spz(str(g["full"]), out, views, keep=g["n"], coord=spz.RUB, return_scores=True)
        assert s.dtype == np.uint64 and x.dtype == np.float32
        return s, x

    single = [scores([v]) for v in g["views"]]
    assert not single[0][0].any() and not single[0][1].any(), "the turned-away view scores nothing"
    want_sum = functools.reduce(np.add, [s for s, _ in single])
    want_max = functools.reduce(np.maximum, [x for _, x in single])
    assert want_sum.any()
    for views in (g["views"], g["views"][::-1]):
        s, x = scores(views)
        assert np.array_equal(s, want_sum)
        assert np.array_equal(x.view(np.uint32), want_max.view(np.uint32))


@pytest.mark.parametrize("iterations", [0, 4])
def test_refine_over_growing_totals(cuda, spz, growing, iterations):
    """iterations = 4 is one pass over the views.  The "before" metrics are compare_spz's; two runs give the same output
    and history.  The backward sums with f32 atomics, and include/spz_amd.h "render backward" lets two runs differ in
    the last bits; at this size (one step without gradients, then views of 1, 6 and 48 tiles) the runs measured on an
    MI355X gave the same bits: history 0.0, 0.08487617001509508, 0.06493576969460364, 0.04028612797316878 both times
    and no differing output byte."""
    from spz_amd import device as D
    g = growing
    a_t, ha, _ = resident(g["sh0"], cuda)
    b_t, hb, _ = resident(g["full"], cuda)
    params = [params_of(v) for v in g["views"]]
    want = spz.compare_spz(str(g["sh0"]), str(g["full"]), g["views"], coord=spz.RUB)
    runs = []
    for _ in range(2):
        with D.refine_packed(a_t, ha, b_t, hb, params, iterations) as res:
            runs.append((res.fetch().copy(), res.report))
    for out, rep in runs:
        assert len(rep["history"]) == iterations
        for k, (m, w) in enumerate(zip(rep["before"], want)):
            assert np.array_equal(as_vec(m).view(np.uint64), as_vec(w).view(np.uint64)), k
    if iterations:
        print("history", runs[0][1]["history"], runs[1][1]["history"])
        print("output bytes that differ between the runs", int((runs[0][0] != runs[1][0]).sum()))
    else:
        assert np.array_equal(runs[0][0], a_t.cpu().numpy())
    assert np.array_equal(np.float64(runs[0][1]["history"]).view(np.uint64),
                          np.float64(runs[1][1]["history"]).view(np.uint64))
    assert np.array_equal(runs[0][0], runs[1][0])


@pytest.fixture(scope="module")
def two_sizes(cuda, spz, tmp_path_factory):
    """A 300-point and a 3000-point file, the turned-away view and an ordinary one."""
    from spz_amd import abi
    d = tmp_path_factory.mktemp("view_pass_sources")
    cs, (small_t, small_h) = scene(cuda, 300, 3, 29, False)
    cl, (large_t, large_h) = scene(cuda, 3000, 3, 31, False)
    small, large = d / "small.spz", d / "large.spz"
    small.write_bytes(gz(small_t.cpu().numpy().tobytes()))
    large.write_bytes(gz(large_t.cpu().numpy().tobytes()))
    views = camera_views([cs["positions"], cl["positions"]], SIZES[1:2], away_size=SIZES[0])
    ts, tl = entry_totals(small_t, small_h, views), entry_totals(large_t, large_h, views)
    print("entry totals", ts, tl)
    assert ts[0] == 0 and tl[0] == 0 and ts[1] > 0 and tl[1] > 0
    # what the small file's first view leaves is smaller than the large file's prepare part
    L = abi.load_library()
    assert L.spz_amd_render_workspace_bytes(300, 0) < L.spz_amd_render_workspace_bytes(3000, 0)
    return {"small": small, "large": large, "views": views}


def test_compare_sources_of_two_sizes(cuda, spz, two_sizes):
    t = two_sizes
    check_views(spz, t["small"], t["large"], t["views"], spz.RUB, reference=False)
    check_views(spz, t["large"], t["small"], t["views"], spz.RUB, reference=False)


@pytest.mark.parametrize("order", ["small_to_large", "large_to_small"])
def test_refine_sources_of_two_sizes(cuda, spz, two_sizes, order):
    from spz_amd import device as D
    t = two_sizes
    fa, fb = (t["small"], t["large"]) if order == "small_to_large" else (t["large"], t["small"])
    a_t, ha, raw_a = resident(fa, cuda)
    b_t, hb, _ = resident(fb, cuda)
    want = spz.compare_spz(str(fa), str(fb), t["views"], coord=spz.RUB)
    with D.refine_packed(a_t, ha, b_t, hb, [params_of(v) for v in t["views"]], 0) as res:
        assert res.fetch().tobytes() == raw_a
        for k, (m, w) in enumerate(zip(res.report["before"], want)):
            assert np.array_equal(as_vec(m).view(np.uint64), as_vec(w).view(np.uint64)), k
