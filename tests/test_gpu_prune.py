"""spz.prune_spz / spz_prune / spz_amd_render_score_device / spz_amd.device.score + score_packed (DESIGN §8 "Prune") on
the GPU, against the float64 restatement of tests/prune_ref.py: weight_sum within 1e-4 relative (or 1e-6 pixels) and
weight_max within 1e-5 for at least 99.9 % of the Gaussians, a few pixels' weight everywhere; a stream and its decoded
floats, two runs, a side stream, a file and its sorted copy bit for bit; the score kernel's image and the render's; the
sums against the images' alpha; removal of the zero-score points; the output against filter_spz's; the CLI."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import prune_ref as PR
import render_ref as RR
from conftest import ROOT
from test_filter_host import golden_streams

pytestmark = pytest.mark.gpu

Q = 2.0 ** -24


@pytest.fixture(scope="module")
def spz(cuda):
    import spz_amd.spz as m
    return m


def gz(b):
    co = zlib.compressobj(-1, zlib.DEFLATED, 16 + 15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(b) + co.flush()


def to_np(cloud_t):
    return {k: v.cpu().numpy() for k, v in cloud_t.items()}


def scene(cuda, n, deg, seed, aa, clustered=True, alpha_cap=None):
    from spz_amd import abi, device as D
    from spz_amd.synth import make_cloud_clustered, make_cloud_numpy
    c = make_cloud_clustered(n, deg, seed, clusters=32, sigma=0.8) if clustered else make_cloud_numpy(n, deg, seed)
    c["scales"] = (c["scales"] * 0.5 - 1.5).astype(np.float32)
    c["alphas"] = (c["alphas"] * 0.5).astype(np.float32)
    if alpha_cap is not None:
        c["alphas"] = np.minimum(c["alphas"], alpha_cap).astype(np.float32)
    return c, encode(cuda, c, n, deg, aa)


def encode(cuda, c, n, deg, aa):
    from spz_amd import abi, device as D
    stream = D.encode(D.to_device(c, cuda), n, deg, aa, abi.RUB, 3)
    rc, h = abi.peek_header(stream.cpu().numpy().tobytes())
    assert rc == 0
    return stream, h


def ring_views(positions, k, width, height, up, coord, seed=0, dist=2.2):
    """k cameras around the middle of the positions (5th..95th percentile box), looking at its centre."""
    from spz_amd import abi
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    lo, hi = np.percentile(p, 5, axis=0), np.percentile(p, 95, axis=0)
    c = 0.5 * (lo + hi)
    ext = float(max(hi - lo)) or 1.0
    rng = np.random.default_rng(seed)
    params, cams = [], []
    for j in range(k):
        a = 2 * np.pi * j / k + rng.uniform(0, 0.3)
        eye = c + ext * dist * np.array([np.sin(a), rng.uniform(-0.3, 0.3), -np.cos(a)])
        m = RR.look_at(eye, c, up)
        f = 0.9 * height
        cx, cy = 0.5 * width + 1.25, 0.5 * height - 0.75
        params.append(abi.render_params(m, f, f, cx, cy, width, height, coord=coord))
        cams.append(RR.camera(m, f, f, cx, cy, width, height))
    return params, cams


def check_scores(wsum_q, wmax, want_sum, want_max):
    got = wsum_q.astype(np.float64) * Q
    err = np.abs(got - want_sum)
    ok = err <= np.maximum(1e-4 * np.abs(want_sum), 1e-6)
    assert ok.mean() >= 0.999, f"weight_sum: only {ok.mean():.5f} within tolerance (worst {err.max()})"
    assert err.max() <= 3.0, f"weight_sum off by {err.max()} pixels"
    errm = np.abs(wmax.astype(np.float64) - want_max)
    okm = errm <= 1e-5
    assert okm.mean() >= 0.999, f"weight_max: only {okm.mean():.5f} within 1e-5 (worst {errm.max()})"
    assert (want_sum > 0).sum() > 0.2 * want_sum.size, "the views see too little of the scene"


CASES = [(0, False, 4, 3, 70, 45), (3, True, 6, 5, 93, 61), (1, False, 6, 8, 50, 37), (3, False, 4, 4, 81, 29)]


@pytest.mark.parametrize("deg,aa,coord,k,w,h", CASES)
def test_scores_match_the_reference(cuda, deg, aa, coord, k, w, h):
    import torch
    from spz_amd import device as D
    n = 1200 + 200 * deg
    _, (stream, hdr) = scene(cuda, n, deg, 31 + deg, aa)
    floats = to_np(D.decode(stream, hdr, coord))
    up = (0.0, 1.0, 0.0) if coord == 4 else (0.0, -1.0, 0.0)
    params, cams = ring_views(floats["positions"], k, w, h, up, coord, seed=deg)
    wsum, wmax = D.score_packed(stream, hdr, params)
    assert wsum.dtype == torch.int64 and wmax.dtype == torch.float32
    want_sum, want_max = PR.scores(floats, deg, cams, aa)
    check_scores(wsum.cpu().numpy(), wmax.cpu().numpy(), want_sum, want_max)
    # zero exactly when never used, and q >= 7 otherwise
    s = wsum.cpu().numpy()
    assert np.array_equal(s == 0, wmax.cpu().numpy() == 0)
    assert (s[s > 0] >= 7).all()
    # the decoded floats score to the same bits; a second run and a side stream repeat them
    fs, fm = D.score(D.decode(stream, hdr, coord), n, deg, params, antialiased=aa)
    assert torch.equal(fs, wsum) and torch.equal(fm.view(torch.int32), wmax.view(torch.int32))
    s2, m2 = D.score_packed(stream, hdr, params)
    assert torch.equal(s2, wsum) and torch.equal(m2.view(torch.int32), wmax.view(torch.int32))
    side = torch.cuda.Stream(cuda)
    s3, m3 = D.score_packed(stream, hdr, params, stream=side)
    side.synchronize()
    assert torch.equal(s3, wsum) and torch.equal(m3.view(torch.int32), wmax.view(torch.int32))


def test_score_images_and_alpha_sums(cuda):
    import torch
    from spz_amd import device as D
    n, deg = 2500, 3
    _, (stream, hdr) = scene(cuda, n, deg, 17, False)
    floats = to_np(D.decode(stream, hdr, 4))
    params, _ = ring_views(floats["positions"], 4, 77, 59, (0.0, 1.0, 0.0), 4, seed=3)
    for p in params:
        p.background[0], p.background[1], p.background[2] = 0.25, 0.5, 0.75
    wsum, wmax, imgs = D.score_packed(stream, hdr, params, images=True)
    for j, p in enumerate(params):
        ref = D.render_packed(stream, hdr, p)
        assert torch.equal(imgs[j].view(torch.int32), ref.view(torch.int32)), f"view {j}: the image differs"
        one_s, _ = D.score_packed(stream, hdr, [p])
        alpha = float(ref[..., 3].double().sum().cpu())
        got = float(one_s.double().sum().cpu()) * Q
        assert alpha > 10.0
        assert abs(got - alpha) <= 1e-4 * alpha, (j, got, alpha)


def test_small_max_entries_sets_the_status_and_leaves_the_scores(cuda):
    import torch
    from spz_amd import device as D
    _, (stream, hdr) = scene(cuda, 1500, 0, 9, False)
    floats = to_np(D.decode(stream, hdr, 4))
    params, _ = ring_views(floats["positions"], 3, 64, 40, (0.0, 1.0, 0.0), 4)
    wsum, wmax, status = D.score_packed(stream, hdr, params, max_entries=10, return_status=True)
    assert status.cpu().tolist() == [1, 1, 1]
    assert not wsum.any() and not wmax.any()
    full, _, st = D.score_packed(stream, hdr, params, max_entries=1 << 22, return_status=True)
    assert st.cpu().tolist() == [0, 0, 0]
    assert torch.equal(full, D.score_packed(stream, hdr, params)[0])


def test_file_and_its_sorted_copy_score_permuted_identically(cuda, spz, tmp_path):
    from spz_amd import device as D
    c, (stream, hdr) = scene(cuda, 2000, 3, 21, False)
    raw = stream.cpu().numpy().tobytes()
    src, srt = tmp_path / "in.spz", tmp_path / "sorted.spz"
    src.write_bytes(gz(raw))
    order = spz.sort_spz(str(src), str(srt))
    floats = to_np(D.decode(stream, hdr, 4))
    views = []
    for v in spz.orbit_views(16, width=71, height=53, fov_y=25.0, scene=str(src), coord=spz.RUB, distance=6.0):
        # only views with distinct depths, where the sorted file blends in the same order
        rec = RR.preprocess(floats, 3, RR.camera(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"],
                                                  v["height"]))
        d = rec["depth"][rec["visible"]]
        if np.unique(d).size == d.size:
            views.append(v)
    assert len(views) >= 3
    ka, ma, sa, xa = spz.prune_spz(str(src), str(tmp_path / "a.spz"), views, keep_fraction=0.5, coord=spz.RUB,
                                   return_scores=True)
    kb, mb, sb, xb = spz.prune_spz(str(srt), str(tmp_path / "b.spz"), views, keep_fraction=0.5, coord=spz.RUB,
                                   return_scores=True)
    assert np.array_equal(sb, sa[order]) and np.array_equal(xb.view(np.uint32), xa[order].view(np.uint32))
    assert (sa > 0).mean() > 0.5


def test_output_equals_filter_with_the_mask(cuda, spz, tmp_path):
    c, (stream, hdr) = scene(cuda, 3000, 2, 5, True)
    n = 3000
    # a few points far outside every view, so some scores are zero
    src = tmp_path / "in.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    views = spz.orbit_views(4, width=60, height=45, fov_y=40.0, scene=str(src), coord=spz.RDF, distance=1.6)
    out, ref = str(tmp_path / "out.spz"), str(tmp_path / "ref.spz")
    _, _, s, x = spz.prune_spz(str(src), out, views, keep=n, coord=spz.RDF, return_scores=True)
    nz = int((s > 0).sum())
    assert 0 < nz < n
    rules = [dict(keep=0), dict(keep=n), dict(keep=17), dict(keep=nz + 50), dict(keep_fraction=0.33),
             dict(keep_fraction=1.0), dict(min_score=0.5), dict(min_score=1e-9), dict(min_score=-1.0)]
    for score in ("sum", "max"):
        for r in rules:
            if score == "max" and "min_score" in r:
                r = dict(min_score=r["min_score"] / 50.0)
            kept, mask, ws, wm = spz.prune_spz(str(src), out, views, score=score, coord=spz.RDF, return_scores=True, **r)
            assert np.array_equal(ws, s) and np.array_equal(wm.view(np.uint32), x.view(np.uint32))
            key = ws if score == "sum" else wm
            rule, value = next(iter(r.items()))
            if rule == "min_score" and score == "sum":
                want = ws.astype(np.float64) * Q >= value
            else:
                want = PR.keep_mask(key, rule, value)
            assert np.array_equal(mask, want), (score, r)
            assert kept == int(mask.sum())
            if rule == "keep" and value == nz + 50:  # every nonzero point, then the first 50 zero ones by index
                zeros = np.nonzero(s == 0)[0]
                assert mask[s > 0].all() and mask[zeros[:50]].all() and not mask[zeros[50:]].any()
            spz.filter_spz(str(src), ref, mask=mask)
            assert open(out, "rb").read() == open(ref, "rb").read(), (score, r)


def test_removing_the_zero_scores_keeps_the_views(cuda, spz, tmp_path):
    from spz_amd.synth import make_cloud_numpy
    n0, deg = 400, 1
    c = make_cloud_numpy(n0, deg, 12)
    c["positions"] = (c["positions"].reshape(-1, 3) * 0.4).astype(np.float32).reshape(-1)
    c["scales"] = (c["scales"] * 0.5 - 2.5).astype(np.float32)
    c["alphas"] = np.minimum(c["alphas"], -1.5).astype(np.float32)
    # outside every frustum, behind the near plane of the view from -z, and under 1/255 everywhere
    extra = make_cloud_numpy(60, deg, 13)
    p = extra["positions"].reshape(-1, 3)
    p[:20] = p[:20] * 0.1 + [60.0, 60.0, 0.0]
    p[20:40] = p[20:40] * 0.01 + [0.0, 0.0, -4.95]
    p[40:] = p[40:] * 0.3
    extra["positions"] = p.astype(np.float32).reshape(-1)
    a = extra["alphas"]
    a[40:] = -7.0
    extra["alphas"] = a.astype(np.float32)
    rng = np.random.default_rng(1)
    allc = {k: np.concatenate([c[k], extra[k]]) for k in c}
    perm = rng.permutation(n0 + 60)
    allc = {k: v.reshape(n0 + 60, -1)[perm].reshape(-1).astype(np.float32) for k, v in allc.items()}
    stream, hdr = encode(cuda, allc, n0 + 60, deg, False)
    src, out = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    views = []
    for eye in ([0.0, 0.0, -5.0], [0.5, 0.3, -4.0], [-0.4, -0.2, -4.5]):
        m = spz.look_at(eye, [0, 0, 0], [0, 1, 0])
        views.append(dict(world_to_camera=m, fx=60.0, fy=60.0, cx=40.0, cy=30.0, width=83, height=61))
    kept, mask, s, _ = spz.prune_spz(str(src), str(out), views, min_score=1e-9, coord=spz.RUB, return_scores=True)
    assert kept == int((s > 0).sum())
    gone = ~mask
    assert gone[np.argsort(perm)[n0:]].sum() >= 50, "the planted splats must score zero"
    for v in views:
        kw = dict(v, background=(0.1, 0.2, 0.3), coord=spz.RUB)
        a = spz.render_spz(str(src), **kw)
        b = spz.render_spz(str(out), **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_removing_splats_behind_walls_changes_only_saturated_pixels(cuda, spz, tmp_path):
    from spz_amd import device as D
    from spz_amd.synth import make_cloud_numpy
    deg = 0
    walls = make_cloud_numpy(4, deg, 2)
    walls["positions"] = np.float32([0, 0, 0, 0.05, 0.0, 0.5, -0.05, 0.0, 1.0, 0.0, 0.05, 1.5])
    walls["scales"] = np.float32([3.5, 3.5, -4.0] * 4)
    walls["rotations"] = np.float32([0, 0, 0, 1] * 4)
    walls["alphas"] = np.float32([9.0] * 4)
    behind = make_cloud_numpy(300, deg, 3)
    behind["positions"] = (behind["positions"].reshape(-1, 3) * 0.5 + [0, 0, 3]).astype(np.float32).reshape(-1)
    behind["scales"] = (behind["scales"] * 0.5 - 2.0).astype(np.float32)
    allc = {k: np.concatenate([walls[k], behind[k]]).astype(np.float32) for k in walls}
    n = 304
    stream, hdr = encode(cuda, allc, n, deg, False)
    src, out = tmp_path / "in.spz", tmp_path / "out.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    views = []
    for eye in ([0.0, 0.0, -4.0], [0.3, 0.2, -4.0]):
        m = spz.look_at(eye, [0, 0, 0], [0, 1, 0])
        views.append(dict(world_to_camera=m, fx=40.0, fy=40.0, cx=35.0, cy=25.0, width=69, height=53))
    kept, mask, s, _ = spz.prune_spz(str(src), str(out), views, min_score=1e-9, coord=spz.RUB, return_scores=True)
    assert kept < n and mask[:2].all()
    from spz_amd import abi
    bg = (0.1, 0.2, 0.3)
    rgb_max = 0.0
    for v in views:
        p = abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"],
                              coord=abi.RUB)
        rec = D.preprocess_packed(stream, hdr, p)
        vis = np.isfinite(rec["depth"].cpu().numpy())
        rgb_max = max(rgb_max, float(np.abs(rec["rgb"].cpu().numpy()[vis]).max()))
    # the Gaussian that ends a pixel (T (1 - a) < 1e-4) is not counted there; with a <= 0.99 the pixel's T is then
    # below 1e-4 / (1 - a) <= 0.01, and the Gaussians that take its place change it by at most T (|rgb| + |bg|)
    span = rgb_max + max(bg)
    for v in views:
        kw = dict(v, background=bg, coord=spz.RUB)
        a = spz.render_spz(str(src), **kw)
        b = spz.render_spz(str(out), **kw)
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=2)
        moved = diff > 0
        alpha = a[..., 3].astype(np.float64)
        assert (alpha[moved] >= 0.99 - 1e-6).all(), "a pixel that the walls did not end changed"
        assert (diff[moved] <= (1.0 - alpha[moved]) * span * 1.001 + 1e-6).all()
        assert (alpha >= 0.99 - 1e-6).mean() > 0.5, "the walls must cover the view"


@pytest.mark.parametrize("name", ["v1", "v2", "v3_sh3"])
def test_golden_streams_prune(cuda, spz, tmp_path, name):
    import torch
    from spz_amd import abi, device as D
    raw = golden_streams()[name]
    rc, h = abi.peek_header(raw)
    assert rc == 0
    stream = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(cuda)
    floats = to_np(D.decode(stream, h, abi.RUB))
    pos = floats["positions"].reshape(-1, 3)
    pos = pos[np.isfinite(pos).all(axis=1)]
    lo, hi = np.percentile(pos, 25, axis=0), np.percentile(pos, 75, axis=0)
    views = spz.orbit_views(3, width=67, height=45, fov_y=60.0, center=(0.5 * (lo + hi)).tolist(),
                            radius=float(np.linalg.norm(hi - lo)) * 0.5 + 1e-3)
    src, out, ref = tmp_path / "in.spz", tmp_path / "out.spz", tmp_path / "ref.spz"
    src.write_bytes(gz(raw))
    kept, mask, s, x = spz.prune_spz(str(src), str(out), views, keep_fraction=0.5, coord=spz.RUB, return_scores=True)
    assert kept == int(np.ceil(0.5 * h.num_points)) and (s > 0).any()
    spz.filter_spz(str(src), str(ref), mask=mask)
    assert out.read_bytes() == ref.read_bytes()
    params = [abi.render_params(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"],
                                coord=abi.RUB) for v in views]
    ws, wm = D.score_packed(stream, h, params)
    assert np.array_equal(ws.cpu().numpy().astype(np.uint64), s)
    cams = [RR.camera(v["world_to_camera"], v["fx"], v["fy"], v["cx"], v["cy"], v["width"], v["height"]) for v in views]
    want_sum, want_max = PR.scores(floats, h.sh_degree, cams, h.antialiased)
    if (want_sum > 0).sum() > 0.2 * s.size:
        check_scores(s, x, want_sum, want_max)


def test_cli_matches_prune_spz(cuda, spz, tmp_path):
    _, (stream, hdr) = scene(cuda, 2000, 1, 44, False)
    src = tmp_path / "in.spz"
    src.write_bytes(gz(stream.cpu().numpy().tobytes()))
    tool = os.path.join(ROOT, "spz_amd", "bin", "spz_prune")
    # --orbit, centre and radius from the file
    a, b = tmp_path / "a.spz", tmp_path / "b.spz"
    views = spz.orbit_views(6, width=64, height=40, fov_y=55.0, scene=str(src), coord=spz.RDF, distance=2.0)
    ka = spz.prune_spz(str(src), str(a), views, keep_fraction=0.4, coord=spz.RDF, score="max")
    r = subprocess.run([tool, str(src), str(b), "--orbit", "6", "--size", "64", "40", "--fov-y", "55", "--distance",
                        "2", "--keep-fraction", "0.4", "--coord", "RDF", "--score", "max"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == f"kept {ka}"
    assert a.read_bytes() == b.read_bytes()
    # --views
    vf = tmp_path / "views.txt"
    lines = ["# width height fx fy cx cy R|t"]
    for v in views[:4]:
        vals = [v["width"], v["height"], v["fx"], v["fy"], v["cx"], v["cy"]] + list(v["world_to_camera"].reshape(-1))
        lines.append(" ".join(repr(float(x)) if not isinstance(x, int) else str(x) for x in vals))
    vf.write_text("\n".join(lines) + "\n")
    parsed = spz.load_views_file(str(vf))
    kc = spz.prune_spz(str(src), str(a), parsed, keep=700)
    r = subprocess.run([tool, str(src), str(b), "--views", str(vf), "--keep", "700"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert kc == 700 and r.stdout.strip() == "kept 700"
    assert a.read_bytes() == b.read_bytes()
