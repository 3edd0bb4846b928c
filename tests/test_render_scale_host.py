"""The scene builders of tests/test_gpu_render_scale.py without a GPU: each builder asserts, from the float64
reference alone, what takes its scene down the path it is for (the tile and digit counts, the run count, the list
lengths and last used positions, the stopped bands, the row count); here they run on the CPU, so that an edit that
turns a scene back into a small case fails before any device sees it."""
import numpy as np
import pytest

import test_gpu_render_scale as S


@pytest.mark.parametrize("name", list(S.SORT_VIEWS))
def test_sort_views_reach_their_digit_counts(name):
    s = S.sort_view(name)
    assert s["tiles"] == {"256_tiles": 256, "289_tiles": 289, "65536_tiles": 65536, "66049_tiles": 66049}[name]
    assert s["entries"] == sum(len(v) for v in s["lists"].values()) > s["n"]


def test_the_289_tile_view_has_no_marginal_pair():
    assert S.gradient_reference("sort", "289_tiles")["dec"]["marginal"] == 0


def test_scan_scene_has_more_than_256_runs_and_lists_of_many_batches():
    s = S.scan_scene()
    assert s["runs"] > 256 and s["lengths"].min() > 3 * S.BATCH and s["share"] <= 0.01
    assert np.isfinite(s["image"]).all() and s["image"][..., 3].max() < 0.5


@pytest.mark.parametrize("name", list(S.DEEP_CASES))
def test_deep_scenes_reach_their_batches_and_exits(name):
    s = S.deep_scene(name)
    assert s["dec"]["marginal"] == 0 and max(f["length"] for f in s["facts"]) > 3 * S.BATCH


def test_reduce_scene_has_157_rows():
    s = S.reduce_scene()
    assert (s["n"] + S.VIEW_ROWS - 1) // S.VIEW_ROWS == 157 and (s["mag"] > 0).all()
