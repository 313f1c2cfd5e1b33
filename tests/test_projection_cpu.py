"""CPU checks of the SearchByProjection oracles against the independent pure-Python restatement
(tests/projection_ref.py) on random scenes, with some keypoints moved onto half cells of the grid."""
from __future__ import annotations

import numpy as np
import pytest

from projection_ref import grid_products, py_search, py_search_local

f32 = np.float32


def on_half_cells(cur):
    """Snap the first 60 keypoints' x and the next 60 keypoints' y onto half cells (the grid
    product is exactly k + 0.5, where C round and round-half-even part ways); they stay within reach of the
    points that project near them."""
    k = cur["keys_un"] = cur["keys_un"].copy()
    w, h = cur["width"] / 64.0, cur["height"] / 48.0
    k["x"][:60] = (np.floor(k["x"][:60] / w) + 0.5) * w
    k["y"][60:120] = (np.floor(k["y"][60:120] / h) + 0.5) * h
    return cur


def assert_half_cells(F):
    gx, gy = grid_products(F)
    assert ((gx[:60] % 1 == 0.5).sum() > 30) and ((gy[60:120] % 1 == 0.5).sum() > 30)


@pytest.mark.parametrize("th,mono,ori,stereo", [(7, False, True, True), (15, True, True, False), (7, False, False, True)])
def test_projection_oracle_matches_python(pkg, oracle, synth, th, mono, ori, stereo):
    cur, last = synth.tracking_pair(n_points=500, clutter=120, seed=41, stereo=stereo)
    C, L = pkg.Frame(**on_half_cells(cur)), pkg.Frame(**last)
    assert_half_cells(C)
    n, m = oracle.search_by_projection_frame(C, L, th, mono, ori)
    pn, pm = py_search(C, L, th, mono, ori)
    assert n == pn and np.array_equal(m, pm), f"{int((m != pm).sum())} differences"
    assert n > 100


@pytest.mark.parametrize("th,far", [(1, False), (3, False), (5, True)])
def test_local_projection_oracle_matches_python(pkg, oracle, synth, th, far):
    cur, _ = synth.tracking_pair(n_points=400, clutter=100, seed=43)
    P = pkg.LocalMapPoints(**synth.local_map_points(cur, n_points=500, seed=44))
    F = pkg.Frame(**on_half_cells(cur))
    assert_half_cells(F)
    taken = (np.random.default_rng(3).random(F.N) < 0.05).astype(np.uint8)
    n, m = oracle.search_by_projection_local(F, P, th, far, 10.0, 0.8, taken)
    pn, pm = py_search_local(F, P, th, far, 10.0, 0.8, taken)
    assert n == pn and np.array_equal(m, pm), f"{int((m != pm).sum())} differences"
    assert n > 50
