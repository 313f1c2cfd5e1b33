"""k_fast_cells' two threshold paths against the CPU oracle.

A cell is scored at iniTh first and again at minTh only when nothing survives at iniTh (no corner, or
every corner ties with a neighbour in the 3x3 maximum test).  Each case is one small frame built so
that its cells take one path, the other, or both within one launch, in each of the kernel's three cell
bodies (52-byte window stride with a 40- or 48-byte score map, and the generic one).  Bar: bit-exact
candidates in cell order, per-cell thresholds, keypoints and descriptors.
"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_scores(img: np.ndarray) -> np.ndarray:
    """Threshold-free FAST-9 score of every pixel at least 3 px inside `img` (0 elsewhere): the largest
    t at which the pixel is a 9-arc corner, i.e. the best arc's smallest |difference| minus 1."""
    v = img.astype(np.int16)
    h, w = v.shape
    c = v[3:h - 3, 3:w - 3]
    d = np.stack([c - v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
    d = np.concatenate([d, d[:8]])
    best = np.full(c.shape, -1, np.int16)
    for a in range(16):
        arc = d[a:a + 9]
        best = np.maximum(best, np.maximum(arc.min(axis=0), -arc.max(axis=0)))
    out = np.zeros((h, w), np.int16)
    out[3:h - 3, 3:w - 3] = best - 1
    return out


def cell_windows(w: int, h: int):
    """Cell grid of a w x h level in the reference (src:1076-1129): cell size, columns and the FAST window
    (x, y, width, height) of each cell."""
    span_x, span_y = w - 32 + 6, h - 32 + 6
    ncols, nrows = span_x // 35, span_y // 35
    wc, hc = -(-span_x // ncols), -(-span_y // nrows)
    wins = []
    for i in range(nrows):
        y0 = 16 + i * hc
        if y0 >= h - 13 - 3:
            continue
        for j in range(ncols):
            x0 = 16 + j * wc
            if x0 >= w - 13 - 6:
                continue
            wins.append((x0, y0, min(x0 + wc + 6, w - 13) - x0, min(y0 + hc + 6, h - 13) - y0))
    return wc, hc, ncols, wins


def compress(img: np.ndarray) -> np.ndarray:
    """Contrast squeezed about mid-grey to 119..137: no FAST score reaches 20, steps of 8 and more stay."""
    return np.rint(128 + (img.astype(np.float32) - 128) * 0.07).astype(np.uint8)


def mirrored(synth, seed: int) -> np.ndarray:
    half = synth.polygon_frame(320, 480, seed=seed, n_shapes=60, noise_sigma=0.0)
    return np.ascontiguousarray(np.concatenate([half, half[:, ::-1]], axis=1))


MIRROR_SEED = 0


@pytest.fixture(scope="module")
def frames(synth):
    poly = synth.polygon_frame(640, 480, seed=41)
    mixed = poly.copy()
    mixed[:, 320:] = compress(poly)[:, 320:]
    mixed[200:290, :] = 128
    return {
        "poly": poly,
        "compressed": compress(poly),
        "mixed": mixed,
        "mirrored": mirrored(synth, MIRROR_SEED),
        "wide752": synth.polygon_frame(752, 480, seed=42),
        "odd333": synth.polygon_frame(333, 257, seed=43),
        "column104": synth.blurred_noise_frame(104, 110, seed=44),
    }


def _decode(keys: np.ndarray):
    keys = keys.astype(np.uint64)
    return np.stack([(keys >> 8) & 0xFFF, keys >> 20, keys & 0xFF], axis=1).astype(np.int64)


def _check(pkg, oracle, img, nf, nlevels, ini, mn):
    """Extractor against oracle: candidates and thresholds per level, status, keypoints, descriptors.
    Returns the oracle's per-level thresholds and candidate counts."""
    h, w = img.shape
    ex = pkg.ORBextractor(nf, 1.2, nlevels, ini, mn, max_width=w, max_height=h)
    ref = oracle.OracleExtractor(nf, 1.2, nlevels, ini, mn)
    kps, desc, mono = ex(img, None, (0, 1000))
    rkps, rdesc, rmono = ref(img, (0, 1000))
    thrs, ncand = [], []
    for l in range(nlevels):
        rc, rthr = ref.level_candidates(l), ref.level_cell_thresholds(l)
        buf = np.zeros(max(1, len(rc) + 64), np.uint32)
        thr = np.zeros(len(rthr) + 1, np.uint8)
        n = ex._lib.orb_debug_level_candidates(ex._h, 0, l, buf.ctypes.data, len(buf), thr.ctypes.data, len(thr))
        assert n == len(rc), f"level {l}: {n} candidates vs oracle {len(rc)}"
        exp = np.stack([rc["x"], rc["y"], rc["response"]], axis=1).astype(np.int64)
        assert np.array_equal(_decode(buf[:n]), exp), f"level {l} candidates"
        assert np.array_equal(thr[:len(rthr)].astype(np.int32), rthr), f"level {l} thresholds"
        thrs.append(rthr)
        ncand.append(len(rc))
    assert ex._lib.orb_debug_status(ex._h) == 0
    assert mono == rmono and len(kps) == len(rkps)
    assert np.array_equal(kps.view(np.uint8), rkps.view(np.uint8))
    assert np.array_equal(desc, rdesc)
    return thrs, ncand


def test_common_path(pkg, oracle, frames):
    """Textured 640x480 frame: nearly every cell emits at iniTh, the last cell column and row are narrower."""
    thrs, ncand = _check(pkg, oracle, frames["poly"], 1000, 8, 20, 7)
    assert np.mean(thrs[0] == 20) > 0.8 and min(ncand) > 0
    wc, hc, _, wins = cell_windows(640, 480)
    assert min(ww for _, _, ww, _ in wins) < wc + 6 and min(wh for _, _, _, wh in wins) < hc + 6


def test_every_cell_falls_back(pkg, oracle, frames):
    """Step heights between minTh and iniTh: no cell has a corner at iniTh, every cell is redone at minTh."""
    thrs, ncand = _check(pkg, oracle, frames["compressed"], 1000, 8, 20, 7)
    assert all((t == 7).all() for t in thrs) and min(ncand) > 0


def test_mixed_paths_and_empty_cells(pkg, oracle, frames):
    """Left half textured, right half compressed, a constant band across: both paths and empty cells in
    one launch."""
    thrs, ncand = _check(pkg, oracle, frames["mixed"], 1000, 8, 20, 7)
    assert 0.2 < np.mean(thrs[0] == 20) < 0.8
    _, _, ncols, wins = cell_windows(640, 480)
    sc = fast_scores(frames["mixed"])
    empty = [(sc[y + 3:y + wh - 3, x + 3:x + ww - 3] < 7).all() for x, y, ww, wh in wins]
    assert sum(empty) >= ncols


def test_corners_that_all_tie(pkg, oracle, frames):
    """Noise-free frame mirrored about the axis between columns 319 and 320: mirror-image neighbours tie
    in score and both lose the 3x3 maximum test, so some cell has corners at iniTh and still ends at minTh."""
    img = frames["mirrored"]
    thrs, _ = _check(pkg, oracle, img, 1000, 8, 20, 7)
    sc = fast_scores(img)
    _, _, _, wins = cell_windows(640, 480)
    assert len(wins) == len(thrs[0])
    tied = [(x, y, ww, wh) for (x, y, ww, wh), t in zip(wins, thrs[0])
            if t == 7 and (sc[y + 3:y + wh - 3, x + 3:x + ww - 3] >= 20).any()]
    assert tied
    # the numpy score is the oracle's response: one such pixel alone in a 7x7 window
    x, y, ww, wh = tied[0]
    py, px = np.argwhere(sc[y + 3:y + wh - 3, x + 3:x + ww - 3] >= 20)[0] + (y + 3, x + 3)
    kp = oracle.fast9(img[py - 3:py + 4, px - 3:px + 4], 20)
    assert len(kp) == 1 and int(kp["response"][0]) == sc[py, px]


@pytest.mark.parametrize("case,nf,nlevels,ini,mn,level,body", [
    ("wide752", 1200, 8, 20, 7, 0, "52/40"),
    ("odd333", 500, 8, 20, 7, 0, "52/48"),
    ("odd333", 500, 8, 12, 12, 0, "52/48"),
    ("column104", 200, 2, 20, 7, 1, "generic"),
    ("column104", 200, 2, 15, 15, 1, "generic"),
])
def test_other_cell_bodies(pkg, oracle, frames, case, nf, nlevels, ini, mn, level, body):
    """Windows wider than 44 px (48-byte score map rows) and windows that do not fit the 52-byte stride
    (generic body: the single 58 x 63 cell of the 104 x 110 frame's level 1); iniTh == minTh makes the
    two lists coincide."""
    img = frames[case]
    h, w = (int(np.rint(np.float32(n) / np.float32(1.2 ** level))) for n in img.shape)
    _, _, _, wins = cell_windows(w, h)
    ww, wh = max(c[2] for c in wins), max(c[3] for c in wins)
    assert body == ("generic" if ww > 52 or wh > 48 else "52/48" if ww > 44 else "52/40")
    thrs, ncand = _check(pkg, oracle, img, nf, nlevels, ini, mn)
    assert sum(ncand) > 0
