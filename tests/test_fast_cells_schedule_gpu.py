"""k_fast_cells' schedule edges against the CPU oracle.

Small frames built so that their cells hit the boundaries of the kernel's loops: the three cell bodies,
detectable heights and widths of every residue the compass rounds and partial octets see, iniTh lists
that end exactly at, one short of and one past a score round (64 lanes), octets that are completely full
beside empty ones, and cells that fall back to minTh beside cells that do not.  Each frame runs once
alone and once as frame 1 of a batch of three different frames on the same handle.  Bar (as in
test_fast_threshold_paths_gpu.py): candidates in cell order, per-cell thresholds for every cell,
keypoints and descriptors, all bit-exact.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_fast_threshold_paths_gpu import _decode, cell_windows, compress, fast_scores

pytestmark = pytest.mark.gpu

INI, MIN = 20, 7
STAMP_W, STAMP_H = 172, 137  # level 0: 4 x 3 cells of 35 px, windows 41 x 41 (35 in the last column and row)


def level_size(n: int, level: int) -> int:
    return int(np.rint(np.float32(n) / np.float32(1.2 ** level)))


def windows(w: int, h: int):
    """The reference's cell grid of a w x h level (src:1076-1129): columns and the FAST window (x, y, width,
    height) of every cell.  cell_windows of test_fast_threshold_paths_gpu.py spans 6 px more, which gives
    the same grid at that file's frame sizes but one more cell column or row at some of the sizes here."""
    span_x, span_y = w - 32, h - 32
    ncols, nrows = span_x // 35, span_y // 35
    wc, hc = -(-span_x // ncols), -(-span_y // nrows)
    wins = []
    for i in range(nrows):
        y0 = 16 + i * hc
        if y0 >= h - 16 - 3:
            continue
        for j in range(ncols):
            x0 = 16 + j * wc
            if x0 >= w - 16 - 6:
                continue
            wins.append((x0, y0, min(x0 + wc + 6, w - 16) - x0, min(y0 + hc + 6, h - 16) - y0))
    return ncols, wins


def compass_pass(img: np.ndarray, t: int) -> np.ndarray:
    """The kernel's pre-filter: two adjacent points of {up, right, down, left} at distance 3 both brighter
    than v + t or both darker than v - t.  False within 3 px of the border."""
    v = img.astype(np.int16)
    h, w = v.shape
    c = v[3:h - 3, 3:w - 3]
    up, down, left, right = v[0:h - 6, 3:w - 3], v[6:h, 3:w - 3], v[3:h - 3, 0:w - 6], v[3:h - 3, 6:w]
    bmax = np.minimum(np.maximum(up, down), np.maximum(left, right))
    dmin = np.maximum(np.minimum(up, down), np.minimum(left, right))
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = np.maximum(bmax - c, c - dmin) > t
    return out


def body_of(ww: int, wh: int) -> str:
    return "generic" if ww > 52 or wh > 48 else "52/48" if ww > 44 else "52/40"


def stamp_frame() -> np.ndarray:
    """Flat frame with single-pixel corners on the global lattice of multiples of 4: no circle or compass
    cross of another pixel holds two of them, so a cell's iniTh list is exactly its stamps, each a corner
    of score d - 1 and a 3x3 maximum.  Texture blocks stay 4 px inside their own cell."""
    img = np.full((STAMP_H, STAMP_W), 128, np.uint8)
    ncols, wins = windows(STAMP_W, STAMP_H)

    def det(i, j):
        x, y, ww, wh = wins[i * ncols + j]
        return x + 3, y + 3, x + ww - 3, y + wh - 3

    def stamp(i, j, k, d):
        x0, y0, x1, y1 = det(i, j)
        pts = [(y, x) for y in range(y0, y1) if y % 4 == 0 for x in range(x0, x1) if x % 4 == 0]
        assert len(pts) >= k
        for y, x in pts[:k]:
            img[y, x] = 128 + d

    stamp(0, 0, 63, 60)
    stamp(0, 1, 64, 60)
    stamp(1, 0, 65, 60)
    stamp(2, 1, 1, 60)
    stamp(0, 3, 1, 60)
    x0, y0, x1, y1 = det(0, 2)  # dense texture: far more than two score rounds
    img[y0 + 4:y1 - 4, x0 + 4:x1 - 4] = np.random.default_rng(7).integers(0, 256, (y1 - y0 - 8, x1 - x0 - 8))
    x0, y0, x1, y1 = det(1, 2)  # octets 1 and 3 full over 12 rows, octets 0, 2 and 4 empty
    for o in (1, 3):
        ys, xs = np.arange(y0 + 6, y0 + 18), np.arange(x0 + 8 * o, x0 + 8 * o + 8)
        img[ys[:, None], xs[None, :]] = 88 + 80 * ((ys[:, None] // 3 + xs[None, :] // 3) & 1)
    stamp(2, 0, 5, 12)   # score 11: nothing at iniTh, redone at minTh
    stamp(1, 1, 70, 12)  # the same with a minTh list of two score rounds
    stamp(2, 3, 2, 12)
    return img  # cells (2, 2) and (1, 3) stay flat: empty at both thresholds


def _mixed(a: np.ndarray) -> np.ndarray:
    out = a.copy()
    out[:, a.shape[1] // 2:] = compress(a)[:, a.shape[1] // 2:]
    return out


@pytest.fixture(scope="module")
def sets(synth):
    """name -> (nlevels, three frames of one size).  Eight levels need 240 px a side (the last level must
    still hold one cell), so the small frames run with fewer.  The two long frames are what it takes to
    get a window narrower than an octet (dw 7 at width 873) or shorter than three rows (dh 2 at height
    1048; the quad-tree's initial node count, round(width / height), must stay between 1 and 8,
    hence 560 and 140 px the other way)."""
    def trio(w, h, s):
        p = synth.polygon_frame(w, h, seed=s, n_shapes=max(20, w * h // 400))
        return [p, synth.blurred_noise_frame(w, h, seed=s + 1), _mixed(synth.polygon_frame(w, h, seed=s + 2, n_shapes=max(20, w * h // 400)))]
    return {
        "stamps": (4, [stamp_frame(), synth.polygon_frame(STAMP_W, STAMP_H, seed=61, n_shapes=50),
                       _mixed(synth.polygon_frame(STAMP_W, STAMP_H, seed=62, n_shapes=50))]),
        "small111": (3, trio(111, 96, 70)),
        "wide873": (1, trio(873, 140, 80)),
        "tall1048": (1, trio(560, 1048, 90)),
    }


@pytest.fixture(scope="module")
def expected(oracle, sets):
    """The oracle's results per (set, frame), computed once."""
    out = {}
    for name, (nl, frames) in sets.items():
        ref = oracle.OracleExtractor(500, 1.2, nl, INI, MIN)
        for i, img in enumerate(frames):
            kps, desc, mono = ref(img, (0, 1000))
            out[name, i] = (kps, desc, mono, [(ref.level_candidates(l), ref.level_cell_thresholds(l)) for l in range(nl)])
    return out


def _level_windows(img, nl):
    h, w = img.shape
    return [windows(level_size(w, l), level_size(h, l))[1] for l in range(nl)]


def test_frames_cover_the_schedule(sets, expected):
    """CPU side: the frames hit every body, residue, list size, octet fill and threshold path the kernel's
    loops distinguish."""
    seen = set()
    for name, (nl, frames) in sets.items():
        for wins in _level_windows(frames[0], nl):
            for _, _, ww, wh in wins:
                dw, dh = ww - 6, wh - 6
                seen |= {("body", body_of(ww, wh)), ("dh", dh % 3 if dh >= 3 else "<3"), ("dw", dw % 8 if dw >= 8 else "<8")}
    assert windows(640, 480)[1] != [] and len(windows(640, 480)[1]) == len(cell_windows(640, 480)[3])
    need = {("body", b) for b in ("52/40", "52/48", "generic")} | {("dh", r) for r in (0, 1, 2, "<3")} | \
           {("dw", r) for r in (0, 1, 4, 7, "<8")}
    assert need <= seen, need - seen

    img = sets["stamps"][1][0]
    ncols, wins = windows(STAMP_W, STAMP_H)
    ini_pass, sc = compass_pass(img, INI), fast_scores(img)
    nlist = [int(ini_pass[y + 3:y + wh - 3, x + 3:x + ww - 3].sum()) for x, y, ww, wh in wins]
    ncorner = [int((sc[y + 3:y + wh - 3, x + 3:x + ww - 3] >= INI).sum()) for x, y, ww, wh in wins]
    cell = lambda i, j: i * ncols + j
    for (i, j), n in {(0, 0): 63, (0, 1): 64, (1, 0): 65, (2, 1): 1, (0, 3): 1, (2, 2): 0, (2, 0): 0, (1, 1): 0}.items():
        assert nlist[cell(i, j)] == n and ncorner[cell(i, j)] == n, (i, j, nlist[cell(i, j)], ncorner[cell(i, j)])
    assert nlist[cell(0, 2)] > 128
    min_pass = compass_pass(img, MIN)
    x, y, ww, wh = wins[cell(1, 1)]
    assert int(min_pass[y + 3:y + wh - 3, x + 3:x + ww - 3].sum()) == 70  # the rebuilt list, two rounds
    # full octets beside empty ones
    x, y, ww, wh = wins[cell(1, 2)]
    rows = ini_pass[y + 3:y + wh - 3, x + 3:x + ww - 3][6:18]
    octs = [rows[:, 8 * o:8 * o + 8] for o in range(5)]
    assert octs[1].all() and octs[3].all() and not (octs[0].any() or octs[2].any() or octs[4].any())
    # both threshold paths within the level-0 launch, and every cell reported
    thr = expected["stamps", 0][3][0][1]
    assert len(thr) == len(wins) and thr[cell(0, 0)] == INI and thr[cell(0, 2)] == INI
    assert thr[cell(2, 0)] == MIN and thr[cell(1, 1)] == MIN and thr[cell(2, 2)] == MIN and thr[cell(2, 1)] == INI
    for name in ("small111", "wide873", "tall1048"):
        t0 = expected[name, 2][3][0][1]
        assert (t0 == INI).any() and (t0 == MIN).any(), name


def _check_levels(ex, frame, exp, img, nl):
    for l, ((rc, rthr), wins) in enumerate(zip(exp[3], _level_windows(img, nl))):
        assert len(rthr) == len(wins)  # one threshold per cell: no cell is left out
        buf = np.zeros(max(1, len(rc) + 64), np.uint32)
        thr = np.zeros(len(rthr) + 1, np.uint8)
        n = ex._lib.orb_debug_level_candidates(ex._h, frame, l, buf.ctypes.data, len(buf), thr.ctypes.data, len(thr))
        assert n == len(rc), f"level {l}: {n} candidates vs oracle {len(rc)}"
        want = np.stack([rc["x"], rc["y"], rc["response"]], axis=1).astype(np.int64)
        assert np.array_equal(_decode(buf[:n]), want), f"level {l} candidates"
        assert np.array_equal(thr[:len(rthr)].astype(np.int32), rthr), f"level {l} thresholds"
    assert ex._lib.orb_debug_status(ex._h) == 0


@pytest.mark.parametrize("name", ["stamps", "small111", "wide873", "tall1048"])
def test_alone_and_inside_a_batch(pkg, sets, expected, name):
    import torch
    nl, frames = sets[name]
    h, w = frames[0].shape
    ex = pkg.ORBextractor(500, 1.2, nl, INI, MIN, max_width=w, max_height=h, max_batch=3)
    for i, img in enumerate(frames):
        exp = expected[name, i]
        # as frame 1 of a batch whose frames 0 and 2 are the two other frames
        order = [(i + 2) % 3, i, (i + 1) % 3]
        imgs = torch.from_numpy(np.stack([frames[k] for k in order])).cuda()
        kps, desc, counts = ex.extract_batch_device(imgs, (0, 1000))
        torch.cuda.synchronize()
        _check_levels(ex, 1, exp, img, nl)
        n = int(counts[1, 0])
        assert n == len(exp[0]) and int(counts[1, 1]) == exp[2]
        assert np.array_equal(pkg.keypoints_to_structured(kps[1], n).view(np.uint8), exp[0].view(np.uint8))
        assert np.array_equal(desc[1, :n].cpu().numpy(), exp[1])
        # alone, on the handle that has just run the batch
        k1, d1, mono = ex(img, None, (0, 1000))
        _check_levels(ex, 0, exp, img, nl)
        assert mono == exp[2] and len(k1) == len(exp[0])
        assert np.array_equal(k1.view(np.uint8), exp[0].view(np.uint8))
        assert len(k1) == 0 or np.array_equal(d1, exp[1])
