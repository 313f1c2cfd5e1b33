"""Hand-built ComputeStereoMatches scenes (reference src/Frame.cc:1102-1358): keypoints and descriptors
written by hand on textured-noise images, one function per group.  Each returns a `Group` whose first
nine fields are (left_image, right_image, kps_l, desc_l, kps_r, desc_r, bf, b, expected_reasons);
`expected_reasons[i]` is the stereo_ref reason code prescribed for left keypoint i.  The cull group runs
its populations as separate calls (`subsets`: name -> left indices); the batch group holds B frames
(images [B, H, W], per-frame keypoint lists).

How a scene fixes the outcome of the SAD search without knowing the pyramid's pixels:
  * the right image is the left one plus +-1 noise ("zero shift"), except in rectangles where it is the
    left image moved by D pixels.  D is chosen so that D / 1.2^octave is an integer to 0.02 px, so the
    level plane of that octave is moved by d = round(D / scale) level pixels there.
  * a left keypoint at level position cuL and a right one at cuR then have their SAD minimum at the
    offset cuL - d - cuR.
  * in a zero-shift area uL = (cuL + 0.4) * scale makes the disparity (0.4 - deltaR) * scale > 0.
  * at level 0 (the input image itself) ties and exact SADs are painted into the pixels.
test_stereo_cases_cpu.py checks every prescription against stereo_ref and the oracle."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import conftest

conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402

f32 = np.float32
NLEVELS, BF, B = 8, 8.0, 0.110074          # maxD = bf / b = 72.68 px fits the frame
EDGE, CELL = 19, 35

# ORBextractor's scale tables (src/ORBextractor.cc:474-495): float products of a double factor
SCALE = [f32(1)]
for _ in range(1, NLEVELS):
    SCALE.append(f32(float(SCALE[-1]) * float(f32(1.2))))
INV_SCALE = [f32(1) / s for s in SCALE]
MAX_D = f32(f32(BF) / f32(B))


def level_size(n, level):
    return int(np.rint(f32(f32(n) * INV_SCALE[level])))  # cvRound(float), src/ORBextractor.cc:1692


def geometry_accepts(w, h):
    """build_geometry's acceptance (csrc/orb_extract_geom.h) for 1.2 / 8 levels: every level holds the
    19-px frame and at least one 35-px FAST cell each way, and 1 to 8 quad-tree roots."""
    for l in range(NLEVELS):
        lw, lh = level_size(w, l), level_size(h, l)
        if lw < 2 * EDGE or lh < 2 * EDGE:
            return False
        wid, hei = f32(lw - 32), f32(lh - 32)
        ncols, nrows = int(wid / f32(CELL)), int(hei / f32(CELL))
        if ncols <= 0 or nrows <= 0:
            return False
        wcell, hcell = int(np.ceil(wid / f32(ncols))), int(np.ceil(hei / f32(nrows)))
        if wcell + 6 >= 128 or hcell + 6 >= 512 or (wcell + 7) // 8 * hcell > 1024:
            return False
        roots = int(np.floor(abs(float(f32(lw - 32) / f32(lh - 32))) + 0.5))
        if roots <= 0 or roots > 8:
            return False
    return True


def smallest_frame():
    """The smallest square frame build_geometry accepts."""
    n = 2 * EDGE
    while not geometry_accepts(n, n):
        n += 1
    return n


S = smallest_frame()   # frame width and height
LW = [level_size(S, l) for l in range(NLEVELS)]


class Group(NamedTuple):
    left_image: np.ndarray
    right_image: np.ndarray
    kps_l: object
    desc_l: object
    kps_r: object
    desc_r: object
    bf: float
    b: float
    expected_reasons: object
    names: object = None        # case name per left keypoint
    expected_idx: object = None  # {left index: right index the Hamming search must choose}
    expected_offset: object = None  # {left index: winning SAD offset}
    ties: object = None         # {left index: right indices / offsets that must tie}
    subsets: object = None      # cull: {population: left indices}
    expected_sad: object = None  # cull: {left index: SAD}
    counts: object = None       # batch: (counts_l, counts_r, cap_l, cap_r)


def lvl_x(level, c, frac=0.0):
    """A float coordinate whose scaled, rounded level position is c (checked)."""
    x = f32((c + frac) * float(SCALE[level]))
    got = np.floor(abs(float(f32(x * INV_SCALE[level]))) + 0.5)
    assert got == c, (level, c, frac, got)
    return x


def half_x(level, c):
    """A float x with x * inv_scale == c + 0.5 exactly in float (std::round gives c + 1, rint gives c for even c)."""
    x = f32((c + 0.5) * float(SCALE[level]))
    for cand in [x] + [f(x, k) for k in range(1, 64) for f in (_up, _down)]:
        if f32(cand * INV_SCALE[level]) == f32(c + 0.5):
            return cand
    return None


def _up(x, k):
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


def _down(x, k):
    for _ in range(k):
        x = np.nextafter(x, f32(-np.inf))
    return x


class Scene:
    def __init__(self, seed, noise=1, smooth=False):
        self.rng = np.random.default_rng(seed)
        self.L = self.rng.integers(2, 254, (S, S)).astype(np.uint8)
        if smooth:
            # a 5x5 box filter, stretched back to the full range: gentler gradients, so that the 0.02 px by
            # which a moved rectangle misses a whole level pixel adds little to the SAD
            a = np.pad(self.L.astype(np.float64), 2, mode="reflect")
            a = sum(a[dy:dy + S, dx:dx + S] for dy in range(5) for dx in range(5)) / 25.0
            a = (a - a.min()) / (a.max() - a.min())
            self.L = (2 + np.rint(a * 251)).astype(np.uint8)
        self.noise = self.rng.integers(-noise, noise + 1, (S, S)) if noise else np.zeros((S, S), np.int64)
        self.R = (self.L.astype(np.int64) + self.noise).astype(np.uint8)
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.fixed_r = {}
        self.reasons, self.names, self.idx, self.offs, self.ties = [], [], {}, {}, {}

    def shift(self, r0, r1, c0, c1, D):
        """right[r0:r1, c0:c1] = left moved D px to the left (a point at x appears at x - D), plus the noise."""
        assert 0 <= c0 and c1 + D <= S
        self.R[r0:r1, c0:c1] = (self.L[r0:r1, c0 + D:c1 + D].astype(np.int64) + self.noise[r0:r1, c0:c1]).astype(np.uint8)

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    @staticmethod
    def flip(d, n, start=0):
        """d with bits start .. start+n-1 flipped: Hamming distance n from d."""
        bits = np.unpackbits(d)
        bits[start:start + n] ^= 1
        return np.packbits(bits)

    def left(self, name, x, y, octave, d, reason, idx=None, off=None):
        self.kl.append((x, y, octave))
        self.dl.append(d)
        self.reasons.append(reason)
        self.names.append(name)
        i = len(self.kl) - 1
        if idx is not None:
            self.idx[i] = idx
        if off is not None:
            self.offs[i] = off
        return i

    def right(self, x, y, octave, d, at=None):
        """Add a right keypoint; `at` pins its index (the others fill the free indices in order)."""
        if at is not None:
            assert at not in self.fixed_r
            self.fixed_r[at] = (x, y, octave, d)
            return at
        self.kr.append((x, y, octave, d))
        return ("free", len(self.kr) - 1)

    def build(self, n_r=None):
        total = max([len(self.kr) + len(self.fixed_r)] + [k + 1 for k in self.fixed_r])
        n_r = total if n_r is None else n_r
        assert n_r >= total, (n_r, total)
        order, free, remap = [], iter(self.kr), {}
        k = 0
        for i in range(n_r):
            if i in self.fixed_r:
                order.append(self.fixed_r[i])
                continue
            nxt = next(free, None)
            if nxt is None:  # filler: a far descriptor on the bottom row, away from every case
                nxt = (f32(3.0), f32(S - 1), 0, self.desc())
            else:
                remap[("free", k)] = i
                k += 1
            order.append(nxt)
        for dct in (self.idx,):
            for key, v in list(dct.items()):
                dct[key] = remap.get(v, v)
        for key, v in list(self.ties.items()):
            if v and isinstance(v[0], tuple):
                self.ties[key] = [remap[t] for t in v]
        kl = np.zeros(len(self.kl), KEYPOINT_DTYPE)
        for i, (x, y, o) in enumerate(self.kl):
            kl[i]["x"], kl[i]["y"], kl[i]["octave"], kl[i]["size"], kl[i]["angle"] = x, y, o, 31.0, 0.0
        kr = np.zeros(n_r, KEYPOINT_DTYPE)
        for i, (x, y, o, _) in enumerate(order):
            kr[i]["x"], kr[i]["y"], kr[i]["octave"], kr[i]["size"], kr[i]["angle"] = x, y, o, 31.0, 0.0
        dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        dr = np.array([o[3] for o in order], np.uint8).reshape(-1, 32)
        return Group(self.L, self.R, kl, dl, kr, dr, BF, B, list(self.reasons), list(self.names), dict(self.idx),
                     dict(self.offs), dict(self.ties))


# ---------------------------------------------------------------------------------------- hamming
def hamming():
    sc = Scene(11)
    D0 = 20
    sc.shift(0, 80, 0, S - D0, D0)       # rows 0..79: disparity 20
    sc.shift(125, 156, 0, S - 72, 72)    # rows 125..155: disparity 72, for the minU edge
    # rows 80..124 stay zero-shift

    def true_pair(name, ul, vl, dist, reason="matched", at=None, start=0):
        d = sc.desc()
        r = sc.right(f32(ul - D0), f32(vl), 0, sc.flip(d, dist, start), at=at)
        return sc.left(name, f32(ul), f32(vl), 0, d, reason, idx=r if dist < 100 else None), d

    # equal best distance: the lower right index wins (first strict minimum, :1212)
    d = sc.desc()
    sc.right(f32(100 - D0), f32(12), 0, sc.flip(d, 20, 0), at=5)
    sc.right(f32(100 - D0 - 30), f32(12), 0, sc.flip(d, 20, 100), at=9)
    i = sc.left("tie_same_chunk", f32(100), f32(12), 0, d, "matched", idx=5)
    sc.ties[i] = [5, 9]
    d = sc.desc()
    sc.right(f32(100 - D0), f32(26), 0, sc.flip(d, 20, 0), at=3)
    sc.right(f32(100 - D0 - 30), f32(26), 0, sc.flip(d, 20, 100), at=70)
    i = sc.left("tie_across_chunks", f32(100), f32(26), 0, d, "matched", idx=3)
    sc.ties[i] = [3, 70]
    # threshold: (TH_HIGH + TH_LOW) / 2 = 75 rejects, 74 passes
    true_pair("dist_74", 60, 40, 74)
    true_pair("dist_75", 120, 40, 75, "hamming_ge_75")
    true_pair("dist_100", 180, 40, 100, "hamming_ge_75")
    # row band of an octave-0 keypoint at y = 50.0: [48, 52]
    d = sc.desc()
    r = sc.right(f32(150 - D0), f32(50.0), 0, sc.flip(d, 10))
    for vl, reason in ((47.9, "no_row_candidates"), (48.0, "matched"), (52.99, "matched"), (53.0, "no_row_candidates")):
        sc.left(f"band0_row_{vl}", f32(150), f32(vl), 0, d, reason, idx=r if reason == "matched" else None)
    # a closer descriptor one row outside its band, a farther one inside
    d = sc.desc()
    sc.right(f32(60 - D0 - 30), f32(62.0), 0, sc.flip(d, 10, 100))      # band [60, 64]: row 65 is outside
    r = sc.right(f32(60 - D0), f32(65.0), 0, sc.flip(d, 30))
    sc.left("gate_row", f32(60), f32(65.0), 0, d, "matched", idx=r)
    # octave gate: levelL + 2 fails, levelL + 1 passes
    d = sc.desc()
    sc.right(f32(200 - D0 - 30), f32(65.0), 2, sc.flip(d, 10, 100))
    r = sc.right(f32(200 - D0), f32(65.0), 1, sc.flip(d, 30))
    sc.left("gate_octave_plus2", f32(200), f32(65.0), 0, d, "matched", idx=r)
    # octave gate: levelL - 2 fails, levelL - 1 passes (left at octave 2, zero-shift rows, min at +2)
    d = sc.desc()
    cu, cv = 40, 70
    sc.right(lvl_x(2, cu - 4), lvl_x(2, cv), 0, sc.flip(d, 10, 100))
    r = sc.right(lvl_x(2, cu - 2), lvl_x(2, cv), 1, sc.flip(d, 30))
    sc.left("gate_octave_minus2", lvl_x(2, cu, 0.4), lvl_x(2, cv), 2, d, "matched", idx=r, off=2)
    # row band of an octave-2 keypoint at a fractional y: r = 2.88, [floor(97.42), ceil(103.18)] = [97, 104]
    d = sc.desc()
    cu = 130
    r = sc.right(lvl_x(1, cu - 2), f32(100.3), 2, sc.flip(d, 10))
    for vl, reason in ((96.9, "no_row_candidates"), (97.0, "matched"), (104.9, "matched"), (105.0, "no_row_candidates")):
        sc.left(f"band2_row_{vl}", lvl_x(1, cu, 0.4), f32(vl), 1, d, reason, idx=r if reason == "matched" else None)
    # uR == maxU passes (zero-shift rows, level 0); the next float above fails
    d = sc.desc()
    ul = f32(200.4)
    r = sc.right(ul, f32(115), 0, sc.flip(d, 10))
    sc.left("uR_eq_maxU", ul, f32(115), 0, d, "matched", idx=r, off=0)
    d = sc.desc()
    ul = f32(30.4)
    sc.right(np.nextafter(ul, f32(np.inf)), f32(115), 0, sc.flip(d, 10, 100))
    r = sc.right(f32(28.0), f32(115), 0, sc.flip(d, 30))
    sc.left("uR_above_maxU", ul, f32(115), 0, d, "matched", idx=r, off=2)
    # uR == minU passes; the next float below fails.  uL = cu + 0.2: minU = cu - 72.48 rounds to cu - 72,
    # the disparity-72 rows put the SAD minimum at offset 0 and the disparity 72.2 - deltaR is below maxD.
    d = sc.desc()
    ul = f32(150.2)
    min_u = f32(ul - MAX_D)
    r = sc.right(min_u, f32(140), 0, sc.flip(d, 10))
    sc.left("uR_eq_minU", ul, f32(140), 0, d, "matched", idx=r, off=0)
    d = sc.desc()
    ul = f32(200.2)
    min_u = f32(ul - MAX_D)
    sc.right(np.nextafter(min_u, f32(-np.inf)), f32(140), 0, sc.flip(d, 10, 100))
    r = sc.right(f32(min_u + f32(0.25)), f32(140), 0, sc.flip(d, 30))
    sc.left("uR_below_minU", ul, f32(140), 0, d, "matched", idx=r, off=0)
    # a left keypoint on row h: (size_t)vL >= nRows
    d = sc.desc()
    sc.right(f32(100), f32(S - 1), 0, sc.flip(d, 10))
    sc.left("y_eq_h", f32(120), f32(S), 0, d, "no_row_candidates")
    return sc.build(n_r=130)


# ----------------------------------------------------------------------------------------- window
# (octave, D, rows, right columns, cv of the cases) of the moved rectangles of the window group
WINDOW_BANDS = {0: (20, (45, 120), (0, S - 20), 60), 7: (68, (122, 197), (0, 150), 44),
                3: (52, (198, S), (0, 100), 126), 1: (24, (198, S), (120, 215), 182)}


def window():
    sc = Scene(12, noise=5, smooth=True)   # +-5: the median SAD stays above half of the moved rectangles' SADs
    for o, (D, (r0, r1), (c0, c1), _) in WINDOW_BANDS.items():
        sc.shift(r0, r1, c0, c1, D)
    for o in (0, 1, 3, 7):
        lw = lh = LW[o]
        D, _, _, cvb = WINDOW_BANDS[o]
        d_o = int(round(D / float(SCALE[o])))

        def pair(name, cul, cvl, cur, reason, off=None, frac=0.4):
            d = sc.desc()
            r = sc.right(lvl_x(o, cur), lvl_x(o, cvl), o, sc.flip(d, 10))
            return sc.left(f"o{o}_{name}", lvl_x(o, cul, frac), lvl_x(o, cvl), o, d, reason, idx=r, off=off)

        # zero-shift area (top rows): the minimum is at cuL - cuR
        pair("right_edge_reject", lw - 9, 20, lw - 11, "window_right_edge")        # scaleduR0 + 11 == lw
        pair("right_edge_accept", lw - 10, 5, lw - 12, "matched", off=2)           # == lw - 1; cvL == 5
        pair("cuR_9", 11, 20, 9, "window_view_bound")
        pair("cuR_10", 12, 5, 10, "matched", off=2)
        pair("cvL_4", 30, 4, 28, "window_view_bound")
        pair("cvL_lh-5", 30, lh - 5, 28, "window_view_bound")
        pair("cuL_4", 4, 20, 3, "window_view_bound")
        pair("cuL_lw-5", lw - 5, 20, lw - 12, "window_view_bound")
        pair("min_plus4", 34, 5, 30, "matched", off=4)
        pair("min_plus5", 45, 5, 40, "best_at_plus_L", off=None)
        for k in range(4):   # left patch start addresses of every residue mod 4
            pair(f"residue_{k}", 20 + k, 5, 18 + k, "matched", off=2)
        # moved rectangle: the minimum is at cuL - d - cuR
        base = {0: 150, 7: 38, 3: 44, 1: 172}[o]
        pair("min_minus4", base, cvb, base - d_o + 4, "matched", off=-4, frac=0.0)
        pair("min_minus5", base + 2, cvb, base + 2 - d_o + 5, "best_at_minus_L", frac=0.0)
        # x * inv_scale == c + .5 exactly: std::round goes away from zero (c + 1), on both sides
        c = base + 4 if (base + 4) % 2 == 0 else base + 5
        xl, xr = half_x(o, c), half_x(o, c - d_o)
        if o == 0 or (xl is not None and xr is not None):
            d = sc.desc()
            r = sc.right(xr, lvl_x(o, cvb), o, sc.flip(d, 10))
            sc.left(f"o{o}_round_half", xl, lvl_x(o, cvb), o, d, "matched", idx=r, off=0)
    # level 0, painted: equal SAD minima from a texture of period 3 -- the first offset wins
    for k, (name, ncols, cul) in enumerate((("tie2", 14, 60), ("tie3", 17, 110))):
        cv, cur = 90, cul - 20
        tile = sc.rng.integers(2, 254, (11, 3)).astype(np.uint8)
        strip = np.tile(tile, (1, 9))
        sc.L[cv - 5:cv + 6, cul - 5:cul + 6] = strip[:, :11]
        c0 = cur - 4 - 5                      # offsets -4, -1 (, +2) see the texture in phase
        sc.R[cv - 5:cv + 6, c0:c0 + ncols] = strip[:, :ncols]
        d = sc.desc()
        r = sc.right(f32(cur), f32(cv), 0, sc.flip(d, 10))
        i = sc.left(f"o0_{name}", f32(cul), f32(cv), 0, d, "matched", idx=r, off=-4)
        sc.ties[i] = [-4, -1] if ncols == 14 else [-4, -1, 2]
    g = sc.build()
    # the unaligned row loads: patch start addresses (plane rows are 128-byte aligned, the view starts at
    # byte 19) cover all four residues mod 4 on the left and, independently, on the right
    res_l, res_r = set(), set()
    for i, reason in enumerate(g.expected_reasons):
        if reason in ("matched", "best_at_plus_L", "best_at_minus_L"):
            o = int(g.kps_l[i]["octave"])
            cul = int(np.floor(float(f32(g.kps_l[i]["x"] * INV_SCALE[o])) + 0.5))
            cur = int(np.floor(float(f32(g.kps_r[g.expected_idx[i]]["x"] * INV_SCALE[o])) + 0.5))
            res_l.add((o, (EDGE + cul - 5) & 3))
            res_r.update((o, (EDGE + cur + inc - 5) & 3) for inc in range(-5, 6))
    for o in (0, 1, 3, 7):
        assert {r for (oo, r) in res_l if oo == o} == {0, 1, 2, 3}, (o, sorted(res_l))
        assert {r for (oo, r) in res_r if oo == o} == {0, 1, 2, 3}, (o, sorted(res_r))
    return g


# -------------------------------------------------------------------------------------- disparity
def disparity():
    sc = Scene(13)
    sc.shift(60, 120, 0, S - 72, 72)
    sc.shift(120, 180, 0, S - 73, 73)

    def pair(name, ul, vl, ur, reason, off):
        d = sc.desc()
        r = sc.right(f32(ur), f32(vl), 0, sc.flip(d, 10))
        return sc.left(name, f32(ul), f32(vl), 0, d, reason, idx=r, off=off)

    # zero-shift rows, exact copy (no noise) around the keypoint: SAD 0 at offset 0, equal neighbours are not
    # needed -- deltaR = (d1 - d3) / (2 (d1 + d3)); paint a mirror-symmetric texture so that d1 == d3, deltaR = 0
    for name, ul, reason in (("exactly_zero", 100.0, "clamped_zero"), ("slightly_negative", 160.0, "disparity_negative")):
        cu, cv = int(ul), 30
        half = sc.rng.integers(2, 254, (11, 11)).astype(np.uint8)
        sym = np.concatenate([half, half[:, -2::-1]], axis=1)   # 21 columns, symmetric about the centre
        sc.L[cv - 5:cv + 6, cu - 10:cu + 11] = sym
        sc.R[cv - 5:cv + 6, cu - 10:cu + 11] = sym
        x = f32(ul) if reason == "clamped_zero" else np.nextafter(f32(ul), f32(-np.inf))
        d = sc.desc()
        r = sc.right(f32(cu - 1), f32(cv), 0, sc.flip(d, 10))  # min at +1: bestuR = cu exactly
        sc.left(name, x, f32(cv), 0, d, reason, idx=r, off=1)
    pair("positive", 60.4, 30, 60.0, "matched", 0)
    # maxD = 72.68.  Both right keypoints pass the uR >= uL - maxD gate (70 px); the SAD minimum moves the
    # match to the true disparity: 72 - deltaR passes, 73 - deltaR does not
    pair("below_maxD", 150.0, 90, 80.0, "matched", -2)
    pair("above_maxD", 160.0, 150, 90.0, "disparity_ge_max", None)
    return sc.build()


# ------------------------------------------------------------------------------------------- cull
def cull_threshold(median):
    return f32(f32(f32(1.5) * f32(1.4)) * f32(median))       # :1338-1339


# population -> (SADs, the median = sorted SADs[M / 2], written by hand)
CULL_POPULATIONS = {
    "M1": ([50], 50), "M1_zero": ([0], 0), "M2": ([10, 21], 21), "M7": ([10, 20, 30, 40, 50, 60, 85], 40),
    "M8": ([10, 20, 30, 40, 50, 60, 70, 100], 50), "straddle_128": ([126, 127, 128, 129, 255, 256, 271, 272], 255),
    "straddle_128_low": ([126, 127, 128, 129, 255, 256], 129),
    "above_16384": ([10, 12, 14, 16, 121 * 140], 14), "all_equal": ([40, 40, 40, 40], 40),
    "median_zero": ([0, 0, 0, 5, 9], 0),
    "threshold": ([100, 100, 100, int(np.floor(cull_threshold(100))), int(np.floor(cull_threshold(100))) + 1], 100),
}


def _spread(rng, base, total):
    """base (11x11 uint8) with absolute pixel changes that add up to `total`."""
    out = base.astype(np.int64)
    order = rng.permutation(121)
    k = 0
    while total > 0:
        y, x = divmod(int(order[k % 121]), 11)
        room = min(total, 60)
        step = room if out[y, x] + room <= 255 else -room
        assert 0 <= out[y, x] + step <= 255
        out[y, x] += step
        total -= room
        k += 1
        assert k <= 121
    return out.astype(np.uint8)


def cull():
    sc = Scene(14, noise=0)
    D0 = 20
    sc.shift(0, S, 0, S - D0, D0)
    subsets, sads = {}, {}
    slot = 0
    for name, (pop, median) in CULL_POPULATIONS.items():
        assert sorted(pop)[len(pop) // 2] == median, name
        th = cull_threshold(median)
        subsets[name] = []
        for s in pop:
            cv, cul = 8 + 13 * (slot // 8), 36 + 25 * (slot % 8)
            slot += 1
            cur = cul - D0
            if s > 16384:   # flat patches: SAD(inc) = 121 * 140 + 11 * 115 * |inc|
                sc.L[cv - 5:cv + 6, cul - 5:cul + 6] = 0
                sc.R[cv - 5:cv + 6, cur - 10:cur + 11] = 255
                sc.R[cv - 5:cv + 6, cur - 5:cur + 6] = 140
            else:
                sc.R[cv - 5:cv + 6, cur - 5:cur + 6] = _spread(sc.rng, sc.L[cv - 5:cv + 6, cul - 5:cul + 6], s)
            d = sc.desc()
            r = sc.right(f32(cur), f32(cv), 0, sc.flip(d, 10))
            i = sc.left(f"{name}_sad{s}", f32(cul), f32(cv), 0, d, "matched" if f32(s) < th else "culled", idx=r, off=0)
            subsets[name].append(i)
            sads[i] = s
    assert 8 + 13 * ((slot - 1) // 8) + 6 < S
    g = sc.build()
    return g._replace(subsets={k: np.array(v) for k, v in subsets.items()}, expected_sad=sads)


# ------------------------------------------------------------------------------------------ batch
BATCH_COUNTS_L, BATCH_COUNTS_R, BATCH_CAP_L, BATCH_CAP_R = [33, 0, 5, 37], [130, 40, 0, 64], 37, 130


def batch():
    """B = 4 frames: n_l not a multiple of the 4 waves of a block, an empty left frame and an empty right frame
    in the middle (no match survives in either), cap_l > n_l, and survivors again in the last frame."""
    frames = []
    D0 = 20
    for f, (nl, nr) in enumerate(zip(BATCH_COUNTS_L, BATCH_COUNTS_R)):
        sc = Scene(20 + f)
        sc.shift(0, S, 0, S - D0, D0)
        for i in range(nl):
            cv, cul = 8 + 13 * (i // 8), 36 + 25 * (i % 8)
            d = sc.desc()
            if nr:
                r = sc.right(f32(cul - D0), f32(cv), 0, sc.flip(d, 10 + i))
                # 10 + i reaches 75 at i = 65: every pair here is below the threshold
                sc.left(f"f{f}_{i}", f32(cul), f32(cv), 0, d, "matched", idx=r, off=0)
            else:
                sc.left(f"f{f}_{i}", f32(cul), f32(cv), 0, d, "no_row_candidates")
        if nl == 0:
            for i in range(min(nr, 8)):
                sc.right(f32(30 + i), f32(40), 0, sc.desc())
        frames.append(sc.build(n_r=nr) if nr else sc.build())
    g0 = frames[0]
    return Group(np.stack([g.left_image for g in frames]), np.stack([g.right_image for g in frames]),
                 [g.kps_l for g in frames], [g.desc_l for g in frames], [g.kps_r for g in frames],
                 [g.desc_r for g in frames], g0.bf, g0.b, [g.expected_reasons for g in frames],
                 [g.names for g in frames], [g.expected_idx for g in frames], [g.expected_offset for g in frames],
                 counts=(BATCH_COUNTS_L, BATCH_COUNTS_R, BATCH_CAP_L, BATCH_CAP_R))


GROUPS = {"hamming": hamming, "window": window, "disparity": disparity, "cull": cull}
# reason codes each group must produce (test_stereo_cases_cpu.py asserts that each occurs)
GROUP_REASONS = {
    "hamming": {"no_row_candidates", "hamming_ge_75", "matched"},
    "window": {"window_right_edge", "window_view_bound", "best_at_minus_L", "best_at_plus_L", "matched"},
    "disparity": {"disparity_negative", "disparity_ge_max", "clamped_zero", "matched"},
    "cull": {"matched", "culled"},
}
