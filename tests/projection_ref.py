"""Python restatement of both ORBmatcher::SearchByProjection overloads the tracker runs -- (CurrentFrame,
LastFrame, th, bMono) (reference src/ORBmatcher.cc:1951-2185) and (Frame, local map points, th, bFarPoints,
thFarPoints) (src/ORBmatcher.cc:46-240) -- with Frame::AssignFeaturesToGrid / GetFeaturesInArea
(src/Frame.cc:1418-1440, 859-951): the second reference next to the C++ oracle, and what the GPU tests
compare against.  float32 arithmetic; the contracted multiply-adds round once (fuse_ref.fma32).

Besides (n, assign) each search returns one record per point saying why it ended as it did, and what the
in-order rule had to do for it, so a test can show on the reference side which path of the kernels a scene
takes (the kernels' own counters are not read):
  reason          one of REASONS
  match, dist     the keypoint taken and its distance (-1, 256: none)
  u, v, radius    the window centre and radius (NaN before they exist)
  cands           [(keypoint, distance)] passing the static tests, in scan order (cells ix outer, iy inner,
                  index order inside a cell): the candidate kernels' lists
  n_usable        candidates with distance < 256 that no map point held before the call
  affected        some usable candidate is also a usable candidate of an earlier observed point
                  (k_resolve_init's classification: only such a point enters the rounds)
  claimed_before  usable candidates an earlier observed point of this call held when the point's turn came
  rank, rank2     position of the best / second-best taken in the (distance, order)-sorted usable list
                  (-1: none); rank >= 8 means the kernels' eight best did not hold the answer
  depth           0 when no claim changed the point's answer, else 1 + the largest depth among the points
                  whose claims did; the scene's rounds_needed = 1 + max depth is the longest displacement
                  chain, a lower bound of the rounds the parallel fixed point takes
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from fuse_ref import fma32, roundf

f32 = np.float32
COLS, ROWS = 64, 48
TH_HIGH = 100

(NOT_VALID, BEHIND, OUT_OF_BOUNDS, NO_WINDOW, NO_CANDIDATE, ABOVE_TH_HIGH, RATIO, MATCHED, REMOVED, NOT_IN_VIEW, BAD,
 FAR) = range(12)
REASONS = ("not valid", "behind the camera", "out of bounds", "no window", "no candidate", "best above 100",
           "ratio test", "matched", "matched, removed by the rotation filter", "not in view", "bad", "too far")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


class Point:
    __slots__ = ("reason", "match", "dist", "u", "v", "radius", "cands", "n_usable", "affected", "claimed_before",
                 "rank", "rank2", "depth", "bin")

    def __init__(self):
        self.reason, self.match, self.dist = NOT_VALID, -1, 256
        self.u = self.v = self.radius = f32(np.nan)
        self.cands, self.n_usable, self.affected, self.claimed_before = [], 0, False, 0
        self.rank = self.rank2 = -1
        self.depth, self.bin = 0, -1

    def __repr__(self):
        return (f"<{REASONS[self.reason]} match={self.match} dist={self.dist} cands={len(self.cands)} "
                f"usable={self.n_usable} claimed={self.claimed_before} rank={self.rank}/{self.rank2} depth={self.depth}>")


class Result(NamedTuple):
    n: int
    assign: np.ndarray
    points: list
    rounds_needed: int
    n_affected: int
    hist: object = None      # frame overload with checkOri: the 30 bin counts
    kept_bins: object = None  # ... and ComputeThreeMaxima's (ind1, ind2, ind3)


def grid_products(F):
    """(x - mnMinX) * mfGridElementWidthInv and the same in y, float32, per keypoint."""
    k = F.mvKeysUn
    return ((k["x"] - f32(F.mnMinX)) * f32(F.mfGridElementWidthInv),
            (k["y"] - f32(F.mnMinY)) * f32(F.mfGridElementHeightInv))


def build_grid(F):
    """Frame::AssignFeaturesToGrid: cell (round(px), round(py)) with C round (half away from zero) on the
    float32 products; (cell_off [3073], cell_idx), cell = ix * 48 + iy, index order inside a cell."""
    if F.N == 0:
        return np.zeros(COLS * ROWS + 1, np.int64), np.zeros(0, np.int64)
    gx, gy = grid_products(F)
    px, py = roundf(gx), roundf(gy)
    idx = np.flatnonzero((px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS))
    cell = px[idx] * ROWS + py[idx]
    order = idx[np.argsort(cell, kind="stable")]
    off = np.zeros(COLS * ROWS + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(cell, minlength=COLS * ROWS))
    return off, order


def window_cells(F, u, v, r):
    """GetFeaturesInArea's cell range (x0, x1, y0, y1), or None."""
    iw, ih = f32(F.mfGridElementWidthInv), f32(F.mfGridElementHeightInv)
    a, b = f32(u - f32(F.mnMinX)), f32(v - f32(F.mnMinY))
    x0 = max(0, math.floor(f32(f32(a - r) * iw)))
    x1 = min(COLS - 1, math.ceil(f32(f32(a + r) * iw)))
    y0 = max(0, math.floor(f32(f32(b - r) * ih)))
    y1 = min(ROWS - 1, math.ceil(f32(f32(b + r) * ih)))
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return None
    return x0, x1, y0, y1


def _scan(F, grid, cells, u, v, r, lo, hi, check, ur, desc):
    """The window's candidates in scan order: level range, |dx|, |dy| < r, the u_R gate; [(j, distance)]."""
    off, order = grid
    kx, ky, ko = F.mvKeysUn["x"], F.mvKeysUn["y"], F.mvKeysUn["octave"]
    x0, x1, y0, y1 = cells
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = ix * ROWS + iy
            for j in order[off[c]:off[c + 1]]:
                if check and (ko[j] < lo or (hi >= 0 and ko[j] > hi)):
                    continue
                if not (abs(f32(kx[j] - u)) < r and abs(f32(ky[j] - v)) < r):
                    continue
                if F.mvuRight is not None and F.mvuRight[j] > 0 and abs(f32(ur - F.mvuRight[j])) > r:
                    continue
                out.append((int(j), hamming(desc, F.mDescriptors[j])))
    return out


class _InOrder:
    """The state both loops share: who holds a keypoint, the first observed lister of each keypoint, and
    the displacement depth of every point."""

    def __init__(self, n_cur, taken=None):
        self.taken0 = np.zeros(n_cur, bool) if taken is None else np.asarray(taken).astype(bool).copy()
        self.owner = np.full(n_cur, -1, np.int64)   # the observed point of this call holding the keypoint
        self.lister = {}
        self.depth = []

    def begin(self, i, p, observed):
        """Fill the record's usable / affected / claimed fields; returns the sorted usable list as
        [(distance, position, keypoint, claimed)]."""
        us = [(d, k, j) for k, (j, d) in enumerate(p.cands) if d < 256 and not self.taken0[j]]
        p.n_usable = len(us)
        p.affected = any(self.lister.get(j, i) < i for _, _, j in us)
        if observed:
            for _, _, j in us:
                self.lister.setdefault(j, i)
        us.sort()
        us = [(d, k, j, self.owner[j] >= 0) for d, k, j in us]
        p.claimed_before = sum(1 for e in us if e[3])
        return us

    def end(self, p, us, limit_rank):
        """depth from the claims ranked before limit_rank (None: all of them)."""
        lim = len(us) if limit_rank is None or limit_rank < 0 else limit_rank
        infl = [self.depth[self.owner[j]] for r, (_, _, j, c) in enumerate(us) if c and r < lim]
        p.depth = 1 + max(infl) if infl else 0


def search_frame(C, L, th, mono, check_ori) -> Result:
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) with the matcher's checkOri."""
    grid = build_grid(C)
    T = C.Tcw.reshape(-1).astype(f32)
    twc = [f32(-fma32(T[8 + i], T[11], fma32(T[i], T[3], f32(T[4 + i] * T[7])))) for i in range(3)]
    Tl = L.Tcw.reshape(-1).astype(f32)
    tlc_z = f32(fma32(Tl[10], twc[2], fma32(Tl[8], twc[0], f32(Tl[9] * twc[1]))) + Tl[11])
    fwd = bool(tlc_z > f32(C.mb)) and not mono
    bwd = bool(-tlc_z > f32(C.mb)) and not mono
    mp = L.map_points
    X = np.asarray(mp["xyz"], f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        xc = [(fma32(T[4 * r + 2], X[:, 2], fma32(T[4 * r], X[:, 0], T[4 * r + 1] * X[:, 1])) + T[4 * r + 3]).astype(f32)
              for r in range(3)] if L.N else [np.zeros(0, f32)] * 3
        invz = (1.0 / xc[2].astype(np.float64)).astype(f32)
        U = (f32(C.fx) * xc[0] / xc[2] + f32(C.cx)).astype(f32)
        V = (f32(C.fy) * xc[1] / xc[2] + f32(C.cy)).astype(f32)
        UR = fma32(-f32(C.mbf), invz, U) if L.N else U
    state = _InOrder(C.N)
    assign = np.full(C.N, -1, np.int64)
    obs = np.asarray(mp["observed"]).astype(bool)
    pts, n = [], 0
    for i in range(L.N):
        p = Point()
        pts.append(p)
        state.depth.append(0)
        if not mp["valid"][i]:
            continue
        if invz[i] < 0:
            p.reason = BEHIND
            continue
        u, v = U[i], V[i]
        p.u, p.v = u, v
        if u < f32(C.mnMinX) or u > f32(C.mnMaxX) or v < f32(C.mnMinY) or v > f32(C.mnMaxY):
            p.reason = OUT_OF_BOUNDS
            continue
        o = int(L.mvKeysUn[i]["octave"])
        r = f32(f32(th) * C.mvScaleFactors[o])
        p.radius = r
        lo, hi = (o, -1) if fwd else ((0, o) if bwd else (o - 1, o + 1))
        cells = window_cells(C, u, v, r)
        if cells is None:
            p.reason = NO_WINDOW
            continue
        p.cands = _scan(C, grid, cells, u, v, r, lo, hi, lo > 0 or hi >= 0, UR[i], mp["desc"][i])
        us = state.begin(i, p, obs[i])
        free = [r_ for r_, e in enumerate(us) if not e[3]]
        p.rank = free[0] if free else -1
        state.end(p, us, p.rank)
        state.depth[i] = p.depth
        if not free:
            p.reason = NO_CANDIDATE
            continue
        d, _, j, _ = us[free[0]]
        p.dist = d
        if d > TH_HIGH:
            p.reason = ABOVE_TH_HIGH
            continue
        p.reason, p.match = MATCHED, j
        assign[j] = i
        if obs[i]:
            state.owner[j] = i
        n += 1
        if check_ori:
            rot = f32(L.mvKeysUn[i]["angle"] - C.mvKeysUn[j]["angle"])
            if rot < 0:
                rot = f32(rot + f32(360))
            b = int(roundf(f32(rot * f32(f32(1) / f32(30)))))
            p.bin = 0 if b == 30 else b
    hist = keep = None
    if check_ori:
        hist = [sum(1 for p in pts if p.bin == b) for b in range(30)]
        keep = three_maxima(hist)
        for p in pts:
            if p.bin >= 0 and p.bin not in keep:
                p.reason = REMOVED
                assign[p.match] = -1
                n -= 1
    return Result(n, assign, pts, 1 + max(state.depth, default=0), sum(p.affected for p in pts), hist, keep)


def three_maxima(sizes):
    """ComputeThreeMaxima (src/ORBmatcher.cc:2336-2378): (ind1, ind2, ind3), -1 where cut."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for b, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, b
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, b
        elif s > m3:
            m3, i3 = s, b
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def search_local(F, P, th, far, th_far, ratio, taken=None) -> Result:
    """SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) with the matcher's nnratio; taken[j]:
    keypoint j held a map point with observations before the call."""
    grid = build_grid(F)
    state = _InOrder(F.N, taken)
    match = np.full(F.N, -1, np.int64)
    ko = F.mvKeysUn["octave"]
    pts, n = [], 0
    for i in range(P.n):
        p = Point()
        pts.append(p)
        state.depth.append(0)
        if not P.track_in_view[i]:
            p.reason = NOT_IN_VIEW
            continue
        if far and P.track_depth[i] > f32(th_far):
            p.reason = FAR
            continue
        if P.is_bad[i]:
            p.reason = BAD
            continue
        lvl = int(P.track_level[i])
        r = f32(2.5) if float(P.track_view_cos[i]) > 0.998 else f32(4.0)
        if f32(th) != f32(1.0):
            r = f32(r * f32(th))
        rad = f32(r * F.mvScaleFactors[lvl])
        x, y, xr = (f32(v) for v in P.track_proj[i])
        p.u, p.v, p.radius = x, y, rad
        cells = window_cells(F, x, y, rad)
        if cells is None:
            p.reason = NO_WINDOW
            continue
        p.cands = _scan(F, grid, cells, x, y, rad, lvl - 1, lvl, True, xr, P.desc[i])
        us = state.begin(i, p, bool(P.observed[i]))
        free = [r_ for r_, e in enumerate(us) if not e[3]]
        p.rank = free[0] if free else -1
        p.rank2 = free[1] if len(free) > 1 else -1
        state.end(p, us, p.rank2)
        state.depth[i] = p.depth
        if not free:
            p.reason = NO_CANDIDATE
            continue
        b1, _, bi, _ = us[free[0]]
        l1 = int(ko[bi])
        b2, l2 = (us[free[1]][0], int(ko[us[free[1]][2]])) if len(free) > 1 else (256, -1)
        p.dist = b1
        if b1 > TH_HIGH:
            p.reason = ABOVE_TH_HIGH
            continue
        if l1 == l2 and f32(b1) > f32(f32(ratio) * f32(b2)):
            p.reason = RATIO
            continue
        p.reason, p.match = MATCHED, bi
        match[bi] = i
        if P.observed[i]:
            state.owner[bi] = i
        n += 1
    return Result(n, match, pts, 1 + max(state.depth, default=0), sum(p.affected for p in pts))


def py_search(C, L, th, mono, check_ori):
    r = search_frame(C, L, th, mono, check_ori)
    return r.n, r.assign


def py_search_local(F, P, th, far, th_far, ratio, taken=None):
    r = search_local(F, P, th, far, th_far, ratio, taken)
    return r.n, r.assign
