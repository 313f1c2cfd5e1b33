"""Hand-built SearchByProjection scenes, one function per group, each returning a `Group`: the inputs of one
call, a name and the prescribed projection_ref reason per point, and the prescribed keypoint where one is.
test_projection_cases_cpu.py checks every prescription against projection_ref and the oracle;
test_projection_cases_gpu.py runs the groups on every form of the kernels.

The frame every group uses: image bounds 0..640 x 0..480 (both grid inverses are the float 0.1), 8 levels of
1.2, identity current pose, fx = fy = 512, cx = 320, cy = 240, bf = 64 (mb = 0.125).  A last-frame point
meant to project to (u, v) sits at depth Z, a power of two: X = (u - cx) Z / fx is then a float, and the
projection fx X / Z + cx gives u back exactly whenever (u - cx) + cx does (checked when the point is added,
and again by the CPU test on the reference's u, v).  "The next float beyond" a bound is np.nextafter, except
below the lower image bounds, where the sum (u - cx) + cx cannot produce a subnormal: there it is the largest
negative value the projection can produce (-2^-15 in u, -2^-16 in v).

Descriptors: a point's descriptor is random; a keypoint meant to lie at distance d from it is the point's
descriptor with d chosen bits flipped, so every distance that matters is prescribed.  Unrelated keypoints
are ~128 +- 8 bits away and never win.

Sites: cases that must not see each other's keypoints sit on a 20-px lattice (th = 7 at octave 0 is a 7-px
radius)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import conftest
import projection_ref as ref

conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402

f32 = np.float32
W, H, FX, CX, CY, BF = 640, 480, 512.0, 320.0, 240.0, 64.0
NLEVELS = 8
SCALE = [f32(1)]
for _ in range(1, NLEVELS):
    SCALE.append(f32(float(SCALE[-1]) * float(f32(1.2))))
SCALE = np.array(SCALE, f32)
LEVEL_SIGMA2 = (SCALE * SCALE).astype(f32)
IDENTITY = np.eye(4, dtype=f32)[:3]

M, R = ref.MATCHED, ref.REMOVED


class Group(NamedTuple):
    kind: str                 # "frame" or "local"
    cur: dict                 # pkg.Frame arguments of the current frame
    last: object              # frame: pkg.Frame arguments of the last frame (with map_points)
    points: object            # local: pkg.LocalMapPoints arguments
    params: dict              # frame: th, mono, check_ori; local: th, far, th_far, ratio, taken
    names: list               # case name per point
    expected: list            # projection_ref reason per point
    expected_match: dict      # {point: keypoint}
    intended_uv: dict         # frame: {point: (u, v)} the projection must give, bit for bit
    claims: dict              # structural claims the CPU test checks on the reference's diagnostics


def up(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


def down(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(-np.inf))
    return x


def flip(desc, d, start=0):
    """desc with bits start .. start + d - 1 flipped: Hamming distance d."""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + d] ^= 1
    return np.packbits(bits)


class _Scene:
    def __init__(self, seed, stereo=True):
        self.rng = np.random.default_rng(seed)
        self.kps, self.kdesc, self.kur = [], [], []
        self.stereo = stereo
        self.names, self.expected, self.match, self.claims = [], [], {}, {}

    def rand_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def kp(self, x, y, octave=0, angle=0.0, desc=None, ur=-1.0):
        self.kps.append((f32(x), f32(y), 31.0, f32(angle), 1.0, int(octave), -1))
        self.kdesc.append(self.rand_desc() if desc is None else np.asarray(desc, np.uint8))
        self.kur.append(f32(ur))
        return len(self.kps) - 1

    def clutter(self, n, y0=300.0, y1=470.0):
        """n keypoints no window of the scene reaches (all windows lie above y0 - 60)."""
        x = self.rng.uniform(10, 630, n).astype(f32)
        y = self.rng.uniform(y0, y1, n).astype(f32)
        o = self.rng.integers(0, NLEVELS, n)
        d = self.rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for i in range(n):
            self.kps.append((x[i], y[i], 31.0, f32(0), 1.0, int(o[i]), -1))
            self.kur.append(f32(-1))
        self.kdesc.extend(d)

    def cur(self):
        k = np.array(self.kps, dtype=KEYPOINT_DTYPE) if self.kps else np.zeros(0, KEYPOINT_DTYPE)
        d = np.array(self.kdesc, np.uint8).reshape(len(k), 32)
        return dict(keys_un=k, descriptors=d, Tcw=IDENTITY.copy(), camera=(FX, FX, CX, CY), scale_factors=SCALE,
                    width=W, height=H, bf=BF, u_right=np.array(self.kur, f32) if self.stereo else None)

    def _case(self, name, expect, match):
        i = len(self.names)
        self.names.append(name)
        self.expected.append(expect)
        if match is not None:
            self.match[i] = match
        return i


class FrameScene(_Scene):
    """A SearchByProjection(CurrentFrame, LastFrame) call.  tz: the last frame's tcw.z, which is tlc.z for
    the identity current pose (forward when tz > mb = 0.125, backward when -tz > mb)."""

    def __init__(self, seed, th=7, mono=False, check_ori=True, stereo=True, tz=0.0):
        super().__init__(seed, stereo)
        self.th, self.mono, self.check_ori, self.tz = th, mono, check_ori, tz
        self.xyz, self.pdesc, self.poct, self.pang, self.valid, self.obs, self.uv = [], [], [], [], [], [], {}

    def pt(self, name, u, v, expect, match=None, Z=4.0, octave=0, angle=0.0, valid=1, observed=1, desc=None, xyz=None):
        i = self._case(name, expect, match)
        if xyz is None:
            u, v = f32(u), f32(v)
            X, Y = f32((float(u) - CX) * Z / FX), f32((float(v) - CY) * Z / FX)
            assert f32(f32(f32(FX) * X) / f32(Z)) + f32(CX) == u and f32(f32(f32(FX) * Y) / f32(Z)) + f32(CY) == v, \
                (name, u, v)
            xyz = (X, Y, f32(Z))
            self.uv[i] = (u, v)
        self.xyz.append(xyz)
        self.pdesc.append(self.rand_desc() if desc is None else np.asarray(desc, np.uint8))
        self.poct.append(octave)
        self.pang.append(f32(angle))
        self.valid.append(valid)
        self.obs.append(observed)
        return i

    def pair(self, name, u, v, expect=M, dist=10, ang=0.0, cur_ang=0.0, observed=1, Z=4.0, octave=0):
        """A keypoint at (u, v) and a point projecting onto it at distance `dist`."""
        d = self.rand_desc()
        j = self.kp(u, v, octave=octave, angle=cur_ang, desc=flip(d, dist))
        return self.pt(name, u, v, expect, match=j if expect in (M, R) else None, Z=Z, octave=octave, angle=ang,
                       observed=observed, desc=d), j

    def build(self, **claims):
        n = len(self.names)
        xyz = np.array(self.xyz, f32).reshape(n, 3)
        assert len({tuple(r) for r in xyz.tolist()}) == n, "last-frame points must have distinct positions"
        lk = np.zeros(n, KEYPOINT_DTYPE)
        lk["x"], lk["y"] = 5.0 + np.arange(n) % 600, 7.0
        lk["octave"], lk["angle"] = self.poct, self.pang
        Tl = IDENTITY.copy()
        Tl[2, 3] = self.tz
        cur = self.cur()
        last = dict(cur, keys_un=lk, descriptors=np.zeros((n, 32), np.uint8), Tcw=Tl, u_right=None,
                    map_points=dict(valid=np.array(self.valid, np.uint8), observed=np.array(self.obs, np.uint8), xyz=xyz,
                                    desc=np.array(self.pdesc, np.uint8).reshape(n, 32)))
        self.claims.update(claims)
        return Group("frame", cur, last, None, dict(th=self.th, mono=self.mono, check_ori=self.check_ori),
                     self.names, self.expected, self.match, self.uv, self.claims)


class LocalScene(_Scene):
    """A SearchByProjection(Frame, local map points) call."""

    def __init__(self, seed, th=1, far=False, th_far=8.0, ratio=0.8, stereo=True):
        super().__init__(seed, stereo)
        self.th, self.far, self.th_far, self.ratio = th, far, th_far, ratio
        self.f = {k: [] for k in ("track_in_view", "is_bad", "observed", "track_proj", "track_view_cos", "track_depth",
                                  "track_level", "desc")}
        self.taken = []

    def pt(self, name, x, y, expect, match=None, xr=0.0, level=0, cos=0.5, depth=1.0, in_view=1, bad=0, observed=1,
           desc=None):
        i = self._case(name, expect, match)
        for k, v in (("track_in_view", in_view), ("is_bad", bad), ("observed", observed),
                     ("track_proj", (f32(x), f32(y), f32(xr))), ("track_view_cos", f32(cos)), ("track_depth", f32(depth)),
                     ("track_level", level), ("desc", self.rand_desc() if desc is None else np.asarray(desc, np.uint8))):
            self.f[k].append(v)
        return i

    def build(self, **claims):
        n = len(self.names)
        pts = dict(self.f, track_proj=np.array(self.f["track_proj"], f32).reshape(n, 3),
                   desc=np.array(self.f["desc"], np.uint8).reshape(n, 32))
        taken = np.zeros(len(self.kps), np.uint8)
        taken[self.taken] = 1
        self.claims.update(claims)
        return Group("local", self.cur(), None, pts, dict(th=self.th, far=self.far, th_far=self.th_far, ratio=self.ratio,
                                                          taken=taken), self.names, self.expected, self.match, {},
                     self.claims)


def sites(x0=30.0, y0=30.0, step=20.0, x1=610.0):
    x, y = x0, y0
    while True:
        yield x, y
        x += step
        if x > x1:
            x, y = x0, y + step


# ---- SearchByProjection(CurrentFrame, LastFrame) ---------------------------------------------------

def frame_gates():
    """valid, depth sign and the image bounds (inclusive on all four sides).  12 points, 11 keypoints."""
    s = FrameScene(101)
    s.pair("valid", 100, 100)
    p, _ = s.pair("valid=0", 140, 100, expect=ref.NOT_VALID)
    s.valid[p] = 0
    d = s.rand_desc()
    s.kp(180, 100, desc=d)
    s.pt("depth<0", 180, 100, ref.BEHIND, desc=d, xyz=(f32(-1.09375), f32(-1.09375), f32(-4.0)))  # projects onto (180, 100)
    for name, u, v, kx, ky in (("u==mnMinX", 0, 200, 4, 200), ("u==mnMaxX", 640, 200, 634, 200),
                               ("v==mnMinY", 300, 0, 300, 4), ("v==mnMaxY", 300, 480, 300, 474)):
        d = s.rand_desc()   # (the keypoint inside: x >= 635 / y >= 475 round to cell 64 / 48, no cell)
        s.pt(name, u, v, M, match=s.kp(kx, ky, desc=flip(d, 10)), desc=d)
    for name, u, v in (("u below mnMinX", f32(-2.0 ** -15), 220), ("u above mnMaxX", up(640), 220),
                       ("v below mnMinY", 340, f32(-2.0 ** -16)), ("v above mnMaxY", 340, up(480))):
        d = s.rand_desc()
        s.kp(min(max(float(u), 0.0), 639.0), min(max(float(v), 0.0), 479.0), desc=d)
        s.pt(name, u, v, ref.OUT_OF_BOUNDS, desc=d)
    return s.build()


def half_cell_keypoints(s, desc_for):
    """Keypoints whose grid product is exactly k + 0.5: C round puts them in cell k + 1 (k >= 0) or k (k < 0),
    rint / numpy's round in the even neighbour.  Returns {keypoint: (axis, product)}."""
    out = {}
    for axis, vals in (("x", (5.0, 15.0, 25.0, 625.0)), ("y", (5.0, 15.0, 465.0))):
        for c in vals:
            x, y = (c, 205.0) if axis == "x" else (305.0, c)
            out[s.kp(x, y, desc=desc_for(x, y))] = (axis, f32(f32(c) * f32(0.1)))
    return out


def frame_grid():
    """Every half-cell keypoint is found from a point 6.5 px away whose window
    reaches its (rounded-up) cell; keypoints at x = -5 (cell -1) and x = 640 (cell 64) are in no cell and
    never candidates although inside a window; windows clamped at columns 0 / 63 and rows 0 / 47."""
    s = FrameScene(102)
    descs = []
    half = half_cell_keypoints(s, lambda x, y: (descs.append(s.rand_desc()), flip(descs[-1], 10))[1])
    for (j, (axis, prod)), d in zip(half.items(), descs):
        x, y = float(s.kps[j][0]), float(s.kps[j][1])
        u, v = (x - 2.5, y) if axis == "x" else (x, y - 2.5)
        s.pt(f"half cell {axis}={x if axis == 'x' else y}", u, v, M, match=j, desc=d)
    d = s.rand_desc()
    out1 = s.kp(-5.0, 105.0, desc=flip(d, 10))
    s.pt("keypoint at x=-5 (cell -1)", 1.0, 105.0, ref.NO_CANDIDATE, desc=d)
    d = s.rand_desc()
    out2 = s.kp(640.0, 125.0, desc=flip(d, 10))
    s.pt("keypoint at x=640 (cell 64)", 636.0, 125.0, ref.NO_CANDIDATE, desc=d)
    d = s.rand_desc()
    out3 = s.kp(325.0, 480.0, desc=flip(d, 10))
    s.pt("keypoint at y=480 (cell 48)", 325.0, 476.0, ref.NO_CANDIDATE, desc=d)
    for name, u, v, kx, ky in (("window clamped at column 0", 2.0, 145.0, 4.0, 145.0),
                               ("window clamped at column 63", 638.0, 165.0, 634.0, 165.0),
                               ("window clamped at row 0", 345.0, 2.0, 345.0, 4.0),
                               ("window clamped at row 47", 365.0, 478.0, 365.0, 474.0)):
        d = s.rand_desc()
        s.pt(name, u, v, M, match=s.kp(kx, ky, desc=flip(d, 10)), desc=d)
    return s.build(half_cells=half, outside=[out1, out2, out3])


def _lattice(s, cx, cy, xs, ys, desc, octave, winner, far_from=60):
    """Keypoints at (cx + dx, cy + dy), dx outer / dy inner; number `winner` at distance 20, the others at
    60 + (k % 30).  Returns the keypoint indices."""
    out, k = [], 0
    for dx in xs:
        for dy in ys:
            out.append(s.kp(cx + dx, cy + dy, octave=octave, desc=flip(desc, 20 if k == winner else far_from + k % 30)))
            k += 1
    return out


def frame_window_walk():
    """th = 15 at octave 7 (radius 53.7 px): windows of 12 x 12 = 144 cells; one holds 154 candidates (the host
    call's first capacity is 128: it grows and runs again) with the winner at list position > 128, one holds
    77; both have columns of empty cells between occupied ones and five keypoints in one cell.  2 points,
    241 keypoints."""
    s = FrameScene(103, th=15)
    xs = [-50, -45, -40, -35, -30, -25, -20, 20, 25, 30, 35, 40, 45, 50]
    ys = list(range(-50, 51, 10))
    d = s.rand_desc()
    ks = _lattice(s, 120.0, 240.0, xs, ys, d, 7, winner=141)
    a = s.pt("154 candidates, winner late", 120, 240, M, match=ks[141], octave=7, desc=d)
    d = s.rand_desc()
    ks = _lattice(s, 450.0, 240.0, xs[:4] + xs[-3:], ys, d, 6, winner=70)
    for q in range(5):   # five more in one cell, scanned before the lattice's entry of that cell
        s.kp(450.0 - 48.0 + 0.5 * q, 240.0 - 49.0, octave=7, desc=flip(d, 90 + q))
    b = s.pt("82 candidates, one cell of six", 450, 240, M, match=ks[70], octave=7, desc=d)
    return s.build(n_cands={a: 154, b: 82}, cells_gt=64, winner_pos_gt={a: 128, b: 64})


def _octave_cases(s, site, lo_fn, hi_fn):
    """For point octaves 0, 3 and 7: one keypoint of every octave 0..7 at one site each."""
    for oct_ in (0, 3, 7):
        r = float(f32(f32(s.th) * SCALE[oct_]))
        for ko in range(NLEVELS):
            x, y = next(site)
            while r > 9 and (x < 60 or x > 580 or y < 60):
                x, y = next(site)
            lo, hi = lo_fn(oct_), hi_fn(oct_)
            ok = ko >= lo and (hi < 0 or ko <= hi)
            d = s.rand_desc()
            j = s.kp(x, y, octave=ko, desc=flip(d, 10))
            s.pt(f"point octave {oct_}, keypoint octave {ko}", x, y, M if ok else ref.NO_CANDIDATE,
                 match=j if ok else None, octave=oct_, desc=d, Z=2.0 ** (1 + ko % 3))


def _radius_edges(s, site):
    for name, dx, dy, ok in (("dx == r", 7.0, 0.0, False), ("dx == -r", -7.0, 0.0, False), ("dy == r", 0.0, 7.0, False),
                             ("dy == -r", 0.0, -7.0, False), ("dx just inside r", float(down(107.0)) - 100.0, 0.0, True),
                             ("dy just inside -r", 0.0, float(up(93.0)) - 100.0, True)):
        x, y = next(site)
        d = s.rand_desc()
        kx = f32(x + dx) if abs(dx) == 7.0 or dx == 0 else (down(x + 7.0) if dx > 0 else up(x - 7.0))
        ky = f32(y + dy) if abs(dy) == 7.0 or dy == 0 else (down(y + 7.0) if dy > 0 else up(y - 7.0))
        j = s.kp(kx, ky, desc=flip(d, 10))
        s.pt(name, x, y, M if ok else ref.NO_CANDIDATE, match=j if ok else None, desc=d)


def _ur_edges(s, site):
    """Z = 4: ur = u - bf / 4 = u - 16."""
    for name, off, ok in (("uR == 0 bypasses", None, True), ("uR == -1 bypasses", None, True),
                          ("|ur - uR| == r passes", 7.0, True), ("|ur - uR| just above r fails", "up", False),
                          ("|ur - uR| == r (uR below) passes", -7.0, True),
                          ("|ur - uR| just above r (uR below) fails", "down", False)):
        x, y = next(site)
        ur = x - 16.0
        if off is None:
            kur = 0.0 if "== 0" in name else -1.0
        elif off == "up":
            kur = up(ur + 7.0)
        elif off == "down":
            kur = down(ur - 7.0)
        else:
            kur = ur + off
        if not s.stereo:
            ok = True
        d = s.rand_desc()
        j = s.kp(x, y, desc=flip(d, 10), ur=kur)
        s.pt(name, x, y, M if ok else ref.NO_CANDIDATE, match=j if ok else None, desc=d)


def _candidates(seed, lo_fn, hi_fn, **kw):
    s = FrameScene(seed, **kw)
    site = sites(100.0, 30.0, 20.0, 560.0)
    _radius_edges(s, site)
    _ur_edges(s, site)
    _octave_cases(s, _wide_sites_from(130.0), lo_fn, hi_fn)
    return s.build()


def _wide_sites_from(y0):
    return sites(70.0, y0, 64.0, 580.0)


def frame_candidates_default():
    """|dx|, |dy| == r rejected and the next float inside accepted; the u_R gate's bypass values and its
    inclusive edge; the default octave window oct-1 .. oct+1 at octaves 0, 3 and 7.  tlc.z == mb exactly:
    neither forward nor backward.  36 points and keypoints."""
    return _candidates(104, lambda o: o - 1, lambda o: o + 1, tz=0.125)


def frame_candidates_forward():
    """tlc.z just above mb: octaves oct .. open; at octave 0 there is no level check at all."""
    return _candidates(105, lambda o: o, lambda o: -1, tz=float(up(0.125)))


def frame_candidates_backward():
    """-tlc.z just above mb: octaves 0 .. oct."""
    return _candidates(106, lambda o: 0, lambda o: o, tz=-float(up(0.125)))


def frame_candidates_mono():
    """bMono disables forward and backward (tlc.z = 1 here): the default window."""
    return _candidates(107, lambda o: o - 1, lambda o: o + 1, tz=1.0, mono=True)


def frame_candidates_no_uright():
    """A frame without mvuRight: no u_R gate."""
    return _candidates(108, lambda o: o - 1, lambda o: o + 1, stereo=False)


def frame_distance():
    """best == 100 accepted, 101 rejected; the complemented descriptor (256) never taken; equal distances: the
    first in scan order (ix outer, iy inner, index inside a cell) wins, also when the lower keypoint index
    is in a later cell.  6 points, 12 keypoints."""
    s = FrameScene(109)
    site = sites()
    s.pair("best == 100", *next(site), dist=100)
    s.pair("best == 101", *next(site), dist=101, expect=ref.ABOVE_TH_HIGH)
    x, y = next(site)
    d = s.rand_desc()
    s.kp(x, y, desc=np.bitwise_not(d))
    s.pt("only candidate at 256", x, y, ref.NO_CANDIDATE, desc=d)
    # ties: site cells -- x = 110 is a cell boundary (cells 10 | 11 split at 105, 115)
    d = s.rand_desc()
    late = s.kp(118.0, 72.0, desc=flip(d, 30))            # column 12: scanned last, lowest index
    first = s.kp(112.0, 68.0, desc=flip(d, 30, 40))       # column 11, row 7
    s.kp(113.0, 76.0, desc=flip(d, 30, 80))               # column 11, row 8
    s.pt("tie: earlier cell beats lower index", 114.0, 72.0, M, match=first, desc=d)
    d = s.rand_desc()
    a = s.kp(211.0, 71.0, desc=flip(d, 30))
    s.kp(212.0, 72.0, desc=flip(d, 30, 40))
    s.pt("tie inside a cell: lower index", 211.5, 71.5, M, match=a, desc=d)
    d = s.rand_desc()
    s.kp(312.0, 78.0, desc=flip(d, 30))                   # row 8
    b = s.kp(313.0, 72.0, desc=flip(d, 30, 40))           # row 7: iy inner, scanned first
    s.pt("tie: iy inner", 312.5, 75.0, M, match=b, desc=d)
    return s.build(late_lower_index=(late, first))


def chain(s, x0, y, n=40, step=10.0, pt=None):
    """Keypoints k(0..n-1) `step` apart; point 0 sees only k(0), point i sees k(i-1) (its best) and k(i):
    in order, i -> k(i), and the parallel rounds need about n iterations."""
    d = s.rand_desc()
    ks = [s.kp(x0 + step * i, y, desc=flip(d, 10 + i)) for i in range(n)]
    for i in range(n):
        s.pt(f"chain point {i}", x0 + step * i - step / 2, y, M, match=ks[i], desc=d, Z=2.0 ** (1 + i % 4))
    return ks


def exhaustion(s, x, y, usable, taken, name):
    """`usable` keypoints within 2 px of (x, y); the `taken` best (distances 10, 11, ...) are each taken
    first by an earlier observed point carrying that keypoint's own descriptor; the others lie at 100, 101,
    ...: the point takes the first of them, at exactly 100, which the kernels reach only by the full scan
    when `taken` >= 8.  th = 3.  Returns {point: (claimed, rank)}."""
    d = s.rand_desc()
    ks = [s.kp(x - 2.0 + 1.0 * (q % 5), y - 1.0 + 1.0 * (q // 5), desc=flip(d, 10 + q if q < taken else 100 + q - taken))
          for q in range(usable)]
    for q in range(taken):
        kx, ky = float(s.kps[ks[q]][0]), float(s.kps[ks[q]][1])
        s.pt(f"{name}: taker {q}", kx, ky, M, match=ks[q], desc=s.kdesc[ks[q]], Z=2.0 ** (1 + q))
    p = s.pt(name, x, y, M if usable > taken else ref.NO_CANDIDATE, match=ks[taken] if usable > taken else None,
             desc=d, Z=2.0 ** 11)
    return {p: (taken, taken if usable > taken else -1)}


def frame_in_order():
    """The in-order rule.  Two observed points on one best keypoint; unobserved then observed (overwrites,
    both count); observed then unobserved (blocked); a 40-point chain; top-8 exhaustion: 12 usable with the 9
    best taken (takes its 10th), exactly 8 usable all taken (no match), 9 usable with 8 taken (the 9th).
    About 90 points and 90 keypoints."""
    s = FrameScene(110, th=3)
    d = s.rand_desc()
    a, b = s.kp(40.0, 30.0, desc=flip(d, 10)), s.kp(42.0, 30.0, desc=flip(d, 100))
    s.pt("same best: first", 41.0, 30.0, M, match=a, desc=d, Z=2.0)
    s.pt("same best: second takes its second best (at 100)", 41.0, 30.0, M, match=b, desc=d, Z=4.0)
    d = s.rand_desc()
    k = s.kp(80.0, 30.0, desc=flip(d, 10))
    s.pt("unobserved first (overwritten, counted)", 80.0, 30.0, M, match=k, desc=d, Z=2.0, observed=0)
    s.pt("observed second overwrites", 80.0, 30.0, M, match=k, desc=d, Z=4.0)
    d = s.rand_desc()
    k = s.kp(120.0, 30.0, desc=flip(d, 10))
    s.pt("observed first", 120.0, 30.0, M, match=k, desc=d, Z=2.0)
    s.pt("unobserved second is blocked", 120.0, 30.0, ref.NO_CANDIDATE, desc=d, Z=4.0, observed=0)
    chain(s, 100.0, 60.0, step=5.0)
    rank = {}
    for name, x, usable, taken in (("12 usable, 9 best taken", 100.0, 12, 9), ("8 usable, all taken", 200.0, 8, 8),
                                   ("9 usable, 8 taken", 300.0, 9, 8)):
        rank.update(exhaustion(s, x, 100.0, usable, taken, name))
    return s.build(rounds_needed=40, exhaustion=rank)


def rot_for_half(k):
    """An angle difference whose float product with 1.0f / 30 is exactly k + 0.5."""
    fac = f32(f32(1) / f32(30))
    x = f32((k + 0.5) * 30)
    for c in [x] + [g(x, q) for q in range(1, 16) for g in (up, down)]:
        if f32(c * fac) == f32(k + 0.5):
            return c
    raise AssertionError(k)


def _rotation(check_ori, counts, seed=111):
    """Matches with prescribed rotation bins.  counts: matches per bin for bins 1, 2, 3, ... (bin b's angle
    difference is 30 b, the factor being 1/30 as upstream has it).  On top: one match with rot * (1/30)
    exactly 4.5 (bin 5), one with rot < 0 (wraps: -30 -> 330 -> bin 11) and one with rot = 890 (bin 30 ->
    0); keypoints assigned twice across dropped / kept bins."""
    s = FrameScene(seed, th=3, check_ori=check_ori)
    site = sites()
    kept = ref.three_maxima([0] + list(counts) + [0] * (29 - len(counts)))
    for b, c in enumerate(counts, start=1):
        for q in range(c):
            x, y = next(site)
            s.pair(f"bin {b} #{q}", x, y, ang=30.0 * b, expect=M if (b in kept or not check_ori) else R)
    extra = {}
    x, y = next(site)
    extra[s.pair("rot * (1/30) == 4.5 -> bin 5", x, y, ang=float(rot_for_half(4)) + 10.0, cur_ang=10.0,
                 expect=M if (5 in kept or not check_ori) else R)[0]] = 5
    x, y = next(site)
    extra[s.pair("rot < 0 wraps -> bin 11", x, y, ang=10.0, cur_ang=40.0, expect=M if (11 in kept or not check_ori) else R)[0]] = 11
    x, y = next(site)
    extra[s.pair("rot 890: bin 30 folds to 0", x, y, ang=890.0, expect=M if (0 in kept or not check_ori) else R)[0]] = 0
    return s, site, kept, extra


def _twice(s, site, kept, check_ori, first_bin, second_bin, name):
    """One keypoint assigned by an unobserved point (first_bin) and then by an observed one (second_bin)."""
    x, y = next(site)
    d = s.rand_desc()
    k = s.kp(x, y, desc=flip(d, 10))
    ex = lambda b: M if (b in kept or not check_ori) else R
    s.pt(f"{name}: unobserved, bin {first_bin}", x, y, ex(first_bin), match=k, desc=d, Z=2.0, observed=0,
         angle=30.0 * first_bin)
    s.pt(f"{name}: observed, bin {second_bin}", x, y, ex(second_bin), match=k, desc=d, Z=4.0, angle=30.0 * second_bin)
    return k


def frame_rotation(check_ori=True):
    """Bins 1, 2, 3 end with 20, 2 and 1 matches: second == 0.1f * max1 is kept, the third (one less) is cut; the
    half-bin, wrap and fold cases; a keypoint assigned in a cut bin (unobserved) and then in a kept bin
    ends at -1 and the count drops by one; both in cut bins: by two.  About 30 points."""
    s, site, kept, extra = _rotation(check_ori, (19, 2, 1))
    k1 = _twice(s, site, kept, check_ori, 7, 1, "cut then kept")
    k2 = _twice(s, site, kept, check_ori, 9, 8, "cut twice")
    # with these bin 1 holds 20; bins 0, 3, 5, 7, 8, 9 and 11 hold one match each and are cut
    return _finish_rotation(s, check_ori, extra, ends_unassigned=[k1, k2] if check_ori else [])


def _finish_rotation(s, check_ori, extra, **claims):
    """The prescriptions were made from the planned counts; fix them from the final histogram (the cases
    added after the plan change it) -- still prescribed by construction, not read from a search."""
    bins = {}
    for i, (a, n) in enumerate(zip(s.pang, s.names)):
        bins[i] = extra.get(i)
        if bins[i] is None:
            bins[i] = int(round(float(a) / 30.0))
    hist = [0] * 30
    for i, b in bins.items():
        if s.expected[i] in (M, R):
            hist[b] += 1
    kept = ref.three_maxima(hist)
    for i, b in bins.items():
        if s.expected[i] in (M, R):
            s.expected[i] = M if (b in kept or not check_ori) else R
    return s.build(hist=hist if check_ori else None, kept=kept if check_ori else None, bins=extra if check_ori else {}, **claims)


def frame_rotation_third():
    """Bins with 20, 5 and 2 matches: the third == 0.1f * max1 is kept."""
    s, site, kept, extra = _rotation(True, (20, 5, 2), seed=112)
    return _finish_rotation(s, True, extra, third_kept=True)


def frame_rotation_third_cut():
    """Bins with 20, 5 and 1 matches: the third is cut, and a second below the cut (20, 1, 1) cuts both."""
    s, site, kept, extra = _rotation(True, (20, 5, 1), seed=113)
    return _finish_rotation(s, True, extra)


def frame_rotation_second_cut():
    s, site, kept, extra = _rotation(True, (20, 1, 1), seed=114)
    return _finish_rotation(s, True, extra)


frame_rotation_second_cut.__doc__ = "Bins with 20, 1 and 1 matches: the second is below 0.1f * max1, both are cut."


def frame_rotation_ties():
    """Four bins with 3 matches each: the first three win, the fourth is cut (every comparison is strict)."""
    s = FrameScene(115, th=3)
    site = sites()
    for b in (2, 4, 6, 9):
        for q in range(3):
            s.pair(f"bin {b} #{q}", *next(site), ang=30.0 * b, expect=R if b == 9 else M)
    return s.build(hist=[3 if b in (2, 4, 6, 9) else 0 for b in range(30)], kept=(2, 4, 6))


def frame_rotation_off():
    """The rotation group with checkOri = False: nothing is removed."""
    return frame_rotation(False)


def _tiled_chains(s, rows, n=40, step=10.0, x0=100.0, y0=20.0, dy=8.0):
    for r in range(rows):
        chain(s, x0, y0 + dy * r, n=n, step=step)


def frame_large_work():
    """53 chains of 40 points and a top-8 exhaustion: more than the 2,048 affected points the rounds hold in
    registers (the work list is then read from memory, the eight best from the per-point table).  2,120 points and keypoints."""
    s = FrameScene(116, th=3)
    _tiled_chains(s, 53, step=5.0, dy=4.0)
    rank = exhaustion(s, 500.0, 300.0, 12, 9, "12 usable, 9 best taken")
    return s.build(rounds_needed=40, affected_gt=2048, exhaustion=rank)


MOTIF = 26


def _contested(s, y=40.0):
    """A small contested motif (MOTIF keypoints): a 12-point chain, a top-8 exhaustion, a same-best pair and a
    blocked unobserved point.  th = 3."""
    chain(s, 100.0, y, n=12, step=5.0)
    s.claims["exhaustion"] = exhaustion(s, 400.0, y, 12, 9, "12 usable, 9 best taken")
    d = s.rand_desc()
    a, b = s.kp(300.0, y, desc=flip(d, 10)), s.kp(302.0, y, desc=flip(d, 20))
    s.pt("same best: first", 301.0, y, M, match=a, desc=d, Z=2.0)
    s.pt("same best: second", 301.0, y, M, match=b, desc=d, Z=4.0)
    s.pt("unobserved third: both held", 301.0, y, ref.NO_CANDIDATE, desc=d, Z=8.0, observed=0)


def frame_large_16385():
    """The contested motif in a frame of 16,385 keypoints, at the highest indices: the claims leave LDS."""
    s = FrameScene(117, th=3)
    s.clutter(16385 - MOTIF)
    _contested(s)
    assert len(s.kps) == 16385
    return s.build(n_cur=16385, motif_last=True)


def frame_large_65537():
    """The same in a frame of 65,537 keypoints: keypoint indices no longer fit the packed 16 bits."""
    s = FrameScene(118, th=3)
    s.clutter(65537 - MOTIF)
    _contested(s)
    assert len(s.kps) == 65537
    return s.build(n_cur=65537, motif_last=True)


def frame_prep_8193():
    """The contested motif in a frame of 8,193 keypoints (the device grid's cell lists leave LDS), clutter
    and motif interleaved so that cells hold non-consecutive indices."""
    s = FrameScene(119, th=3)
    s.clutter(4000)
    _contested(s)
    s.clutter(4000, y0=150.0, y1=470.0)
    s.pair("late keypoint", 500.0, 40.0)
    s.clutter(8193 - len(s.kps))
    assert len(s.kps) == 8193
    return s.build(n_cur=8193)


# ---- SearchByProjection(Frame, local map points) ---------------------------------------------------

def lpair(s, name, x, y, expect=M, dist=10, octave=0, **kw):
    d = s.rand_desc()
    j = s.kp(x, y, octave=octave, desc=flip(d, dist))
    return s.pt(name, x, y, expect, match=j if expect == M else None, desc=d, **kw), j


def local_gates(far=True):
    """track_in_view = 0, is_bad, depth == th_far kept and the next float above dropped (far points on); with
    far points off nothing is dropped for depth.  5 points."""
    s = LocalScene(201, far=far, th_far=8.0)
    site = sites()
    lpair(s, "in view", *next(site))
    lpair(s, "track_in_view=0", *next(site), expect=ref.NOT_IN_VIEW, in_view=0)
    lpair(s, "is_bad", *next(site), expect=ref.BAD, bad=1)
    lpair(s, "depth == th_far", *next(site), depth=8.0)
    lpair(s, "depth just above th_far", *next(site), expect=ref.FAR if far else M, depth=up(8.0))
    return s.build()


def local_gates_far_off():
    """The gates with far points off."""
    return local_gates(False)


def local_radius(th=1):
    """RadiusByViewingCos: track_view_cos == float(0.998) is above the double 0.998 -> 2.5, the next float
    below -> 4.0; th == 1 does not multiply; level 0 allows only octave 0, level 7 octaves 6 and 7; strict
    radius edges and the u_R gate against track_proj[2].  About 30 points."""
    s = LocalScene(202 + th, th=th)
    site = sites()
    c998 = f32(0.998)
    assert float(c998) > 0.998 > float(down(c998))
    r25, r40 = float(f32(f32(2.5) * f32(th)) if th != 1 else f32(2.5)), float(f32(f32(4.0) * f32(th)) if th != 1 else f32(4.0))
    for name, cos, r, dx, ok in (("cos == float(0.998): 2.5, dx == 2.5 r", c998, r25, 1.0, False),
                                 ("cos == float(0.998): 2.5, just inside", c998, r25, "in", True),
                                 ("cos just below: 4.0, dx between", down(c998), r40, 0.8, True),
                                 ("cos just below: 4.0, dx == 4.0 r", down(c998), r40, 1.0, False),
                                 ("cos just below: 4.0, just inside", down(c998), r40, "in", True)):
        x, y = next(site)
        if th != 1:
            x, y = next(site)
        d = s.rand_desc()
        kx = down(x + r) if dx == "in" else f32(x + r * dx)
        j = s.kp(kx, y, desc=flip(d, 10))
        s.pt(name, x, y, M if ok else ref.NO_CANDIDATE, match=j if ok else None, desc=d, cos=cos)
    for lvl in (0, 7):
        for ko in range(NLEVELS):
            x, y = next(site)
            if th != 1 or lvl == 7:
                x, y = next(site)
            ok = lvl - 1 <= ko <= lvl
            d = s.rand_desc()
            j = s.kp(x, y, octave=ko, desc=flip(d, 10))
            s.pt(f"level {lvl}, keypoint octave {ko}", x, y, M if ok else ref.NO_CANDIDATE, match=j if ok else None,
                 desc=d, level=lvl, cos=0.999)
    for name, kur, ok in (("uR == 0 bypasses", 0.0, True), ("uR == -1 bypasses", -1.0, True),
                          ("|xr - uR| == r passes", 50.0 + r40, True), ("|xr - uR| just above r fails", up(50.0 + r40), False)):
        x, y = next(site)
        if th != 1:
            x, y = next(site)
        d = s.rand_desc()
        j = s.kp(x, y, desc=flip(d, 10), ur=kur)
        s.pt(name, x, y, M if ok else ref.NO_CANDIDATE, match=j if ok else None, desc=d, xr=50.0)
    return s.build(radii=(r25, r40))


def local_radius_th3():
    """The radius group with th = 3: the radius is multiplied."""
    return local_radius(3)


def _two(s, x, y, name, b1, b2, expect, l1=0, l2=0, level=None):
    """A point with two candidates at distances b1 < b2 at octaves l1, l2."""
    d = s.rand_desc()
    j = s.kp(x - 1.0, y, octave=l1, desc=flip(d, b1))
    s.kp(x + 1.0, y, octave=l2, desc=flip(d, b2, 128))
    return s.pt(name, x, y, expect, match=j if expect == M else None, desc=d, level=max(l1, l2) if level is None else level)


def local_ratio(ratio=0.8):
    """b1 > ratio * b2 in float.  ratio 0.8: (40, 50) accepted, (41, 50) rejected; different levels skip the
    test; a single candidate (second 256, level -1) is accepted; two at the same distance and level are
    rejected.  6 points."""
    s = LocalScene(210, ratio=ratio)
    site = sites()
    cases = {0.8: ((40, 50, M), (41, 50, ref.RATIO)), 0.9: ((45, 50, M), (46, 50, ref.RATIO)),
             0.6: ((30, 50, M), (31, 50, ref.RATIO))}[ratio]
    for b1, b2, ex in cases:
        _two(s, *next(site), f"({b1}, {b2}) at ratio {ratio}", b1, b2, ex)
    _two(s, *next(site), "l1 != l2 skips the test", 49, 50, M, l1=1, l2=0)
    lpair(s, "single candidate", *next(site), dist=100)
    x, y = next(site)
    d = s.rand_desc()
    s.kp(x - 1.0, y, desc=flip(d, 30))
    s.kp(x + 1.0, y, desc=flip(d, 30, 128))
    s.pt("b2 == b1, same level", x, y, ref.RATIO, desc=d)
    lpair(s, "best == 100", *next(site), dist=100)
    lpair(s, "best == 101", *next(site), dist=101, expect=ref.ABOVE_TH_HIGH)
    return s.build()


def local_ratio_09():
    """ratio 0.9: the float product 0.9f * 50 (44.9999988 before rounding) rounds to 45.0f, so (45, 50) is
    accepted -- 45 > 45.0f is false -- and (46, 50) is rejected.  (In exact arithmetic 0.9f * 50 < 45 would
    reject it; the reference multiplies in float, and so do the oracle and the kernels.)"""
    return local_ratio(0.9)


def local_ratio_06():
    """ratio 0.6: (30, 50) is accepted (0.6f * 50 > 30), (31, 50) rejected."""
    return local_ratio(0.6)


def local_claims(observed_taker=True):
    """frame_taken keypoints are neither best nor second best; a second best claimed by an earlier observed
    point makes the ratio test pass that fails when that point is unobserved (both variants); the second
    best beyond the eight best: 10 usable at one level, 7 of the 8 best claimed, the true second best is the
    9th and (best, 9th) fails the ratio test; a 40-point chain whose neighbours alternate octaves, so the
    ratio test never applies.  About 60 points."""
    s = LocalScene(220 + int(observed_taker), th=1)
    site = sites()
    # frame_taken: the best and the would-be second best are held; the third alone is matched
    x, y = next(site)
    d = s.rand_desc()
    t1, t2 = s.kp(x - 1.0, y, desc=flip(d, 5)), s.kp(x + 1.0, y, desc=flip(d, 41, 100))
    j = s.kp(x, y + 1.0, desc=flip(d, 40, 50))
    s.taken += [t1, t2]
    s.pt("frame_taken best and second", x, y, M, match=j, desc=d)
    # second best claimed by an earlier point
    x, y = next(site)
    d = s.rand_desc()
    k1, k2 = s.kp(x - 1.0, y, desc=flip(d, 41)), s.kp(x + 1.0, y, desc=flip(d, 50, 128))
    s.pt("taker of the second best", x + 1.0, y, M, match=k2, desc=s.kdesc[k2], observed=int(observed_taker), level=0,
         cos=0.999)   # radius 2.5: sees only k2 (k1 is 2 px away... and at distance 91 from it)
    s.pt("second best claimed" if observed_taker else "second best assigned by an unobserved point", x, y,
         M if observed_taker else ref.RATIO, match=k1 if observed_taker else None, desc=d)
    # the second best beyond the top 8
    x, y = next(site)
    x, y = next(site)
    d = s.rand_desc()
    ks = [s.kp(x - 2.0 + 1.0 * (q % 5), y - 0.5 + 1.0 * (q // 5), desc=flip(d, 40 + q)) for q in range(10)]
    for q in range(1, 8):
        kx, ky = float(s.kps[ks[q]][0]), float(s.kps[ks[q]][1])
        s.pt(f"top 8: taker {q}", kx, ky, M, match=ks[q], desc=s.kdesc[ks[q]], cos=0.999)
    top = s.pt("second best is the 9th: (40, 48) fails", x, y, ref.RATIO, desc=d)
    # the chain: level-1 points, keypoints of alternating octaves 0 / 1, radius 4.8
    d = s.rand_desc()
    cy = 110.0
    ks = [s.kp(100.0 + 6.0 * i, cy, octave=i % 2, desc=flip(d, 10 + i)) for i in range(40)]
    for i in range(40):
        s.pt(f"chain point {i}", 100.0 + 6.0 * i - 3.0, cy, M, match=ks[i], desc=d, level=1)
    return s.build(rounds_needed=40, second_rank={top: 8})


def local_claims_unobserved():
    """The claims group with the taker of the second best unobserved: the ratio test then fails."""
    return local_claims(False)


def local_large_work():
    """53 chains of 40 local points: more than 2,048 affected points.  2,120 points and keypoints."""
    s = LocalScene(230, th=1)
    for r in range(53):
        d = s.rand_desc()
        cy = 20.0 + 5.0 * r
        ks = [s.kp(100.0 + 6.0 * i, cy, octave=i % 2, desc=flip(d, 10 + i)) for i in range(40)]
        for i in range(40):
            s.pt(f"chain {r} point {i}", 100.0 + 6.0 * i - 3.0, cy, M, match=ks[i], desc=d, level=1)
    return s.build(rounds_needed=40, affected_gt=2048)


FRAME_GROUPS = {f.__name__: f for f in (
    frame_gates, frame_grid, frame_window_walk, frame_candidates_default, frame_candidates_forward,
    frame_candidates_backward, frame_candidates_mono, frame_candidates_no_uright, frame_distance, frame_in_order,
    frame_rotation, frame_rotation_third, frame_rotation_third_cut, frame_rotation_second_cut, frame_rotation_ties,
    frame_rotation_off, frame_large_work, frame_large_16385, frame_large_65537, frame_prep_8193)}
LOCAL_GROUPS = {f.__name__: f for f in (
    local_gates, local_gates_far_off, local_radius, local_radius_th3, local_ratio, local_ratio_09, local_ratio_06,
    local_claims, local_claims_unobserved, local_large_work)}
GROUPS = {**FRAME_GROUPS, **LOCAL_GROUPS}

_cache = {}


def group(name) -> Group:
    """The built group (built once; the arrays are not to be modified)."""
    if name not in _cache:
        _cache[name] = GROUPS[name]()
    return _cache[name]


_refs = {}


def reference(pkg, name):
    """(group, current frame, last frame or local map points, projection_ref result), computed once per
    session and shared by the tests; not to be modified."""
    if name not in _refs:
        g = group(name)
        C, p = pkg.Frame(**g.cur), g.params
        if g.kind == "frame":
            X = pkg.Frame(**g.last)
            r = ref.search_frame(C, X, p["th"], p["mono"], p["check_ori"])
        else:
            X = pkg.LocalMapPoints(**g.points)
            r = ref.search_local(C, X, p["th"], p["far"], p["th_far"], p["ratio"], p["taken"])
        _refs[name] = (g, C, X, r)
    return _refs[name]
