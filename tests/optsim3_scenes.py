"""Problems for OptimizeSim3 (tests/test_optsim3_ref_cpu.py, tests/test_optsim3_gpu.py): hand-built ones with
every classification far from th2, and one seeded batch with noise and wrong pairs.  A problem is the dict
tests/optsim3_ref.py takes (the fields of orb_optsim3_problem_t).

Geometry: points 2-8 m in front of camera 2 over the EuRoC image, P3D1c = float32(S12 P3D2c) as the reference's
float32 gather leaves it (so "exact" data carry ~1e-4 px of rounding, chi2 ~1e-8), obs1 / obs2 the pixel
projections, th2 = 10 as LoopClosing passes it.  The start is the truth left-multiplied by a few degrees and
centimetres (and a few per cent of scale when it is free).
"""
from __future__ import annotations

import functools

import numpy as np

import optsim3_ref as ref

f32 = np.float32
CAM = (458.654, 457.296, 367.215, 248.375)
TH2 = 10.0
SCALE_FACTOR = 1.2
ROOM = 1024          # ORB_OPTSIM3_MAX_PAIRS


def inv_sigma2(level):
    return (f32(1.0) / (f32(SCALE_FACTOR) ** (2 * np.asarray(level))).astype(f32)).astype(f32)


def truth(scale=1.0):
    return ref.Sim3.exp(np.array([0.10, -0.25, 0.05, 0.4, -0.1, 0.2, 0.0])) * ref.Sim3([0, 0, 0, 1], [0, 0, 0], scale)


def make(n, seed, *, fix_scale, scale=1.0, noise=0.0, wrong=(), wrong_px=40.0, normalised=(), levels=None,
         start=(0.03, -0.04, 0.02, 0.03, -0.02, 0.04, 0.03)):
    """wrong: indices whose obs1 is moved by +-wrong_px in both coordinates; normalised: indices that follow the
    i2 < 0 rule (obs2 = float32 (x / z, y / z) of P3D2c, information mvInvLevelSigma2[0] = 1)."""
    rng = np.random.default_rng(seed)
    S = truth(scale)
    z = rng.uniform(2.0, 8.0, n)
    u, v = rng.uniform(40, 712, n), rng.uniform(40, 440, n)
    p2 = np.stack([(u - CAM[2]) * z / CAM[0], (v - CAM[3]) * z / CAM[1], z], 1).astype(f32).astype(np.float64)
    p1 = S.map(p2).reshape(n, 3).astype(f32).astype(np.float64)
    lv = rng.integers(0, 8, n) if levels is None else np.full(n, levels)
    sig = SCALE_FACTOR ** lv.astype(np.float64)
    obs1 = ref.project(CAM, S.map(p2).reshape(n, 3)) + noise * sig[:, None] * rng.normal(size=(n, 2))
    lv2 = rng.integers(0, 8, n) if levels is None else np.full(n, levels)
    obs2 = ref.project(CAM, p2) + noise * (SCALE_FACTOR ** lv2.astype(np.float64))[:, None] * rng.normal(size=(n, 2))
    obs1, obs2 = obs1.astype(f32).astype(np.float64), obs2.astype(f32).astype(np.float64)   # cv::Point2f
    is1, is2 = inv_sigma2(lv), inv_sigma2(lv2)
    for i in wrong:
        obs1[i] += wrong_px * rng.choice([-1.0, 1.0], 2)
    for i in normalised:
        invz = f32(1) / f32(p2[i, 2])
        obs2[i] = [f32(p2[i, 0]) * invz, f32(p2[i, 1]) * invz]
        is2[i] = inv_sigma2(0)
    upd = np.array(start, np.float64)
    if fix_scale:
        upd[6] = 0.0
    s0 = ref.Sim3.exp(upd) * S
    return {"p1c": p1, "p2c": p2, "obs1": obs1, "obs2": obs2, "inv_sigma2_1": is1, "inv_sigma2_2": is2, "cam1": CAM,
            "cam2": CAM, "s12": s0.vector(), "th2": TH2, "fix_scale": fix_scale, "truth": S.vector()}


HAND = {
    "exact_fixed": lambda: make(60, 1, fix_scale=True),                                   # nBad == 0: 5 more
    "exact_free_scale_1p3": lambda: make(60, 2, fix_scale=False, scale=1.3 * np.exp(-0.03)),   # starts at s = 1.3
    "wrong_pairs": lambda: make(60, 3, fix_scale=True, wrong=range(0, 60, 10)),          # nBad == 6: 10 more
    "wrong_pairs_free": lambda: make(80, 4, fix_scale=False, wrong=range(3, 80, 9)),
    "left_9": lambda: make(14, 5, fix_scale=True, wrong=(1, 4, 7, 10, 13)),               # the < 10 exit
    "left_10": lambda: make(15, 6, fix_scale=True, wrong=(1, 4, 7, 10, 13)),
    "i2_negative": lambda: make(40, 7, fix_scale=True, normalised=range(2, 40, 5)),       # 8 pairs by the i2 < 0 rule
    "room": lambda: make(ROOM, 8, fix_scale=False, wrong=range(0, ROOM, 16)),
}
for _n in (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257):
    HAND[f"n_{_n}"] = functools.partial(make, _n, 100 + _n, fix_scale=bool(_n & 1))

BATCH_SEED = 20
BATCH_SIZE = 12


def batch(seed=BATCH_SEED):
    """12 problems of 40-300 pairs: 1 px noise scaled by level, 10 % wrong pairs at +-20 px, mixed fix_scale."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(BATCH_SIZE):
        n = int(rng.integers(40, 301))
        wrong = rng.choice(n, n // 10, replace=False)
        out.append(make(n, int(rng.integers(1 << 30)), fix_scale=bool(k & 1), scale=1.0 if k & 1 else 1.1, noise=1.0,
                        wrong=wrong, wrong_px=20.0))
    return out


@functools.lru_cache(maxsize=None)
def hand(name):
    """(problem, restatement result), computed once and shared."""
    p = HAND[name]()
    return p, ref.optimize_sim3(p)


@functools.lru_cache(maxsize=None)
def batch_results():
    ps = batch()
    return ps, [ref.optimize_sim3(p) for p in ps]
