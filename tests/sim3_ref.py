"""Python restatement of Sim3Solver's hypothesis evaluation and control flow (reference src/Sim3Solver.cc:
ComputeSim3 :311-412, CheckInliers :415-439, both iterate overloads :149-294, SetRansacParameters :123-147 and
the sampling of :172-186): what the tests of orb_sim3_ransac compare against.

  evaluate()   float64 on the float32 inputs.  Per hypothesis: T12 [s R | t], the scale and the relative gap
               (l1 - l2) / |l1| between the two largest eigenvalues of Horn's N (LAPACK's symmetric solver: not
               the kernel's Jacobi).  Per (hypothesis, point): the inlier bit and the relative margin
               min(|err1 - thr1| / thr1, |err2 - thr2| / thr2); a pair is *decisive* when that margin is
               > 1e-3.  The kernel projects in float32 with a transform rounded to float32: ~1e-4 px on a
               ~3 px threshold distance, a relative 1e-4 on the squared error, so outside the undecided set
               the kernel's bit is the float64 one.
  Replay       both iterate overloads over an array of per-hypothesis counts.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
DECISIVE = 1e-3


def max_err(sigma2):
    """mvnMaxError: (float)(9.210 * (double)sigma2) per correspondence."""
    return (9.210 * np.asarray(sigma2, f32).astype(np.float64)).astype(f32)


def project(X, cam):
    fx, fy, cx, cy = (float(c) for c in cam)
    return np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], -1)


def closed_form(x1, x2, samples, fix_scale):
    """Horn's closed form for every triple.  Returns T12 [H, 3, 4], T21 [H, 3, 4], scale [H], gap [H] (float64)."""
    P1 = np.asarray(x1, f32).astype(np.float64)[samples]      # [H, point, xyz]
    P2 = np.asarray(x2, f32).astype(np.float64)[samples]
    O1, O2 = P1.sum(1) / 3.0, P2.sum(1) / 3.0
    r1, r2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.einsum("hia,hib->hab", r2, r1)
    N = np.empty((len(samples), 4, 4))
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    N[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    N[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    N[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    for a in range(4):
        for b in range(a):
            N[:, a, b] = N[:, b, a]
    lam, vec = np.linalg.eigh(N)                              # ascending
    q = vec[:, :, 3]
    with np.errstate(all="ignore"):
        gap = (lam[:, 3] - lam[:, 2]) / np.abs(lam[:, 3])
        vn = np.linalg.norm(q[:, 1:], axis=1)
        ang = 2.0 * np.arctan2(vn, q[:, 0])
        ax = q[:, 1:] / vn[:, None]
        K = np.zeros((len(samples), 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ax[:, 2], ax[:, 1], -ax[:, 0]
        K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = ax[:, 2], -ax[:, 1], ax[:, 0]
        R = (np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K))
        P3 = np.einsum("hab,hib->hia", R, r2)
        s = np.ones(len(samples)) if fix_scale else (r1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))
        t = O1 - s[:, None] * np.einsum("hab,hb->ha", R, O2)
        T12 = np.concatenate([s[:, None, None] * R, t[:, :, None]], 2)
        Rinv = np.swapaxes(R, 1, 2) / s[:, None, None]
        T21 = np.concatenate([Rinv, -np.einsum("hab,hb->ha", Rinv, t)[:, :, None]], 2)
    return T12, T21, s, gap


def evaluate(prob):
    """prob: a dict with x3dc1, x3dc2 [n, 3] float32, max_err1, max_err2 [n] float32, cam1, cam2, fix_scale,
    samples [H, 3].  Returns a dict: bits [H, n] bool, margin [H, n], T12 [H, 12], scale [H], gap [H]."""
    x1, x2 = np.asarray(prob["x3dc1"], f32).astype(np.float64), np.asarray(prob["x3dc2"], f32).astype(np.float64)
    thr1, thr2 = np.asarray(prob["max_err1"], f32).astype(np.float64), np.asarray(prob["max_err2"], f32).astype(np.float64)
    T12, T21, s, gap = closed_form(prob["x3dc1"], prob["x3dc2"], np.asarray(prob["samples"]), prob["fix_scale"])
    im1, im2 = project(x1, prob["cam1"]), project(x2, prob["cam2"])
    with np.errstate(all="ignore"):
        X2in1 = np.einsum("hab,nb->hna", T12[:, :, :3], x2) + T12[:, None, :, 3]
        X1in2 = np.einsum("hab,nb->hna", T21[:, :, :3], x1) + T21[:, None, :, 3]
        err1 = ((im1[None] - project(X2in1, prob["cam1"])) ** 2).sum(-1)
        err2 = ((project(X1in2, prob["cam2"]) - im2[None]) ** 2).sum(-1)
        bits = (err1 < thr1[None]) & (err2 < thr2[None])
        margin = np.minimum(np.abs(err1 - thr1[None]) / thr1[None], np.abs(err2 - thr2[None]) / thr2[None])
    margin[np.isnan(margin)] = np.inf   # a non-finite transform: every comparison is false, whatever the rounding
    return {"bits": bits, "margin": margin, "T12": T12.reshape(len(T12), 12), "scale": s, "gap": gap}


def count_bounds(ev):
    """Per hypothesis: (decided inliers, undecided pairs).  The kernel's count lies in [lo, lo + und]."""
    und = ev["margin"] <= DECISIVE
    return (ev["bits"] & ~und).sum(1), und.sum(1)


def ransac_max_its(n, probability=0.99, min_inliers=6, max_its=300):
    """mRansacMaxIts after SetRansacParameters (:123-147), or None when n < min_inliers (iterate: bNoMore)."""
    if n < min_inliers:
        return None
    if min_inliers == n:
        its = 1
    else:
        eps = float(f32(min_inliers) / f32(n))                 # float epsilon
        its = int(math.ceil(math.log(1 - probability) / math.log(1 - eps ** 3)))
    return max(1, min(its, max_its))


def draw_samples(n, n_hyp, random_int):
    """The triples of n_hyp iterations (:172-186): random_int(lo, hi) is DUtils::Random::RandomInt."""
    out = np.zeros((n_hyp, 3), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        for k in range(3):
            r = random_int(0, len(avail) - 1)
            out[h, k] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


class Replay:
    """The control flow of Sim3Solver::iterate over per-hypothesis counts.  iterate(k) consumes the next k
    hypotheses and returns a dict: hyp (the hypothesis whose mT12i is returned, -1 for the identity / an unset
    bestSim3), no_more, n_inliers, converge."""

    def __init__(self, counts, n, min_inliers, max_its):
        self.counts, self.n, self.min_inliers, self.max_its = list(counts), n, min_inliers, max_its
        self.iterations, self.best_inliers, self.best = 0, 0, -1

    def iterate(self, n_iterations, with_converge=False):
        r = {"hyp": -1, "no_more": False, "n_inliers": 0, "converge": False}
        if self.n < self.min_inliers:
            r["no_more"] = True
            return r
        done, chunk_best = 0, -1
        while self.iterations < self.max_its and done < n_iterations:
            h = self.iterations
            done += 1
            self.iterations += 1
            c = self.counts[h]
            if c >= self.best_inliers:
                self.best_inliers, self.best = c, h
                if c > self.min_inliers:
                    r.update(hyp=h, n_inliers=c, converge=True)
                    return r
                chunk_best = h
        if self.iterations >= self.max_its:
            r["no_more"] = True
        if with_converge:
            r["hyp"] = chunk_best
        return r


def host_sim3():
    """csrc/orb_sim3_math.h compiled for the host (tests/native/sim3_host.cpp) as a ctypes library."""
    import ctypes
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parents[1]
    build = root / "build" / "tests"
    build.mkdir(parents=True, exist_ok=True)
    so = build / "libsim3_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror",
                    str(root / "tests" / "native" / "sim3_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.sim3_host_evaluate.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_void_p] * 4
    lib.sim3_host_evaluate.restype = None
    return lib


def host_evaluate(prob):
    """The kernel's per-lane arithmetic on the host: (T12 [H, 12] float32, scale [H] float32, bits [H, n] bool)."""
    lib = host_sim3()
    c = lambda a, d: np.ascontiguousarray(a, d)  # noqa: E731
    x1, x2, e1, e2 = (c(prob[k], f32) for k in ("x3dc1", "x3dc2", "max_err1", "max_err2"))
    cam1, cam2, smp = c(prob["cam1"], f32), c(prob["cam2"], f32), c(prob["samples"], np.int32)
    n, H = len(x1), len(smp)
    t12, scale, bits = np.zeros((H, 12), f32), np.zeros(H, f32), np.zeros((H, n), np.uint8)
    lib.sim3_host_evaluate(n, x1.ctypes.data, x2.ctypes.data, e1.ctypes.data, e2.ctypes.data, cam1.ctypes.data,
                           cam2.ctypes.data, int(prob["fix_scale"]), H, smp.ctypes.data, t12.ctypes.data,
                           scale.ctypes.data, bits.ctypes.data)
    return t12, scale, bits.astype(bool)
