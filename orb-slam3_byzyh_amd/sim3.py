"""Sim3Solver's RANSAC (reference src/Sim3Solver.cc) over orb_sim3_ransac / orb_sim3_ransac_device: every
hypothesis of every loop-closing candidate in one call.

    problems = [Sim3Problem(x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, fix_scale, min_inliers, samples), ...]
    results = Sim3Solver(problems).run()          # one dict per problem

numpy arrays take the host form, torch tensors on the GPU the device form (no host hop; the results are
torch tensors on the same device, the call is asynchronous on the current stream).  The sample triples are an
input: draw_samples() reproduces the reference's swap-with-back scheme for the caller's integer generator.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib

MAX_HYPOTHESES = 1024


def ransac_max_its(n: int, probability: float = 0.99, min_inliers: int = 6, max_its: int = 300):
    """mRansacMaxIts as Sim3Solver::SetRansacParameters leaves it (:123-147, float epsilon), or None when
    n < min_inliers (iterate() then sets bNoMore without evaluating anything)."""
    if n < min_inliers:
        return None
    if min_inliers == n:
        its = 1
    else:
        eps = float(np.float32(min_inliers) / np.float32(n))
        its = int(math.ceil(math.log(1 - probability) / math.log(1 - eps ** 3)))
    return max(1, min(its, max_its))


def draw_samples(n: int, n_hyp: int, rng) -> np.ndarray:
    """[n_hyp, 3] int32: the triples Sim3Solver::iterate draws (:172-186).  rng(lo, hi) returns an integer in
    [lo, hi] (DUtils::Random::RandomInt); three calls per iteration, in order, each index taken out of the
    available list by overwriting it with the list's last entry."""
    out = np.empty((n_hyp, 3), np.int32)
    for h in range(n_hyp):
        avail = np.arange(n)
        size = n
        for k in range(3):
            r = int(rng(0, size - 1))
            out[h, k] = avail[r]
            avail[r] = avail[size - 1]
            size -= 1
    return out


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


class Sim3Problem:
    """What the Sim3Solver constructor gathers (:71-118) plus the draws: x3dc1 / x3dc2 [n, 3] float32
    (mvX3Dc1 / mvX3Dc2), max_err1 / max_err2 [n] float32 ((float)(9.210 * sigma2)), cam1 / cam2 (fx, fy, cx, cy;
    pinhole), samples [n_hyp, 3] int32.  All arrays numpy, or all torch tensors on one GPU."""

    def __init__(self, x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, fix_scale, min_inliers, samples):
        self.device = _is_torch(x3dc1)
        arrays = (x3dc1, x3dc2, max_err1, max_err2, samples)
        if any(_is_torch(a) != self.device for a in arrays):
            raise TypeError("Sim3Problem: numpy arrays or torch tensors, not a mixture")
        if self.device:
            import torch
            if any(not a.is_cuda for a in arrays):
                raise ValueError("Sim3Problem: torch tensors must live on the GPU")
            f = lambda a: a.to(torch.float32).contiguous()  # noqa: E731
            self.samples = samples.to(torch.int32).contiguous()
        else:
            f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
            self.samples = np.ascontiguousarray(samples, np.int32)
        self.x3dc1, self.x3dc2, self.max_err1, self.max_err2 = f(x3dc1), f(x3dc2), f(max_err1), f(max_err2)
        self.n = int(self.x3dc1.shape[0])
        self.n_hyp = int(self.samples.shape[0])
        if tuple(self.x3dc1.shape) != (self.n, 3) or tuple(self.x3dc2.shape) != (self.n, 3) or \
                tuple(self.max_err1.shape) != (self.n,) or tuple(self.max_err2.shape) != (self.n,) or \
                tuple(self.samples.shape) != (self.n_hyp, 3):
            raise ValueError("Sim3Problem: x3dc [n, 3], max_err [n], samples [n_hyp, 3]")
        self.cam1 = tuple(float(c) for c in cam1)
        self.cam2 = tuple(float(c) for c in cam2)
        if len(self.cam1) != 4 or len(self.cam2) != 4:
            raise ValueError("Sim3Problem: a camera is (fx, fy, cx, cy)")
        self.fix_scale, self.min_inliers = bool(fix_scale), int(min_inliers)


def _ptr(a):
    if a is None:
        return None
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


class Sim3Solver:
    """run(): one dict per problem with hyp_inliers [n_hyp], hyp_t12 [n_hyp, 12] (rows of [s R | t]), hyp_scale
    [n_hyp], winner (the first hypothesis with more than min_inliers inliers, or -1), best (the last hypothesis
    attaining the maximum count, or -1), inlier_mask [n] (of winner if there is one, else of best) and, with
    hyp_mask=True, hyp_mask [n_hyp, ceil(n / 64)] uint64 (bit i & 63 of word i >> 6: point i).  A problem with
    n < min_inliers is not evaluated: winner = best = -1 and its per-hypothesis arrays stay zero."""

    def __init__(self, problems):
        self.problems = [problems] if isinstance(problems, Sim3Problem) else list(problems)
        if any(p.device != self.problems[0].device for p in self.problems[1:]):
            raise TypeError("Sim3Solver: host and device problems cannot share a call")
        self.device = bool(self.problems) and self.problems[0].device

    def _alloc(self, p, hyp_mask):
        words = (p.n + 63) // 64
        shapes = {"hyp_inliers": ((p.n_hyp,), "int32"), "hyp_t12": ((p.n_hyp, 12), "float32"),
                  "hyp_scale": ((p.n_hyp,), "float32"), "winner": ((1,), "int32"), "best": ((1,), "int32"),
                  "inlier_mask": ((p.n,), "uint8")}
        if hyp_mask:
            shapes["hyp_mask"] = ((p.n_hyp, words), "uint64")
        if not self.device:
            return {k: np.zeros(s, d) for k, (s, d) in shapes.items()}
        import torch
        dev = p.x3dc1.device
        # (torch has no unsigned 64-bit arithmetic: the words travel as int64 with the same bits)
        return {k: torch.zeros(s, dtype=getattr(torch, "int64" if d == "uint64" else d), device=dev)
                for k, (s, d) in shapes.items()}

    def run(self, hyp_mask: bool = False, stream=None):
        lib = _lib.load()
        k = len(self.problems)
        if k == 0:
            _lib.check(lib.orb_sim3_ransac(None, 0, None), "orb_sim3_ransac")
            return []
        probs, outs = (_lib.Sim3Problem * k)(), (_lib.Sim3Out * k)()
        results = []
        for i, p in enumerate(self.problems):
            r = self._alloc(p, hyp_mask)
            results.append(r)
            probs[i] = _lib.Sim3Problem(p.n, _ptr(p.x3dc1), _ptr(p.x3dc2), _ptr(p.max_err1), _ptr(p.max_err2),
                                        (ctypes.c_float * 4)(*p.cam1), (ctypes.c_float * 4)(*p.cam2),
                                        int(p.fix_scale), p.min_inliers, p.n_hyp, _ptr(p.samples))
            outs[i] = _lib.Sim3Out(_ptr(r["hyp_inliers"]), _ptr(r["hyp_t12"]), _ptr(r["hyp_scale"]), _ptr(r["winner"]),
                                   _ptr(r["best"]), _ptr(r["inlier_mask"]), _ptr(r.get("hyp_mask")))
        if self.device:
            import torch
            if stream is None:
                stream = torch.cuda.current_stream(self.problems[0].x3dc1.device).cuda_stream
            _lib.check(lib.orb_sim3_ransac_device(probs, k, outs, ctypes.c_void_p(stream)), "orb_sim3_ransac_device")
        else:
            _lib.check(lib.orb_sim3_ransac(probs, k, outs), "orb_sim3_ransac")
            for r in results:
                r["winner"], r["best"] = int(r["winner"][0]), int(r["best"][0])
        return results
