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


class LoopBowKeyFrame:
    """What loop_bow_problems reads of a keyframe: mp_id [n] int32 (the feature's map point as an index into the
    pool, -1: NULL), kps (mvKeysUn: a KEYPOINT_DTYPE array, or a [n, 7] float32 CUDA tensor in the extractor's
    layout), level_sigma2 (mvLevelSigma2, host) and optionally obs_ok [n] uint8 (the point's
    GetIndexInKeyFrame(this keyframe) >= 0).  numpy arrays for the host form, CUDA tensors for the device form."""

    def __init__(self, mp_id, kps, level_sigma2, obs_ok=None):
        self.device = _is_torch(mp_id)
        if self.device:
            import torch
            self.mp_id = mp_id.to(torch.int32).contiguous()
            self.kps = kps.contiguous()
            self.obs_ok = None if obs_ok is None else obs_ok.to(torch.uint8).contiguous()
        else:
            self.mp_id = np.ascontiguousarray(mp_id, np.int32)
            self.kps = np.ascontiguousarray(kps, _lib.KEYPOINT_DTYPE)
            self.obs_ok = None if obs_ok is None else np.ascontiguousarray(obs_ok, np.uint8)
        self.n = int(self.mp_id.shape[0])
        if int(self.kps.shape[0]) != self.n or (self.obs_ok is not None and int(self.obs_ok.shape[0]) != self.n):
            raise ValueError("LoopBowKeyFrame: mp_id, kps and obs_ok hold one entry per feature")
        self.level_sigma2 = np.ascontiguousarray(level_sigma2, np.float32)
        if not 1 <= len(self.level_sigma2) <= 12:
            raise ValueError("LoopBowKeyFrame: 1 to 12 pyramid levels")

    def record(self) -> "_lib.LoopBowKf":
        s2 = (ctypes.c_float * 12)(*[float(x) for x in self.level_sigma2])
        return _lib.LoopBowKf(self.n, _ptr(self.mp_id), _ptr(self.kps), _ptr(self.obs_ok), len(self.level_sigma2), s2)


def loop_bow_problems(matcher, kf1: LoopBowKeyFrame, Tcw1, kfs2, group, Tcw2, xyz, matches12, ok1=None, bad=None,
                      pair_ok=None, stream=None):
    """The merge of the window's SearchByBoW matches (src/LoopClosing.cc:855-881) and the Sim3Solver constructor's
    gather (src/Sim3Solver.cc:71-118) for every candidate in one call (orb_loop_bow_problems[_device]; DESIGN.md
    section 4p).  kf1: the current keyframe, kfs2: the window keyframes candidate after candidate (LoopBowKeyFrame),
    group [n_cand + 1]: candidate c owns pairs group[c] .. group[c+1]-1, Tcw1 [3, 4] and Tcw2 [n_cand, 3, 4]: the poses
    of the current keyframe and of the candidates, xyz [n_points, 3] / bad [n_points]: the map-point pool,
    matches12 [n_pairs, C]: the rows of SearchByBoWKFMany / SearchByBoWKFDevice, ok1 [kf1.n] (None: from mp_id and
    bad), pair_ok [n_pairs] (host; 0: the window keyframe is NULL or bad).

    numpy arrays take the host form, CUDA tensors the device form (asynchronous on `stream`, the results are
    CUDA tensors).  Returns a dict: matched_point, matched_pair, idx1 [n_cand, C] int32, num_bow, n [n_cand] int32,
    x3dc1, x3dc2 [n_cand, C, 3] float32, max_err1, max_err2 [n_cand, C] float32; entry i < n[c] of row c is the
    reference's i-th correspondence."""
    lib = _lib.load()
    kfs2 = list(kfs2)
    device = _is_torch(matches12)
    if any(k.device != device for k in [kf1] + kfs2) or _is_torch(xyz) != device:
        raise TypeError("loop_bow_problems: numpy arrays or CUDA tensors, not a mixture")
    group = np.ascontiguousarray(group, np.int32)
    n_cand, n_pairs = len(group) - 1, len(kfs2)
    Tcw2 = np.ascontiguousarray(Tcw2, np.float32).reshape(max(n_cand, 0), 12)
    pok = None if pair_ok is None else np.ascontiguousarray(pair_ok, np.uint8)
    if pok is not None and len(pok) != n_pairs:
        raise ValueError("pair_ok: one flag per pair")
    if device:
        import torch
        i32 = lambda a: a.to(torch.int32).contiguous()  # noqa: E731
        u8 = lambda a: None if a is None else a.to(torch.uint8).contiguous()  # noqa: E731
        xyz = xyz.to(torch.float32).contiguous()
    else:
        i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)  # noqa: E731
        xyz = np.ascontiguousarray(xyz, np.float32)
    matches12, ok1, bad = i32(matches12), u8(ok1), u8(bad)
    C = int(matches12.shape[1]) if matches12.ndim == 2 else 0
    if matches12.ndim != 2 or int(matches12.shape[0]) < n_pairs or (ok1 is not None and int(ok1.shape[0]) < kf1.n) or \
            (bad is not None and int(bad.shape[0]) != int(xyz.shape[0])):
        raise ValueError("loop_bow_problems: matches12 [n_pairs, C], ok1 [kf1.n], bad [n_points]")
    shapes = {"matched_point": ((n_cand, C), "int32"), "matched_pair": ((n_cand, C), "int32"),
              "num_bow": ((n_cand,), "int32"), "n": ((n_cand,), "int32"), "idx1": ((n_cand, C), "int32"),
              "x3dc1": ((n_cand, C, 3), "float32"), "x3dc2": ((n_cand, C, 3), "float32"),
              "max_err1": ((n_cand, C), "float32"), "max_err2": ((n_cand, C), "float32")}
    if device:
        # (the library writes every element of all nine: no fill)
        res = {k: torch.empty(s, dtype=getattr(torch, d), device=matches12.device) for k, (s, d) in shapes.items()}
    else:
        res = {k: np.zeros(s, d) for k, (s, d) in shapes.items()}
    recs = (_lib.LoopBowKf * max(n_pairs, 1))(*[k.record() for k in kfs2])
    arg = _lib.LoopBowIn(kf1.record(), _ptr(ok1), (ctypes.c_float * 12)(*np.asarray(Tcw1, np.float32).reshape(12)),
                         n_pairs, n_cand, ctypes.cast(recs, ctypes.c_void_p), _ptr(pok), _ptr(group), _ptr(Tcw2),
                         int(xyz.shape[0]), _ptr(xyz), _ptr(bad), _ptr(matches12), C)
    out = _lib.LoopBowOut(*[_ptr(res[k]) for k in ("matched_point", "matched_pair", "num_bow", "n", "idx1", "x3dc1",
                                                   "x3dc2", "max_err1", "max_err2")])
    if device:
        if stream is None:
            stream = torch.cuda.current_stream(matches12.device).cuda_stream
        _lib.check(lib.orb_loop_bow_problems_device(matcher._handle(), ctypes.byref(arg), ctypes.byref(out),
                                                    ctypes.c_void_p(stream)), "orb_loop_bow_problems_device")
    else:
        _lib.check(lib.orb_loop_bow_problems(matcher._handle(), ctypes.byref(arg), ctypes.byref(out)),
                   "orb_loop_bow_problems")
    return res


def loop_bow_sim3_problems(res, n, samples, cam1, cams2, fix_scale, min_inliers):
    """The Sim3Problem records of loop_bow_problems' result, one per candidate, for Sim3Solver: n[c] (read back
    by the caller, who draws samples[c] [n_hyp, 3] from it), cam1 and cams2[c] (fx, fy, cx, cy of the current
    keyframe and of candidate c).  The arrays are views of `res`: nothing is copied."""
    return [Sim3Problem(res["x3dc1"][c, :int(n[c])], res["x3dc2"][c, :int(n[c])], res["max_err1"][c, :int(n[c])],
                        res["max_err2"][c, :int(n[c])], cam1, cams2[c], fix_scale, min_inliers, samples[c])
            for c in range(len(samples))]


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
