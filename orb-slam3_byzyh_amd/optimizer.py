"""Optimizer::LocalBundleAdjustment's solve on the MI355X (reference src/Optimizer.cc:1740-2188).

The reference gathers the local window from its map (B1, :1744-1855), builds a g2o graph, runs
optimizer.optimize(10) (:2101), then culls edges by chi2 / depth and writes the estimates back
(B10, :2107-2185).  This module takes the flattened graph (poses as g2o::SE3Quat vectors, points,
edges with their measurements, information and camera) and runs the g2o Levenberg-Marquardt /
Schur solve on the GPU through orb_ba_optimize (include/orbgpu.h).  `local_bundle_adjustment`
then applies the reference's culling thresholds (5.991 mono, 7.815 stereo) and reports the
observations LocalBundleAdjustment would erase.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check

CHI2_MONO = 5.991    # src/Optimizer.cc:2115
CHI2_STEREO = 7.815  # src/Optimizer.cc:2145

_p = ctypes.c_void_p


class BaProblem(ctypes.Structure):
    _fields_ = [("n_poses", ctypes.c_int32), ("n_points", ctypes.c_int32), ("n_edges", ctypes.c_int32),
                ("pose", _p), ("pose_id", _p), ("pose_fixed", _p), ("pose_camera", _p), ("point", _p),
                ("point_id", _p), ("edges", _p)]


class BaOptions(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("user_lambda_init", ctypes.c_double), ("stop_flag", _p), ("stop_flag_bool", _p)]


class BaResult(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("trials", ctypes.c_int32), ("terminated", ctypes.c_int32),
                ("stopped", ctypes.c_int32), ("initial_chi2", ctypes.c_double), ("final_chi2", ctypes.c_double),
                ("lambda_", ctypes.c_double)]

    def as_dict(self):
        return {"iterations": self.iterations, "trials": self.trials, "terminated": self.terminated,
                "stopped": self.stopped, "initial_chi2": self.initial_chi2, "final_chi2": self.final_chi2,
                "lambda": self.lambda_}


def make_problem_struct(prob: dict) -> tuple[BaProblem, dict]:
    """Contiguous copies of the problem arrays (pose and point are optimised in place) + the struct."""
    from .synth import BA_CAMERA_DTYPE, BA_EDGE_DTYPE
    arrs = {
        "pose": np.ascontiguousarray(prob["pose"], dtype=np.float64).copy(),
        "pose_id": np.ascontiguousarray(prob["pose_id"], dtype=np.int64),
        "pose_fixed": np.ascontiguousarray(prob["pose_fixed"], dtype=np.uint8),
        "pose_camera": np.ascontiguousarray(prob["pose_camera"], dtype=BA_CAMERA_DTYPE),
        "point": np.ascontiguousarray(prob["point"], dtype=np.float64).copy(),
        "point_id": np.ascontiguousarray(prob["point_id"], dtype=np.int64),
        "edges": np.ascontiguousarray(prob["edges"], dtype=BA_EDGE_DTYPE),
    }
    s = BaProblem(len(arrs["pose"]), len(arrs["point"]), len(arrs["edges"]), arrs["pose"].ctypes.data,
                  arrs["pose_id"].ctypes.data, arrs["pose_fixed"].ctypes.data, arrs["pose_camera"].ctypes.data,
                  arrs["point"].ctypes.data, arrs["point_id"].ctypes.data, arrs["edges"].ctypes.data)
    return s, arrs


def stop_flag_address(stop_flag):
    """Address the library polls for pbStopFlag, or None.  The flag must be memory the caller's
    other thread writes: a silent converting copy would never see the request, so anything other
    than a C-contiguous np.int32 array or a ctypes.c_int32 is rejected."""
    if stop_flag is None:
        return None
    if isinstance(stop_flag, ctypes.c_int32):
        return ctypes.addressof(stop_flag)
    if isinstance(stop_flag, np.ndarray):
        if stop_flag.dtype != np.int32 or not stop_flag.flags["C_CONTIGUOUS"] or stop_flag.size < 1:
            raise TypeError("stop_flag must be a non-empty C-contiguous np.int32 array")
        return stop_flag.ctypes.data
    raise TypeError(f"stop_flag must be an np.int32 array or ctypes.c_int32, not {type(stop_flag).__name__}")


# orb_ba_host_reduce_fn (include/orbgpu.h): in-place all-reduce of n doubles, op 0 = SUM, 1 = MAX
HOST_REDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t,
                                  ctypes.c_int)
BA_SUM, BA_MAX = 0, 1


def make_host_reducer(group=None):
    """An orb_ba_host_reduce_fn that all-reduces the library's host buffer with the group's own
    all_reduce (in place, float64).  Returns nonzero to the library when the collective raises."""
    import torch
    import torch.distributed as dist
    ops = {BA_SUM: dist.ReduceOp.SUM, BA_MAX: dist.ReduceOp.MAX}

    def reduce_cb(_ctx, buf, n, op):
        try:
            t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(n,)))
            dist.all_reduce(t, op=ops[op], group=group)
            return 0
        except Exception:  # noqa: BLE001 -- reported to the library as a failed collective
            return -1

    return HOST_REDUCE_FN(reduce_cb)


class LocalBA:
    """A device handle for repeated local BA solves (one per LocalMapping thread).

    attach() shards each solve's landmarks over the ranks of a torch.distributed group (DESIGN.md
    sec. 5): every rank passes the SAME problem; each builds the Schur complement of its landmark
    range and the partial systems are all-reduced (RCCL for an nccl group, the group's own
    all_reduce on host buffers for gloo).  Results are identical on every rank.
    """

    def __init__(self):
        lib = _lib.load()
        _lib.require_device()
        h = ctypes.c_void_p()
        check(lib.orb_ba_create(ctypes.byref(h)), "orb_ba_create")
        self._h = h
        self._lib = lib

    def attach(self, group=None, transport: str | None = None):
        """Join the ranks of `group` (default: the world group) for sharded solves.

        transport: "rccl" (device all-reduce inside the library, needs one GPU per rank) or "host"
        (the group's all_reduce on CPU tensors through a callback).  Default: "rccl" when the
        group's backend is nccl, else "host"."""
        import torch
        import torch.distributed as dist
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        if transport is None:
            transport = "rccl" if dist.get_backend(group) == "nccl" else "host"
        if transport == "rccl":
            uid = (ctypes.c_uint8 * 128)()
            if rank == 0:
                check(self._lib.orb_ba_dist_unique_id(uid), "orb_ba_dist_unique_id")
            box = [bytes(uid)]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0,
                                       group=group)
            uid = (ctypes.c_uint8 * 128).from_buffer_copy(box[0])
            check(self._lib.orb_ba_dist_init_rccl(self._h, uid, world, rank), "orb_ba_dist_init_rccl")
            self._reduce_cb = None
        elif transport == "host":
            self._reduce_cb = make_host_reducer(group)  # kept alive with the handle
            check(self._lib.orb_ba_dist_init_host(self._h, self._reduce_cb, None, world, rank),
                  "orb_ba_dist_init_host")
        else:
            raise ValueError(f"unknown transport {transport!r}")
        self.world, self.rank, self.transport = world, rank, transport
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.orb_ba_destroy(h)
            except Exception:
                pass
            self._h = None

    def optimize(self, prob: dict, iterations: int = 10, user_lambda_init: float = 0.0, stop_flag=None):
        """Run optimize(iterations) on a copy of `prob`.  Returns (pose, point, edge_chi2, depth_ok, result).

        stop_flag is the reference's pbStopFlag (sparse_optimizer.h:188): a C-contiguous np.int32
        array (element 0 is polled) or a ctypes.c_int32, shared with the thread that sets it."""
        s, arrs = make_problem_struct(prob)
        opt = BaOptions(int(iterations), float(user_lambda_init), stop_flag_address(stop_flag))
        ne = len(arrs["edges"])
        chi2 = np.zeros(ne, np.float64)
        depth = np.zeros(ne, np.uint8)
        res = BaResult()
        rc = self._lib.orb_ba_optimize(self._h, ctypes.byref(s), ctypes.byref(opt), chi2.ctypes.data,
                                       depth.ctypes.data, ctypes.byref(res))
        if rc != _lib.ORB_ERR_ABORTED:
            check(rc, "orb_ba_optimize")
        return arrs["pose"], arrs["point"], chi2, depth.astype(bool), res.as_dict()


def local_bundle_adjustment(prob: dict, iterations: int = 10, solver: LocalBA | None = None):
    """optimize(10) and the reference's culling pass (src/Optimizer.cc:2107-2160): returns
    (pose, point, erase_mask over edges, result)."""
    import time
    lib = _lib.load()
    timed = lib.orb_timers_enabled() != 0  # REGISTER_TIMES "LBA": the whole call (src/LocalMapping.cc:208-219)
    t0 = time.perf_counter()
    solver = solver or LocalBA()
    pose, point, chi2, depth, res = solver.optimize(prob, iterations)
    stereo = np.asarray(prob["edges"]["stereo"]) != 0
    erase = np.where(stereo, chi2 > CHI2_STEREO, chi2 > CHI2_MONO) | ~depth
    if timed:
        check(lib.orb_timer_add(b"LBA", (time.perf_counter() - t0) * 1e3), "orb_timer_add")
    return pose, point, erase, res


def pose_optimization(frames, edges):
    """Optimizer::PoseOptimization (src/Optimizer.cc:55-415) on a batch of frames, on the GPU.

    frames: POSE_FRAME_DTYPE records (Tcw as SE3Quat vector, camera, the frame's edge range);
    edges: POSE_EDGE_DTYPE records (MapPoint position, observation, information, stereo flag).
    Returns (poses [n, 7], mvbOutlier per edge (bool), inliers per frame = the reference's return
    value).  The reference's Frame writes (SetPose, mvbOutlier) are the caller's."""
    from ._lib import POSE_EDGE_DTYPE, POSE_FRAME_DTYPE
    fr = np.ascontiguousarray(frames, POSE_FRAME_DTYPE)
    ed = np.ascontiguousarray(edges, POSE_EDGE_DTYPE)
    poses = np.zeros((len(fr), 7), np.float64)
    outl = np.zeros(max(len(ed), 1), np.uint8)
    inl = np.zeros(max(len(fr), 1), np.int32)
    check(_lib.load().orb_pose_optimization(len(fr), fr.ctypes.data, len(ed), ed.ctypes.data, poses.ctypes.data,
                                            outl.ctypes.data, inl.ctypes.data), "orb_pose_optimization")
    return poses, outl[:len(ed)].astype(bool), inl[:len(fr)]


OPTSIM3_MAX_PAIRS = 1024  # ORB_OPTSIM3_MAX_PAIRS


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def optimize_sim3(problems, chi2: bool = False, stream=None):
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:4195-4494) on a batch of gathered loop / merge candidates, on the
    GPU (orb_optimize_sim3 / orb_optimize_sim3_device).

    problems: a list of dicts with p1c, p2c [n, 3] and obs1, obs2 [n, 2] (float64), inv_sigma2_1, inv_sigma2_2 [n]
    (float32), cam1, cam2 (fx, fy, cx, cy; pinhole), s12 (8 doubles: qx qy qz qw tx ty tz s), th2, fix_scale.
    n is at most OPTSIM3_MAX_PAIRS.  The six arrays are numpy (the host form, synchronous) or torch tensors on one
    GPU (the device form: no host hop, asynchronous on the current stream or `stream`; the results are tensors).

    Returns one dict per problem: s12 [8] (the input when the reference returns 0 through its < 10 exit), n_in
    (the reference's return value), n_bad (the first cull's), inlier [n] (where vpMatches1 stays set) and, with
    chi2=True, chi2_12 / chi2_21 [n]."""
    lib = _lib.load()
    problems = list(problems)
    k = len(problems)
    if k == 0:
        check(lib.orb_optimize_sim3(None, 0, None), "orb_optimize_sim3")
        return []
    keys = ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")
    device = _is_torch(problems[0]["p1c"])
    if any(_is_torch(p[key]) != device for p in problems for key in keys):
        raise TypeError("optimize_sim3: numpy arrays or torch tensors, not a mixture")
    probs, outs = (_lib.OptSim3Problem * k)(), (_lib.OptSim3Out * k)()
    keep, results = [], []
    if device:
        import torch
    for i, p in enumerate(problems):
        if device:
            if any(not p[key].is_cuda for key in keys):
                raise ValueError("optimize_sim3: torch tensors must live on the GPU")
            a = [p[key].to(torch.float64 if j < 4 else torch.float32).contiguous() for j, key in enumerate(keys)]
            dev = a[0].device
            new = lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device=dev)  # noqa: E731
            ptr = lambda t: t.data_ptr()  # noqa: E731
        else:
            a = [np.ascontiguousarray(p[key], np.float64 if j < 4 else np.float32) for j, key in enumerate(keys)]
            new = lambda shape, dt: np.zeros(shape, dt)  # noqa: E731
            ptr = lambda t: t.ctypes.data  # noqa: E731
        n = int(a[0].shape[0])
        shapes = [(n, 3), (n, 3), (n, 2), (n, 2), (n,), (n,)]
        if any(tuple(t.shape) != s for t, s in zip(a, shapes)):
            raise ValueError("optimize_sim3: p1c / p2c [n, 3], obs1 / obs2 [n, 2], inv_sigma2 [n]")
        cam1, cam2 = [float(c) for c in p["cam1"]], [float(c) for c in p["cam2"]]
        s12 = [float(v) for v in p["s12"]]
        if len(cam1) != 4 or len(cam2) != 4 or len(s12) != 8:
            raise ValueError("optimize_sim3: a camera is (fx, fy, cx, cy), s12 is qx qy qz qw tx ty tz s")
        r = {"s12": new((8,), "float64"), "n_in": new((1,), "int32"), "n_bad": new((1,), "int32"),
             "inlier": new((max(n, 1),), "uint8")}
        if chi2:
            r["chi2_12"], r["chi2_21"] = new((max(n, 1),), "float64"), new((max(n, 1),), "float64")
        probs[i] = _lib.OptSim3Problem(n, *[ptr(t) for t in a], (ctypes.c_float * 4)(*cam1), (ctypes.c_float * 4)(*cam2),
                                       (ctypes.c_double * 8)(*s12), float(p["th2"]), int(bool(p["fix_scale"])))
        outs[i] = _lib.OptSim3Out(ptr(r["s12"]), ptr(r["n_in"]), ptr(r["n_bad"]), ptr(r["inlier"]),
                                  ptr(r["chi2_12"]) if chi2 else None, ptr(r["chi2_21"]) if chi2 else None)
        keep.append(a)
        for key in ("inlier", "chi2_12", "chi2_21"):
            if key in r:
                r[key] = r[key][:n]
        results.append(r)
    if device:
        if stream is None:
            stream = torch.cuda.current_stream(keep[0][0].device).cuda_stream
        check(lib.orb_optimize_sim3_device(probs, k, outs, ctypes.c_void_p(stream)), "orb_optimize_sim3_device")
        for r, a in zip(results, keep):
            r["_inputs"] = a  # the call is asynchronous: the converted inputs live as long as the results
    else:
        check(lib.orb_optimize_sim3(probs, k, outs), "orb_optimize_sim3")
        for r in results:
            r["n_in"], r["n_bad"], r["inlier"] = int(r["n_in"][0]), int(r["n_bad"][0]), r["inlier"].astype(bool)
    return results
