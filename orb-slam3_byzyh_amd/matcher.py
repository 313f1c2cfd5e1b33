"""ORBmatcher with the reference's interface (include/ORBmatcher.h), HIP-backed."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check
from .keyframe import (NEWPOINT_DTYPE, DeviceKeyFrame, Frame, FuseKfView, FusePoints, FusePointsView, KeyFrame,
                       KfDeviceView, KfView, LocalMapPoints, NewPointsKf, NewPointsKfDevice, NewPointsOut,
                       NewPointsParams, PairGeom, Sim3ProjJob, Sim3ProjKfView)

TH_HIGH = 100  # src/ORBmatcher.cc:36
TH_LOW = 50    # src/ORBmatcher.cc:37
HISTO_LENGTH = 30  # src/ORBmatcher.cc:38
# the modes of a SearchByProjectionSim3 job (ORB_S3P_* of include/orbgpu.h)
ORB_S3P_CLAIM_PROJECT, ORB_S3P_CLAIM_INVZ, ORB_S3P_FUSE = 0, 1, 2


def sim3_pose(R, t, s):
    """(Tcw [3, 4], Ow [3]) in float32 of a Sim3 (R, t, s) as loop closing's searches decompose it
    (src/ORBmatcher.cc:508-509): Tcw = [R | t / s], Ow = -R^T (t / s).  For tests and callers without Sophus; a
    C++ caller runs the reference's two Sophus lines (GpuORBmatcher's adapter)."""
    R = np.asarray(R, np.float32).reshape(3, 3)
    ts = (np.asarray(t, np.float32).reshape(3) / np.float32(s)).astype(np.float32)
    Ow = -(R.T @ ts).astype(np.float32)
    return np.concatenate([R, ts[:, None]], axis=1).astype(np.float32), Ow.astype(np.float32)


class ORBmatcher:
    TH_HIGH = TH_HIGH
    TH_LOW = TH_LOW
    HISTO_LENGTH = HISTO_LENGTH

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self._h = None

    def _handle(self):
        if self._h is None:
            lib = _lib.load()
            h = ctypes.c_void_p()
            check(lib.orb_matcher_create(self.mfNNratio, int(self.mbCheckOrientation), ctypes.byref(h)),
                  "orb_matcher_create")
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().orb_matcher_destroy(h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def pair_geometry(pKF1: KeyFrame, pKF2: KeyFrame) -> PairGeom:
        """R12, t12 of T12 = T1w * Tw2 and the epipole of KF1's centre in KF2 (src/ORBmatcher.cc:1063-1090)."""
        g = PairGeom()
        check(_lib.load().orb_kf_pair_geometry(pKF1.Tcw.ctypes.data, pKF2.Tcw.ctypes.data, pKF2.fx, pKF2.fy,
                                               pKF2.cx, pKF2.cy, ctypes.byref(g)), "orb_kf_pair_geometry")
        return g

    def SearchForTriangulation(self, pKF1: KeyFrame, pKF2: KeyFrame, bOnlyStereo: bool, bCoarse: bool = False):
        """src/ORBmatcher.cc:1046-1324.  Returns (nmatches, vMatchedPairs as a list of (idx1, idx2))."""
        (n, m12), = self.SearchForTriangulationMany(pKF1, [pKF2], bOnlyStereo, bCoarse)
        pairs = [(int(i), int(m12[i])) for i in np.flatnonzero(m12 >= 0)]
        return n, pairs

    def SearchForTriangulationMany(self, pKF1: KeyFrame, neighbours, bOnlyStereo: bool, bCoarse: bool = False,
                                   geoms=None):
        """SearchForTriangulation of pKF1 against every keyframe in `neighbours` in one device launch
        (the loop of LocalMapping::CreateNewMapPoints).  Returns [(nmatches, vMatches12 int32[N1])]."""
        neighbours = list(neighbours)
        p = len(neighbours)
        if p == 0:
            return []
        views = (KfView * p)(*[k.view() for k in neighbours])
        if geoms is None:
            geoms = [self.pair_geometry(pKF1, k) for k in neighbours]
        garr = (PairGeom * p)(*geoms)
        m12 = np.full((p, max(pKF1.N, 1)), -1, np.int32)
        cnt = np.zeros(p, np.int32)
        check(_lib.load().orb_search_for_triangulation(self._handle(), ctypes.byref(pKF1.view()), views, garr, p,
                                                       int(bOnlyStereo), int(bCoarse), m12.ctypes.data,
                                                       cnt.ctypes.data), "orb_search_for_triangulation")
        return [(int(cnt[i]), m12[i, :pKF1.N]) for i in range(p)]

    def SearchForTriangulationDevice(self, pKF1: DeviceKeyFrame, neighbours, bOnlyStereo: bool, bCoarse: bool = False,
                                     stream=None, out=None):
        """SearchForTriangulation of a device-resident keyframe against device-resident neighbours
        (orb_search_for_triangulation_device): no host hop for features, stereo depths or FeatureVectors.
        Returns (matches12 [P, cap1] int32, counts [P] int32) CUDA tensors, asynchronous on `stream`."""
        return self.SearchForTriangulationDeviceBatch([(pKF1, list(neighbours))], bOnlyStereo, bCoarse, stream, out)

    def SearchForTriangulationDeviceBatch(self, groups, bOnlyStereo: bool, bCoarse: bool = False, stream=None, out=None,
                                          prepared=None):
        """Several new keyframes, each with its neighbours, in one launch: groups = [(kf1, [kf2, ...]), ...].
        Returns (matches12 [P, C] int32, counts [P] int32), pairs in group order, C = max cap of the kf1s.
        `prepared` (from prepare_device_batch) reuses the ctypes arrays of an identical earlier call."""
        import torch
        if prepared is None:
            prepared = self.prepare_device_batch(groups)
        kf1v, n1, kf2v, k1, geoms, n_pairs, C, dev = prepared
        if out is None:
            out = (torch.empty((max(n_pairs, 1), C), dtype=torch.int32, device=dev),
                   torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev))
        if n_pairs == 0:
            return out
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_search_for_triangulation_device(self._handle(), kf1v, n1, kf2v, k1, geoms, n_pairs,
                                                              int(bOnlyStereo), int(bCoarse), out[0].data_ptr(),
                                                              out[1].data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_search_for_triangulation_device")
        return out

    def prepare_device_batch(self, groups):
        """The ctypes arguments of SearchForTriangulationDeviceBatch for `groups` (views, pair table, geometry)."""
        groups = [(k1, list(nb)) for k1, nb in groups]
        n1 = len(groups)
        kf1v = (KfDeviceView * max(n1, 1))(*[g[0].view() for g in groups])
        pairs = [(i, k2) for i, (_, nb) in enumerate(groups) for k2 in nb]
        n_pairs = len(pairs)
        kf2v = (KfDeviceView * max(n_pairs, 1))(*[k2.view() for _, k2 in pairs])
        k1 = (ctypes.c_int32 * max(n_pairs, 1))(*[i for i, _ in pairs])
        geoms = (PairGeom * max(n_pairs, 1))(*[self.pair_geometry(groups[i][0], k2) for i, k2 in pairs])
        C = max(g[0].cap for g in groups)
        return kf1v, n1, kf2v, k1, geoms, n_pairs, C, groups[0][0]._keep[0].device

    def SearchByBoW(self, pKF: KeyFrame, F: KeyFrame, point_ok=None):
        """SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (src/ORBmatcher.cc:260-494),
        single camera.  F: the frame as a KeyFrame-shaped view (keypoints, descriptors, mFeatVec).  point_ok[i]:
        pKF's map point i is non-NULL and not isBad() (None: pKF.has_mappoint).  Returns (nmatches, match
        int32[F.N]) with match[iF] = the feature of pKF whose map point vpMapPointMatches[iF] receives (-1: NULL)."""
        (n, m), = self.SearchByBoWMany([pKF], F, None if point_ok is None else [point_ok])
        return n, m

    def SearchByBoWMany(self, kfs, F: KeyFrame, point_ok=None):
        """SearchByBoW of every keyframe in `kfs` against F in one device launch (the candidate loop of
        Tracking::Relocalization).  point_ok: per keyframe a flag array or None.  Returns [(nmatches, match)]."""
        kfs = list(kfs)
        p = len(kfs)
        if p == 0:
            return []
        views = (KfView * p)(*[k.view() for k in kfs])
        oks = [None] * p if point_ok is None else [None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
                                                   for a in point_ok]
        if len(oks) != p or any(a is not None and len(a) != k.N for a, k in zip(oks, kfs)):
            raise ValueError("point_ok: one array of pKF.N flags (or None) per keyframe")
        okp = (ctypes.c_void_p * p)(*[None if a is None else a.ctypes.data for a in oks])
        m = np.full((p, max(F.N, 1)), -1, np.int32)
        cnt = np.zeros(p, np.int32)
        check(_lib.load().orb_search_by_bow(self._handle(), views, okp, p, ctypes.byref(F.view()), m.ctypes.data,
                                            cnt.ctypes.data), "orb_search_by_bow")
        return [(int(cnt[i]), m[i, :F.N]) for i in range(p)]

    def SearchByBoWDevice(self, kfs, frames, point_ok=None, pair_frame=None, stream=None, out=None):
        """SearchByBoW on device-resident sides (orb_search_by_bow_device): pair p matches the DeviceKeyFrame
        kfs[p] against frames[pair_frame[p]] (a single DeviceKeyFrame or a list; pair_frame None: frames[0]).
        point_ok: per keyframe a uint8 CUDA tensor of cap flags or None (the keyframe's has_mappoint).
        Returns (match [P, C] int32, counts [P] int32) CUDA tensors, C = max cap of the frames; a side
        flagged ORB_ERR_CAPACITY gives that count.  Asynchronous on `stream`."""
        import torch
        kfs = list(kfs)
        frames = [frames] if isinstance(frames, DeviceKeyFrame) else list(frames)
        p, nf = len(kfs), len(frames)
        dev = frames[0]._keep[0].device
        C = max(f.cap for f in frames)
        if out is None:
            out = (torch.empty((max(p, 1), C), dtype=torch.int32, device=dev),
                   torch.empty(max(p, 1), dtype=torch.int32, device=dev))
        if p == 0:
            return out
        kv = (KfDeviceView * p)(*[k.view() for k in kfs])
        fv = (KfDeviceView * nf)(*[f.view() for f in frames])
        oks = [None] * p if point_ok is None else list(point_ok)
        okp = (ctypes.c_void_p * p)(*[None if a is None else a.data_ptr() for a in oks])
        pf = None if pair_frame is None else (ctypes.c_int32 * p)(*[int(i) for i in pair_frame])
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_search_by_bow_device(self._handle(), kv, okp, p, fv, nf, pf, out[0].data_ptr(),
                                                   out[1].data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_search_by_bow_device")
        return out

    def SearchByBoWKF(self, pKF1: KeyFrame, pKF2: KeyFrame, ok1=None, ok2=None):
        """SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (src/ORBmatcher.cc:893-1044),
        single camera.  ok1[i] / ok2[i]: the keyframe's map point i is non-NULL and not isBad() (None: its
        has_mappoint).  Returns (nmatches, matches12 int32[pKF1.N]) with matches12[idx1] = the feature of pKF2 whose
        map point vpMatches12[idx1] receives (-1: NULL)."""
        (n, m), = self.SearchByBoWKFMany(pKF1, [pKF2], ok1, None if ok2 is None else [ok2])
        return n, m

    def SearchByBoWKFMany(self, pKF1: KeyFrame, kfs2, ok1=None, ok2=None):
        """SearchByBoW of pKF1 against every keyframe in `kfs2` in one device launch (the window loop of
        LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:840-851).  ok2: per keyframe a flag array or
        None.  Returns [(nmatches, matches12)]."""
        kfs2 = list(kfs2)
        p = len(kfs2)
        if p == 0:
            return []
        views = (KfView * p)(*[k.view() for k in kfs2])
        a1 = None if ok1 is None else np.ascontiguousarray(ok1, dtype=np.uint8)
        oks = [None] * p if ok2 is None else [None if a is None else np.ascontiguousarray(a, dtype=np.uint8)
                                              for a in ok2]
        if (a1 is not None and len(a1) != pKF1.N) or len(oks) != p or \
                any(a is not None and len(a) != k.N for a, k in zip(oks, kfs2)):
            raise ValueError("ok1: pKF1.N flags; ok2: one array of pKF2.N flags (or None) per keyframe")
        okp = (ctypes.c_void_p * p)(*[None if a is None else a.ctypes.data for a in oks])
        m = np.full((p, max(pKF1.N, 1)), -1, np.int32)
        cnt = np.zeros(p, np.int32)
        check(_lib.load().orb_search_by_bow_kf(self._handle(), ctypes.byref(pKF1.view()),
                                               None if a1 is None else a1.ctypes.data, views, okp, p, m.ctypes.data,
                                               cnt.ctypes.data), "orb_search_by_bow_kf")
        return [(int(cnt[i]), m[i, :pKF1.N]) for i in range(p)]

    def SearchByBoWKFDevice(self, kf1s, kfs2, pair_kf1=None, ok1=None, ok2=None, stream=None, out=None):
        """SearchByBoW(KF1, KF2) on device-resident sides (orb_search_by_bow_kf_device): pair p matches
        kf1s[pair_kf1[p]] (a single DeviceKeyFrame or a list; pair_kf1 None: kf1s[0]) against kfs2[p].  ok1: per
        kf1 a uint8 CUDA tensor of cap flags or None (its has_mappoint); ok2: the same per pair.  Returns
        (matches12 [P, C] int32, counts [P] int32) CUDA tensors, C = max cap of the kf1s; a side flagged
        ORB_ERR_CAPACITY gives that count and an all -1 row.  Asynchronous on `stream`."""
        import torch
        kf1s = [kf1s] if isinstance(kf1s, DeviceKeyFrame) else list(kf1s)
        kfs2 = list(kfs2)
        n1, p = len(kf1s), len(kfs2)
        dev = kf1s[0]._keep[0].device
        C = max(k.cap for k in kf1s)
        if out is None:
            out = (torch.empty((max(p, 1), C), dtype=torch.int32, device=dev),
                   torch.empty(max(p, 1), dtype=torch.int32, device=dev))
        if p == 0:
            return out
        v1 = (KfDeviceView * n1)(*[k.view() for k in kf1s])
        v2 = (KfDeviceView * p)(*[k.view() for k in kfs2])
        o1 = [None] * n1 if ok1 is None else list(ok1)
        o2 = [None] * p if ok2 is None else list(ok2)
        if len(o1) != n1 or len(o2) != p:
            raise ValueError("ok1: one entry per kf1; ok2: one entry per pair")
        p1 = (ctypes.c_void_p * n1)(*[None if a is None else a.data_ptr() for a in o1])
        p2 = (ctypes.c_void_p * p)(*[None if a is None else a.data_ptr() for a in o2])
        pk = None if pair_kf1 is None else (ctypes.c_int32 * p)(*[int(i) for i in pair_kf1])
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_search_by_bow_kf_device(self._handle(), v1, n1, p1, v2, p2, pk, p, out[0].data_ptr(),
                                                      out[1].data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_search_by_bow_kf_device")
        return out

    def Fuse(self, kfs, points: FusePoints, th: float = 3.0, skip=None):
        """The search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:
        1356-1506) for every keyframe of `kfs` (a Frame carrying Ow / mvInvLevelSigma2 / mfLogScaleFactor, or a
        list of them) against one point set in one launch: LocalMapping::SearchInNeighbors' forward loop, or
        with one keyframe its reverse call.  skip[k, i] != 0: vpMapPoints[i] is NULL, isBad() or
        IsInKeyFrame(kfs[k]).  Returns (best_idx [K, n], best_dist [K, n]) int32: bestIdx where bestDist <=
        TH_LOW (else -1) and the minimum distance found (256: none).  Step 7, the map mutation, is the caller's."""
        kfs = [kfs] if isinstance(kfs, Frame) else list(kfs)
        K, n = len(kfs), points.n
        idx = np.full((K, n), -1, np.int32)
        dist = np.full((K, n), 256, np.int32)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, dtype=np.uint8)
            if sk.size != K * n:
                raise ValueError("skip: one flag per (keyframe, point)")
        views = (FuseKfView * max(K, 1))(*[k.fuse_view() for k in kfs])
        check(_lib.load().orb_fuse(self._handle(), views, K, ctypes.byref(points.view()),
                                   None if sk is None else sk.ctypes.data, float(th), idx.ctypes.data, dist.ctypes.data),
              "orb_fuse")
        return idx, dist

    def FuseDevice(self, kfs, points, th: float = 3.0, skip=None, Ow=None, log_scale_factor=None, stream=None,
                   out=None):
        """The same on device-resident keyframes and points (orb_fuse_device), asynchronous on `stream`.  kfs:
        tracking.DeviceFrame objects (their counts are read on the device; a flagged count gives -1 / 256 for
        that keyframe); points: CUDA tensors (pos [n, 3], normal [n, 3], min_dist [n], max_dist [n] float32,
        desc [n, 32] uint8); skip: uint8 [K, n] CUDA tensor or None; Ow: [K, 3] camera centres (None: -Rcw^T tcw
        in float32); log_scale_factor: mfLogScaleFactor (None: logf(mvScaleFactors[1])).  Returns (best_idx,
        best_dist) int32 [K, n] CUDA tensors."""
        import torch
        from .keyframe import logf
        from .tracking import FrameDeviceView, FuseKfDeviceView  # (tracking imports this module)

        kfs = list(kfs)
        pos, normal, min_dist, max_dist, desc = (t.contiguous() for t in points)
        K, n, dev = len(kfs), int(pos.shape[0]), pos.device
        if out is None:
            out = (torch.empty((max(K, 1), max(n, 1)), dtype=torch.int32, device=dev),
                   torch.empty((max(K, 1), max(n, 1)), dtype=torch.int32, device=dev))
        views = (FuseKfDeviceView * max(K, 1))()
        for k, kf in enumerate(kfs):
            ow = -(kf.Tcw[:, :3].T @ kf.Tcw[:, 3]) if Ow is None else np.asarray(Ow, np.float32)[k]
            lsf = logf(kf.mvScaleFactors[1]) if log_scale_factor is None else log_scale_factor
            ctypes.memmove(ctypes.byref(views[k].frame), ctypes.byref(kf.view()), ctypes.sizeof(FrameDeviceView))
            views[k].Ow[:] = [float(np.float32(x)) for x in ow]
            views[k].inv_level_sigma2 = kf.mvInvLevelSigma2.ctypes.data
            views[k].log_scale_factor = float(np.float32(lsf))
        pv = FusePointsView(n, pos.data_ptr(), normal.data_ptr(), min_dist.data_ptr(), max_dist.data_ptr(), desc.data_ptr())
        sk = None if skip is None else skip.contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_fuse_device(self._handle(), views, K, ctypes.byref(pv), None if sk is None else sk.data_ptr(),
                                          float(th), out[0].data_ptr(), out[1].data_ptr(),
                                          ctypes.c_void_p(st.cuda_stream)), "orb_fuse_device")
        return out[0][:K, :n], out[1][:K, :n]

    @staticmethod
    def _sim3_jobs(jobs, n_kfs):
        """The ctypes job records of SearchByProjectionSim3[Device] and the point offsets [B + 1]."""
        jobs = list(jobs)
        B = len(jobs)
        arr = (Sim3ProjJob * max(B, 1))()
        offs = np.zeros(B + 1, np.int64)
        for b, j in enumerate(jobs):
            a = arr[b]
            a.kf, a.first, a.count, a.mode = int(j["kf"]), int(j["first"]), int(j["count"]), int(j["mode"])
            a.th, a.ratio_hamming = float(np.float32(j["th"])), float(np.float32(j.get("ratio", 1.0)))
            a.Tcw[:] = [float(x) for x in np.asarray(j["Tcw"], np.float32).reshape(12)]
            a.Ow[:] = [float(x) for x in np.asarray(j["Ow"], np.float32).reshape(3)]
            offs[b + 1] = offs[b] + max(a.count, 0)
        return arr, offs

    def SearchByProjectionSim3(self, kfs, jobs, points: FusePoints, skip=None, taken0=None, stride=None):
        """Loop closing's three Sim3 searches (src/ORBmatcher.cc:496-619, :621-733 and the search half of Fuse,
        :1547-1651), batched (orb_sim3_projection).  kfs: Frame objects (a list).  jobs: dicts, one per call of
        a reference function: kf (index into kfs), first / count (the job's points in the pool `points`), mode
        (ORB_S3P_CLAIM_PROJECT, ORB_S3P_CLAIM_INVZ or ORB_S3P_FUSE), th, ratio (ratioHamming, default 1.0), Tcw
        (3 x 4) and Ow (3) as sim3_pose gives them.  skip: uint8, one flag per point of every job in job order
        (isBad() || spAlreadyFound.count(pMP)), or None; taken0: uint8 [B, stride], vpMatched[idx] != NULL before
        the call, or None; stride (default: the largest N) is the row length of `matched`.  Returns a dict:
        matched [B, stride] (the point of the job matched to each keypoint, -1 none), nmatches [B], best_idx and
        best_dist (one entry per point of every job, in job order) and offsets [B + 1] (job b's points are
        offsets[b] : offsets[b + 1]).  All int32 but offsets."""
        kfs = [kfs] if isinstance(kfs, Frame) else list(kfs)
        K = len(kfs)
        arr, offs = self._sim3_jobs(jobs, K)
        B, T = len(offs) - 1, int(offs[-1])
        if stride is None:
            stride = max([k.N for k in kfs] + [1])
        out = dict(matched=np.full((max(B, 1), stride), -1, np.int32), nmatches=np.zeros(max(B, 1), np.int32),
                   best_idx=np.full(max(T, 1), -1, np.int32), best_dist=np.full(max(T, 1), 256, np.int32))
        sk = tk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
            if sk.size != T:
                raise ValueError("skip: one flag per point of every job")
        if taken0 is not None:
            tk = np.ascontiguousarray(taken0, dtype=np.uint8)
            if tk.shape != (B, stride):
                raise ValueError("taken0: [jobs, stride] flags")
        views = (Sim3ProjKfView * max(K, 1))()
        for k, kf in enumerate(kfs):
            kf.fuse_view()  # (fills mfLogScaleFactor's default)
            views[k] = Sim3ProjKfView(kf.view(), kf.mfLogScaleFactor)
        check(_lib.load().orb_sim3_projection(self._handle(), views, K, arr, B, ctypes.byref(points.view()),
                                              None if sk is None else sk.ctypes.data,
                                              None if tk is None else tk.ctypes.data, int(stride),
                                              out["matched"].ctypes.data, out["nmatches"].ctypes.data,
                                              out["best_idx"].ctypes.data, out["best_dist"].ctypes.data),
              "orb_sim3_projection")
        return dict(matched=out["matched"][:B], nmatches=out["nmatches"][:B], best_idx=out["best_idx"][:T],
                    best_dist=out["best_dist"][:T], offsets=offs)

    def SearchByProjectionSim3Device(self, kfs, jobs, points, skip=None, taken0=None, stride=None,
                                     log_scale_factor=None, stream=None, out=None):
        """The same on device-resident keyframes and points (orb_sim3_projection_device), asynchronous on
        `stream`.  kfs: tracking.DeviceFrame objects (counts read on the device; a flagged count gives an empty
        result for every job of that keyframe); points: CUDA tensors (pos [n, 3], normal [n, 3], min_dist [n],
        max_dist [n] float32, desc [n, 32] uint8); skip / taken0: uint8 CUDA tensors or None; stride (default:
        the largest capacity); log_scale_factor: mfLogScaleFactor (None: logf(mvScaleFactors[1])).  Returns the
        dict of SearchByProjectionSim3 with CUDA tensors (offsets stays a numpy array), which `out` reuses."""
        import torch
        from .keyframe import logf
        from .tracking import FrameDeviceView, Sim3ProjKfDeviceView  # (tracking imports this module)

        kfs = list(kfs)
        K = len(kfs)
        pos, normal, min_dist, max_dist, desc = (t.contiguous() for t in points)
        n, dev = int(pos.shape[0]), pos.device
        arr, offs = self._sim3_jobs(jobs, K)
        B, T = len(offs) - 1, int(offs[-1])
        if stride is None:
            stride = max([k.cap for k in kfs] + [1])
        if out is None:
            out = dict(matched=torch.empty((max(B, 1), stride), dtype=torch.int32, device=dev),
                       nmatches=torch.empty(max(B, 1), dtype=torch.int32, device=dev),
                       best_idx=torch.empty(max(T, 1), dtype=torch.int32, device=dev),
                       best_dist=torch.empty(max(T, 1), dtype=torch.int32, device=dev))
        views = (Sim3ProjKfDeviceView * max(K, 1))()
        for k, kf in enumerate(kfs):
            lsf = logf(kf.mvScaleFactors[1]) if log_scale_factor is None else log_scale_factor
            ctypes.memmove(ctypes.byref(views[k].frame), ctypes.byref(kf.view()), ctypes.sizeof(FrameDeviceView))
            views[k].log_scale_factor = float(np.float32(lsf))
        pv = FusePointsView(n, pos.data_ptr(), normal.data_ptr(), min_dist.data_ptr(), max_dist.data_ptr(), desc.data_ptr())
        sk = None if skip is None else skip.contiguous()
        tk = None if taken0 is None else taken0.contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_sim3_projection_device(self._handle(), views, K, arr, B, ctypes.byref(pv),
                                                     None if sk is None else sk.data_ptr(),
                                                     None if tk is None else tk.data_ptr(), int(stride),
                                                     out["matched"].data_ptr(), out["nmatches"].data_ptr(),
                                                     out["best_idx"].data_ptr(), out["best_dist"].data_ptr(),
                                                     ctypes.c_void_p(st.cuda_stream)), "orb_sim3_projection_device")
        return dict(matched=out["matched"][:B], nmatches=out["nmatches"][:B], best_idx=out["best_idx"][:T],
                    best_dist=out["best_dist"][:T], offsets=offs)

    @staticmethod
    def _newpoints_params(pKF1, inertial, far_points, th_far_points, ratio_factor) -> NewPointsParams:
        if ratio_factor is None:  # 1.5f * mfScaleFactor (src/LocalMapping.cc:555)
            ratio_factor = np.float32(1.5) * pKF1.mvScaleFactors[1] if len(pKF1.mvScaleFactors) > 1 else 1.5
        return NewPointsParams(int(bool(inertial)), int(bool(far_points)), float(np.float32(th_far_points)),
                               float(np.float32(ratio_factor)))

    def CreateNewMapPoints(self, pKF1: KeyFrame, neighbours, matches12, n_matches=None, inertial: bool = False,
                           far_points: bool = False, th_far_points: float = 0.0, ratio_factor=None) -> dict:
        """The triangulation half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:626-910) for the
        matches of pKF1 against every keyframe of `neighbours` in one call: matches12 [P, N1] (and n_matches [P],
        optional) as SearchForTriangulationMany returned them.  Returns a dict: status [P, N1] int32 (NP_* of
        keyframe.py), x3d [P, N1, 3], from_stereo [P, N1] uint8, taken_by [N1] int32 and `new`, the records of
        the new map points (NEWPOINT_DTYPE) in upstream's creation order.  Step 6, the map mutation, is the
        caller's."""
        neighbours = list(neighbours)
        P, n1 = len(neighbours), pKF1.N
        C = max(n1, 1)
        m12 = np.full((max(P, 1), C), -1, np.int32)
        if P and n1:
            m12[:P, :n1] = np.asarray(matches12, np.int32).reshape(P, n1)
        cnt = None if n_matches is None else np.ascontiguousarray(n_matches, dtype=np.int32).reshape(P)
        status = np.zeros((max(P, 1), C), np.int32)
        x3d = np.zeros((max(P, 1), C, 3), np.float32)
        fs = np.zeros((max(P, 1), C), np.uint8)
        taken = np.full(C, -1, np.int32)
        rec = np.zeros(C, NEWPOINT_DTYPE)
        n_new = np.zeros(1, np.int32)
        out = NewPointsOut(status.ctypes.data, x3d.ctypes.data, fs.ctypes.data, taken.ctypes.data, rec.ctypes.data,
                           n_new.ctypes.data)
        v1 = pKF1.newpoints_view()
        v2 = (NewPointsKf * max(P, 1))(*[k.newpoints_view() for k in neighbours])
        prm = self._newpoints_params(pKF1, inertial, far_points, th_far_points, ratio_factor)
        check(_lib.load().orb_create_new_map_points(self._handle(), ctypes.byref(v1), v2, P, ctypes.byref(prm),
                                                    m12.ctypes.data, None if cnt is None else cnt.ctypes.data,
                                                    ctypes.byref(out)), "orb_create_new_map_points")
        return dict(status=status[:P, :n1], x3d=x3d[:P, :n1], from_stereo=fs[:P, :n1], taken_by=taken[:n1],
                    new=rec[:int(n_new[0])])

    def CreateNewMapPointsDevice(self, pKF1: DeviceKeyFrame, neighbours, matches12, n_matches, inertial: bool = False,
                                 far_points: bool = False, th_far_points: float = 0.0, ratio_factor=None, stream=None,
                                 out=None) -> dict:
        """The same on device-resident keyframes (orb_create_new_map_points_device), asynchronous on `stream`
        with no host synchronisation: matches12 [P, cap1] / n_matches [P] are the CUDA tensors
        SearchForTriangulationDevice(pKF1, neighbours, ...) returned, taken as they are (a pair flagged
        ORB_ERR_CAPACITY yields no points).  Returns a dict of CUDA tensors -- status [P, cap1] int32, x3d
        [P, cap1, 3] float32, from_stereo [P, cap1] uint8, taken_by [cap1] int32, records [cap1, 12] int32 (the
        bytes of NEWPOINT_DTYPE; newpoints_records() decodes a downloaded copy), n_new [1] int32 -- which `out`
        (an earlier call's dict) reuses."""
        import torch
        neighbours = list(neighbours)
        P, C = len(neighbours), pKF1.cap
        dev = pKF1._keep[0].device
        if out is None:
            out = dict(status=torch.empty((max(P, 1), C), dtype=torch.int32, device=dev),
                       x3d=torch.empty((max(P, 1), C, 3), dtype=torch.float32, device=dev),
                       from_stereo=torch.empty((max(P, 1), C), dtype=torch.uint8, device=dev),
                       taken_by=torch.empty(C, dtype=torch.int32, device=dev),
                       records=torch.empty((C, 12), dtype=torch.int32, device=dev),
                       n_new=torch.empty(1, dtype=torch.int32, device=dev))
        o = NewPointsOut(*[out[k].data_ptr() for k in ("status", "x3d", "from_stereo", "taken_by", "records", "n_new")])
        v1 = pKF1.newpoints_view()
        v2 = (NewPointsKfDevice * max(P, 1))(*[k.newpoints_view() for k in neighbours])
        prm = self._newpoints_params(pKF1, inertial, far_points, th_far_points, ratio_factor)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_lib.load().orb_create_new_map_points_device(self._handle(), ctypes.byref(v1), v2, P, ctypes.byref(prm),
                                                           matches12.data_ptr(),
                                                           None if n_matches is None else n_matches.data_ptr(),
                                                           ctypes.byref(o), ctypes.c_void_p(st.cuda_stream)),
              "orb_create_new_map_points_device")
        return out

    @staticmethod
    def newpoints_records(records, n_new) -> np.ndarray:
        """The first n_new records of CreateNewMapPointsDevice's `records` tensor as NEWPOINT_DTYPE (a download)."""
        n = int(n_new.item()) if hasattr(n_new, "item") else int(n_new)
        return np.ascontiguousarray(records.cpu().numpy()).view(NEWPOINT_DTYPE).reshape(-1)[:n]

    @staticmethod
    def DescriptorDistance(a, b) -> int:
        """Hamming distance of two 32-byte descriptors (src/ORBmatcher.cc:2384-2404)."""
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(32)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(32)
        return check(_lib.load().orb_descriptor_distance(a.ctypes.data, b.ctypes.data), "orb_descriptor_distance")

    @staticmethod
    def knn2_device(query, train, stream=None):
        """Best/second-best Hamming match of every query row among train rows (torch uint8 [n, 32] on GPU)."""
        import torch
        q = query.contiguous()
        t = train.contiguous()
        n = q.shape[0]
        idx = torch.empty(n, dtype=torch.int32, device=q.device)
        d1 = torch.empty(n, dtype=torch.int32, device=q.device)
        d2 = torch.empty(n, dtype=torch.int32, device=q.device)
        st = stream if stream is not None else torch.cuda.current_stream(q.device)
        check(_lib.load().orb_hamming_knn2_device(q.data_ptr(), n, t.data_ptr(), t.shape[0], idx.data_ptr(),
                                                  d1.data_ptr(), d2.data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_hamming_knn2_device")
        return idx, d1, d2

    @staticmethod
    def knn2_frames_device(desc, counts, pairs, stream=None, out=None):
        """Cross-frame knn2 over a batch of device feature blocks (orb_hamming_knn2_frames_device):
        desc uint8 [F, cap, 32], counts int32 [F, >= 1] (column 0 = descriptors per frame), pairs int32
        [P, 2] (query frame, train frame) on the device.  Returns (idx, best, second), int32 [P, cap]."""
        import torch
        d = desc.contiguous()
        c = counts.contiguous()
        pr = pairs.to(device=d.device, dtype=torch.int32).contiguous()
        n_pairs, cap = pr.shape[0], d.shape[1]
        if out is None:
            out = tuple(torch.empty((n_pairs, cap), dtype=torch.int32, device=d.device) for _ in range(3))
        st = stream if stream is not None else torch.cuda.current_stream(d.device)
        check(_lib.load().orb_hamming_knn2_frames_device(d.data_ptr(), c.data_ptr(), c.shape[1], cap, pr.data_ptr(),
                                                         n_pairs, out[0].data_ptr(), out[1].data_ptr(),
                                                         out[2].data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_hamming_knn2_frames_device")
        return out

    def ComputeDistinctiveDescriptors(self, desc, offsets):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-529) for a batch of map points:
        point p's observation descriptors are rows offsets[p]..offsets[p+1] of desc (uint8 [n, 32]).
        Returns (best int32[P], mDescriptor uint8[P, 32]); best -1 / a zero row for a point without
        descriptors (the reference leaves its mDescriptor unchanged)."""
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = len(offsets) - 1
        best = np.full(max(n, 1), -1, np.int32)
        out = np.zeros((max(n, 1), 32), np.uint8)
        check(_lib.load().orb_compute_distinctive_descriptors(self._handle(), desc.ctypes.data, offsets.ctypes.data, n,
                                                              best.ctypes.data, out.ctypes.data),
              "orb_compute_distinctive_descriptors")
        return best[:n], out[:n]

    @staticmethod
    def compute_distinctive_descriptors_device(desc, offsets, out=None, stream=None):
        """The same on device tensors (desc uint8 [n, 32], offsets int32 [P + 1]); async on `stream`.
        Returns (best int32 [P], out uint8 [P, 32])."""
        import torch
        d = desc.contiguous()
        o = offsets.contiguous()
        n = o.shape[0] - 1
        best = torch.empty(max(n, 1), dtype=torch.int32, device=d.device)
        if out is None:
            out = torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=d.device)
        st = stream if stream is not None else torch.cuda.current_stream(d.device)
        check(_lib.load().orb_compute_distinctive_descriptors_device(d.data_ptr(), o.data_ptr(), n, best.data_ptr(),
                                                                     out.data_ptr(), ctypes.c_void_p(st.cuda_stream)),
              "orb_compute_distinctive_descriptors_device")
        return best[:n], out[:n]

    def SearchByProjectionFrame(self, CurrentFrame: Frame, LastFrame: Frame, th: float, bMono: bool):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
        (src/ORBmatcher.cc:1951-2185).  Returns (nmatches, match) with match[i2] = the LastFrame index
        whose map point CurrentFrame.mvpMapPoints[i2] receives (-1: none)."""
        m = np.full(max(CurrentFrame.N, 1), -1, np.int32)
        n = ctypes.c_int32()
        check(_lib.load().orb_search_by_projection_frame(self._handle(), ctypes.byref(CurrentFrame.view()),
                                                         ctypes.byref(LastFrame.last_points()), float(th),
                                                         int(bMono), m.ctypes.data, ctypes.byref(n)),
              "orb_search_by_projection_frame")
        return n.value, m[:CurrentFrame.N]

    def SearchByProjection(self, F: Frame, vpMapPoints: LocalMapPoints, th: float = 3, bFarPoints: bool = False,
                           thFarPoints: float = 50.0, frame_taken=None):
        """SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, bFarPoints, thFarPoints)
        (src/ORBmatcher.cc:46-240).  frame_taken[i]: keypoint i already holds a map point with
        observations.  Returns (nmatches, match) with match[i] = index of the map point assigned."""
        m = np.full(max(F.N, 1), -1, np.int32)
        n = ctypes.c_int32()
        tk = None if frame_taken is None else np.ascontiguousarray(frame_taken, dtype=np.uint8)
        check(_lib.load().orb_search_by_projection_local(self._handle(), ctypes.byref(F.view()),
                                                         None if tk is None else tk.ctypes.data,
                                                         ctypes.byref(vpMapPoints.view()), float(th), int(bFarPoints),
                                                         float(thFarPoints), m.ctypes.data, ctypes.byref(n)),
              "orb_search_by_projection_local")
        return n.value, m[:F.N]
