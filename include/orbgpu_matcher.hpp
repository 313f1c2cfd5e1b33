/*
 * orbgpu_matcher.hpp -- header-only drop-in for the ORB_SLAM3::ORBmatcher methods on the GPU path
 * (include/ORBmatcher.h:40-76, src/ORBmatcher.cc) over the C ABI (orbgpu.h):
 *
 *   ORBmatcher(float nnratio = 0.6, bool checkOri = true)                       (:41)
 *   static int DescriptorDistance(a, b)                                          (:2384-2404)
 *   int SearchForTriangulation(KeyFrame*, KeyFrame*, vector<pair<size_t,size_t>>&, bOnlyStereo, bCoarse)
 *                                                                                (:1046-1324)
 *   int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)   (:1951-2185)
 *   int SearchByProjection(Frame& F, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) (:46-240)
 *   int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)   (:260-494)
 *   int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  (:893-1044), and its batched
 *       form over vpCovKFi (src/LoopClosing.cc:840-851; needs A::IsBad(KeyFrame*))
 *   int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th = 3.0)          (:1326-1534, bRight = false)
 *   int SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)            (:496-619)
 *   int SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)  (:621-733)
 *   int Fuse(KeyFrame*, Sim3f& Scw, vpPoints, th, vpReplacePoint)  (:1547-1676), and batched forms of the three
 *   void Fuse(const vector<KeyFrame*>&, const vector<MapPoint*>&, th, vector<int>& vnFused)   (the forward loop
 *                                                             of SearchInNeighbors, src/LocalMapping.cc:991-1001)
 *
 * The class translates the reference's KeyFrame / Frame / MapPoint objects into the ABI's flat views
 * (orb_kf_view_t, orb_frame_view_t, orb_last_points_t, orb_local_points_t), calls the HIP matcher,
 * and writes the results back exactly where the reference writes them (vMatchedPairs,
 * CurrentFrame.mvpMapPoints, F.mvpMapPoints, vpMapPointMatches).  The object graph is reached through an accessor type A
 * so that the same code runs on the reference's classes (orbgpu::ORBSLAM3MatcherAccess below, compiled
 * inside the reference build) and on a mock graph in this repository's CPU test
 * (tests/native/matcher_shim_check.cpp):
 *
 *   struct A {
 *     using KeyFrame = ...; using Frame = ...; using MapPoint = ...;
 *     // keyframes (SearchForTriangulation)
 *     static int N(KeyFrame*);                          static const orb_keypoint_t* KeysUn(KeyFrame*);
 *     static const uint8_t* Descriptors(KeyFrame*);     static const float* URight(KeyFrame*);
 *     static std::vector<MapPoint*> MapPointMatches(KeyFrame*);
 *     static const FeatureVector& FeatVec(KeyFrame*);   // std::map<node id, std::vector<unsigned>>
 *     static void Pinhole(KeyFrame*, float K[4]);       // fx, fy, cx, cy of mpCamera
 *     static int Levels(KeyFrame*);  static const float* ScaleFactors(KeyFrame*);
 *     static const float* LevelSigma2(KeyFrame*);
 *     static orb_kf_pair_geom_t PairGeometry(KeyFrame* pKF1, KeyFrame* pKF2);   // :1054-1072
 *     static bool SingleCamera(KeyFrame*);              // mpCamera2 == NULL (and NLeft == -1)
 *     // frames (SearchByProjection)
 *     static orb_frame_view_t View(const Frame&);       // keypoints, grid, camera, levels, GetPose()
 *     static bool SingleCamera(const Frame&);           // Nleft == -1
 *     static std::vector<MapPoint*>& MapPoints(Frame&); // mvpMapPoints
 *     static const std::vector<MapPoint*>& MapPoints(const Frame&);
 *     static bool Outlier(const Frame&, int i);         // mvbOutlier[i]
 *     static const FeatureVector& FeatVec(const Frame&);  // mFeatVec after Frame::ComputeBoW (SearchByBoW only;
 *                                                       // it reads the frame's keypoints and descriptors from View)
 *     // map points
 *     static int Observations(MapPoint*);  static bool IsBad(MapPoint*);
 *     static void WorldPos(MapPoint*, float X[3]);  static void Descriptor(MapPoint*, uint8_t d[32]);
 *     static void Track(MapPoint*, orbgpu::TrackFields*);   // mbTrackInView, mTrackProjX/Y/XR, ...
 *     // Fuse only (int Fuse(KeyFrame*, const vector<MapPoint*>&, th) :1326-1534 and its batched overload)
 *     static void FuseGeometry(KeyFrame*, orb_fuse_kf_t*);  // frame.min_x .. max_y, grid_inv_w / h, bf, Tcw =
 *                                   // GetPose(); Ow = GetCameraCenter(); mvInvLevelSigma2; mfLogScaleFactor
 *     static MapPoint* GetMapPoint(KeyFrame*, int idx);   static void AddMapPoint(KeyFrame*, MapPoint*, int idx);
 *     static bool IsInKeyFrame(MapPoint*, KeyFrame*);     static void AddObservation(MapPoint*, KeyFrame*, int idx);
 *     static void Replace(MapPoint* pMP, MapPoint* by);   // pMP->Replace(by)
 *     static void Normal(MapPoint*, float n[3]);          // GetNormal()
 *     static float MinDistance(MapPoint*);  static float MaxDistance(MapPoint*);   // mfMinDistance, mfMaxDistance
 *   };
 *
 * Scope: pinhole single-camera frames and keyframes (the configuration the ABI covers).  For the
 * two-camera fisheye rig (mpCamera2 / Nleft != -1) Supports() is false and the caller keeps the
 * reference's CPU body.
 *
 * Failures (orbgpu_status.hpp): nothing here throws.  A library failure returns the reference's result
 * for a search that matches nothing -- 0, vMatchedPairs empty, no map point written (SearchByBoW: every
 * entry of vpMapPointMatches NULL) -- and a failed
 * ComputeDistinctiveDescriptors leaves every descriptor as it was; orbgpu::LastShimError() reports it.
 */
#ifndef ORBGPU_MATCHER_HPP
#define ORBGPU_MATCHER_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "orbgpu.h"
#include "orbgpu_status.hpp"

namespace orbgpu {

// The tracking fields Frame::isInFrustum leaves in a map point (src/Frame.cc:667-773).
struct TrackFields {
    bool in_view = false;      // mbTrackInView
    float proj[3] = {0, 0, 0}; // mTrackProjX, mTrackProjY, mTrackProjXR
    float view_cos = 0;        // mTrackViewCos
    float depth = 0;           // mTrackDepth
    int level = 0;             // mnTrackScaleLevel
};

namespace detail {

// One device matcher handle per (thread, nnratio, checkOri): the reference constructs ORBmatcher
// objects on the stack per call site (e.g. src/LocalMapping.cc:536, src/Tracking.cc:4120), and a
// handle owns a HIP stream and staging buffers that should outlive them.
class HandleCache {
public:
    orb_matcher_t Get(float nnratio, bool check_ori) {
        const auto key = std::make_pair(nnratio, check_ori);
        auto it = handles_.find(key);
        if (it != handles_.end()) return it->second;
        orb_matcher_t h = nullptr;
        if (Failed(orb_matcher_create(nnratio, check_ori ? 1 : 0, &h), "orb_matcher_create"))
            return nullptr;  // not cached: the next call tries again
        handles_[key] = h;
        return h;
    }
    ~HandleCache() {
        for (auto& kv : handles_) orb_matcher_destroy(kv.second);
    }

private:
    std::map<std::pair<float, bool>, orb_matcher_t> handles_;
};

inline orb_matcher_t ThreadHandle(float nnratio, bool check_ori) {
    thread_local HandleCache cache;
    return cache.Get(nnratio, check_ori);
}

// A DBoW2::FeatureVector (std::map: node ids ascending, each node's indices in insertion order) as the
// views' CSR arrays.
template <class FV>
inline void FlattenFeatVec(const FV& fv, std::vector<uint32_t>& node, std::vector<int32_t>& offset,
                           std::vector<int32_t>& index) {
    node.reserve(fv.size());
    offset.reserve(fv.size() + 1);
    offset.push_back(0);
    for (const auto& kv : fv) {
        node.push_back((uint32_t)kv.first);
        for (auto idx : kv.second) index.push_back((int32_t)idx);
        offset.push_back((int32_t)index.size());
    }
}

// A keyframe's orb_kf_view_t and the arrays it points into.
template <class A>
struct KfViewStore {
    orb_kf_view_t view{};
    std::vector<uint8_t> has_mp;
    std::vector<uint32_t> node;
    std::vector<int32_t> offset, index;

    explicit KfViewStore(typename A::KeyFrame* k) {
        const int n = A::N(k);
        const auto mps = A::MapPointMatches(k);
        has_mp.resize(n);
        for (int i = 0; i < n; ++i) has_mp[i] = (i < (int)mps.size() && mps[i]) ? 1 : 0;  // GetMapPoint(i) != NULL
        FlattenFeatVec(A::FeatVec(k), node, offset, index);
        float K[4];
        A::Pinhole(k, K);
        view.n = n;
        view.kps_un = A::KeysUn(k);
        view.desc = A::Descriptors(k);
        view.u_right = A::URight(k);
        view.has_mappoint = has_mp.data();
        view.n_nodes = (int32_t)node.size();
        view.fv_node = node.data();
        view.fv_offset = offset.data();
        view.fv_index = index.data();
        view.fx = K[0];
        view.fy = K[1];
        view.cx = K[2];
        view.cy = K[3];
        view.nlevels = A::Levels(k);
        view.scale_factors = A::ScaleFactors(k);
        view.level_sigma2 = A::LevelSigma2(k);
    }
    KfViewStore(const KfViewStore&) = delete;
    KfViewStore& operator=(const KfViewStore&) = delete;
};

// A keyframe's orb_fuse_kf_t (it points into the keyframe's own arrays).
template <class A>
struct FuseKfStore {
    orb_fuse_kf_t view{};
    explicit FuseKfStore(typename A::KeyFrame* k) {
        float K[4];
        A::Pinhole(k, K);
        orb_frame_view_t& f = view.frame;
        f.n = A::N(k);
        f.kps_un = A::KeysUn(k);
        f.desc = A::Descriptors(k);
        f.u_right = A::URight(k);
        f.fx = K[0];
        f.fy = K[1];
        f.cx = K[2];
        f.cy = K[3];
        f.nlevels = A::Levels(k);
        f.scale_factors = A::ScaleFactors(k);
        A::FuseGeometry(k, &view);  // bounds, grid inverses, mbf, GetPose(), Ow, mvInvLevelSigma2, mfLogScaleFactor
    }
};

// vpMapPoints as orb_fuse_points_t: dead[i] = NULL or isBad() (zero rows, skipped for every keyframe).
template <class A>
struct FusePointStore {
    orb_fuse_points_t view{};
    std::vector<uint8_t> dead, desc;
    std::vector<float> pos, normal, min_dist, max_dist;
    explicit FusePointStore(const std::vector<typename A::MapPoint*>& pts) {
        const size_t n = pts.size();
        dead.assign(n, 0);
        desc.assign(32 * n, 0);
        pos.assign(3 * n, 0.f);
        normal.assign(3 * n, 0.f);
        min_dist.assign(n, 0.f);
        max_dist.assign(n, 0.f);
        for (size_t i = 0; i < n; ++i) {
            if (!pts[i] || A::IsBad(pts[i])) {
                dead[i] = 1;
                continue;
            }
            A::WorldPos(pts[i], &pos[3 * i]);
            A::Normal(pts[i], &normal[3 * i]);
            min_dist[i] = A::MinDistance(pts[i]);
            max_dist[i] = A::MaxDistance(pts[i]);
            A::Descriptor(pts[i], &desc[32 * i]);
        }
        view.n = (int32_t)n;
        view.pos = pos.data();
        view.normal = normal.data();
        view.min_dist = min_dist.data();
        view.max_dist = max_dist.data();
        view.desc = desc.data();
    }
};
}  // namespace detail

template <class A>
void ComputeDistinctiveDescriptors(const std::vector<typename A::MapPoint*>& points);

template <class A>
class ORBmatcher {
public:
    using KeyFrame = typename A::KeyFrame;
    using Frame = typename A::Frame;
    using MapPoint = typename A::MapPoint;

    static const int TH_LOW = 50;        // src/ORBmatcher.cc:36-38
    static const int TH_HIGH = 100;
    static const int HISTO_LENGTH = 30;

    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orb_descriptor_distance(a, b); }

    static bool Supports(KeyFrame* a, KeyFrame* b) { return A::SingleCamera(a) && A::SingleCamera(b); }
    static bool Supports(const Frame& f) { return A::SingleCamera(f); }
    static bool Supports(KeyFrame* k, const Frame& f) { return A::SingleCamera(k) && A::SingleCamera(f); }

    // src/ORBmatcher.cc:1046-1324.  vMatchedPairs = (idx1, idx2) in increasing idx1 (:1313-1321).
    int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               const bool bOnlyStereo, const bool bCoarse = false) {
        std::vector<std::vector<std::pair<size_t, size_t>>> all;
        const std::vector<int> n = SearchForTriangulation(pKF1, std::vector<KeyFrame*>{pKF2}, all, bOnlyStereo, bCoarse);
        vMatchedPairs = std::move(all[0]);
        return n[0];
    }

    // The loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:565-610) in one launch: pKF1
    // against every neighbour, all against pKF1's map points as they are at the call.  The loop adds
    // map points to pKF1 while it walks the neighbours (AddMapPoint(pMP, idx1)), so a caller that
    // triangulates neighbour p's pairs after neighbour q < p must drop the pairs whose idx1 received
    // a map point meanwhile; with checkOri == false (LocalMapping's ORBmatcher(0.6, false)) every other
    // pair equals what the per-neighbour call would return, since vbMatched2 is never set (:1256-1257).
    std::vector<int> SearchForTriangulation(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2,
                                            std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatchedPairs,
                                            const bool bOnlyStereo, const bool bCoarse = false) {
        const size_t p = vpKF2.size();
        vvMatchedPairs.assign(p, {});
        std::vector<int> counts(p, 0);
        if (p == 0) return counts;
        detail::KfViewStore<A> v1(pKF1);
        std::vector<std::unique_ptr<detail::KfViewStore<A>>> v2;
        std::vector<orb_kf_view_t> views(p);
        std::vector<orb_kf_pair_geom_t> geoms(p);
        for (size_t i = 0; i < p; ++i) {
            v2.emplace_back(new detail::KfViewStore<A>(vpKF2[i]));
            views[i] = v2.back()->view;
            geoms[i] = A::PairGeometry(pKF1, vpKF2[i]);
        }
        const int n1 = v1.view.n;
        std::vector<int32_t> m12((size_t)p * (n1 > 0 ? n1 : 1), -1), cnt(p, 0);
        if (Failed(orb_search_for_triangulation(Handle(), &v1.view, views.data(), geoms.data(), (int)p,
                                                bOnlyStereo ? 1 : 0, bCoarse ? 1 : 0, m12.data(), cnt.data()),
                   "orb_search_for_triangulation"))
            return counts;  // no pairs, 0 matches
        for (size_t k = 0; k < p; ++k) {
            auto& out = vvMatchedPairs[k];
            out.reserve(cnt[k]);
            for (int i = 0; i < n1; ++i) {
                const int32_t j = m12[k * n1 + i];
                if (j >= 0) out.emplace_back((size_t)i, (size_t)j);
            }
            counts[k] = cnt[k];
        }
        return counts;
    }

    // src/ORBmatcher.cc:1951-2185.  The matches are written into CurrentFrame.mvpMapPoints as the
    // reference does (CurrentFrame.mvpMapPoints[i2] = LastFrame.mvpMapPoints[i]); entries it does not
    // match keep what they held.  Tracking clears the vector before every call (src/Tracking.cc:4137,
    // 4156); a keypoint that already holds a map point with observations is skipped by every candidate
    // search (:2038-2041), so the shim hides it from the grid (its copy of the keypoint is moved out of
    // the frame bounds), which is the same skip for every last-frame point.
    int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) {
        auto& cur_mps = A::MapPoints(CurrentFrame);
        orb_frame_view_t cur = A::View(CurrentFrame);
        std::vector<orb_keypoint_t> hidden;
        for (int i2 = 0; i2 < cur.n && i2 < (int)cur_mps.size(); ++i2) {
            if (!cur_mps[i2] || A::Observations(cur_mps[i2]) <= 0) continue;
            if (hidden.empty()) hidden.assign(cur.kps_un, cur.kps_un + cur.n);
            hidden[i2].x = cur.min_x - 1e6f;  // outside every grid cell (Frame::PosInGrid fails)
        }
        if (!hidden.empty()) cur.kps_un = hidden.data();
        const orb_frame_view_t lastv = A::View(LastFrame);
        const auto& last_mps = A::MapPoints(LastFrame);
        const int nl = lastv.n;
        std::vector<uint8_t> valid(nl, 0), observed(nl, 0), desc((size_t)nl * 32, 0);
        std::vector<float> xyz((size_t)nl * 3, 0.f);
        for (int i = 0; i < nl; ++i) {
            MapPoint* pMP = i < (int)last_mps.size() ? last_mps[i] : nullptr;
            if (!pMP || A::Outlier(LastFrame, i)) continue;  // (:1980-1984)
            valid[i] = 1;
            observed[i] = A::Observations(pMP) > 0 ? 1 : 0;
            A::WorldPos(pMP, &xyz[3 * (size_t)i]);
            A::Descriptor(pMP, &desc[32 * (size_t)i]);
        }
        orb_last_points_t last{};
        last.n = nl;
        last.valid = valid.data();
        last.observed = observed.data();
        last.xyz = xyz.data();
        last.desc = desc.data();
        last.kps_un = lastv.kps_un;
        for (int k = 0; k < 12; ++k) last.Tcw[k] = lastv.Tcw[k];
        std::vector<int32_t> match(cur.n > 0 ? cur.n : 1, -1);
        int32_t n = 0;
        if (Failed(orb_search_by_projection_frame(Handle(), &cur, &last, th, bMono ? 1 : 0, match.data(), &n),
                   "orb_search_by_projection_frame"))
            return 0;
        for (int i2 = 0; i2 < cur.n; ++i2)
            if (match[i2] >= 0) cur_mps[i2] = last_mps[match[i2]];
        return n;
    }

    // src/ORBmatcher.cc:46-240 (Tracking::SearchLocalPoints, src/Tracking.cc:4825), after
    // Frame::isInFrustum has set the tracking fields of vpMapPoints.
    int SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th = 3,
                           const bool bFarPoints = false, const float thFarPoints = 50.0f) {
        const orb_frame_view_t fv = A::View(F);
        auto& fmps = A::MapPoints(F);
        std::vector<uint8_t> taken(fv.n > 0 ? fv.n : 1, 0);
        for (int i = 0; i < fv.n && i < (int)fmps.size(); ++i)
            taken[i] = (fmps[i] && A::Observations(fmps[i]) > 0) ? 1 : 0;  // (:103-105)
        const int np = (int)vpMapPoints.size();
        std::vector<uint8_t> in_view(np), bad(np), observed(np), desc((size_t)np * 32, 0);
        std::vector<float> proj((size_t)np * 3), view_cos(np), depth(np);
        std::vector<int32_t> level(np);
        for (int i = 0; i < np; ++i) {
            MapPoint* pMP = vpMapPoints[i];
            TrackFields t;
            A::Track(pMP, &t);
            in_view[i] = t.in_view ? 1 : 0;
            bad[i] = A::IsBad(pMP) ? 1 : 0;
            observed[i] = A::Observations(pMP) > 0 ? 1 : 0;
            for (int k = 0; k < 3; ++k) proj[3 * (size_t)i + k] = t.proj[k];
            view_cos[i] = t.view_cos;
            depth[i] = t.depth;
            level[i] = t.level;
            if (t.in_view && !bad[i]) A::Descriptor(pMP, &desc[32 * (size_t)i]);
        }
        orb_local_points_t pts{};
        pts.n = np;
        pts.track_in_view = in_view.data();
        pts.is_bad = bad.data();
        pts.observed = observed.data();
        pts.track_proj = proj.data();
        pts.track_view_cos = view_cos.data();
        pts.track_depth = depth.data();
        pts.track_level = level.data();
        pts.desc = desc.data();
        std::vector<int32_t> match(fv.n > 0 ? fv.n : 1, -1);
        int32_t n = 0;
        if (Failed(orb_search_by_projection_local(Handle(), &fv, taken.data(), &pts, th, bFarPoints ? 1 : 0,
                                                  thFarPoints, match.data(), &n),
                   "orb_search_by_projection_local"))
            return 0;
        for (int i = 0; i < fv.n; ++i)
            if (match[i] >= 0) fmps[i] = vpMapPoints[match[i]];  // F.mvpMapPoints[bestIdx] = pMP (:156)
        return n;
    }

    // src/ORBmatcher.cc:260-494 (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:3943; Relocalization's
    // candidate loop).  vpMapPointMatches is set to F.N NULL entries first (:266); entry i then receives
    // pKF's map point of the keyframe feature matched to keypoint i.  F.mFeatVec must be computed
    // (Frame::ComputeBoW, as both callers do before the search).
    int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
        const std::vector<MapPoint*> vpMapPointsKF = A::MapPointMatches(pKF);
        const orb_frame_view_t fv = A::View(F);
        const int nf = fv.n > 0 ? fv.n : 0;
        vpMapPointMatches.assign(nf, static_cast<MapPoint*>(nullptr));
        detail::KfViewStore<A> kv(pKF);
        std::vector<uint8_t> usable(kv.view.n > 0 ? kv.view.n : 1, 0);
        for (int i = 0; i < kv.view.n && i < (int)vpMapPointsKF.size(); ++i)  // pMP && !pMP->isBad() (:307-313)
            usable[i] = (vpMapPointsKF[i] && !A::IsBad(vpMapPointsKF[i])) ? 1 : 0;
        std::vector<uint32_t> node;
        std::vector<int32_t> offset, index;
        detail::FlattenFeatVec(A::FeatVec(static_cast<const Frame&>(F)), node, offset, index);
        orb_kf_view_t frame{};  // what a search reads of the frame: n, keypoints (angle), descriptors, FeatureVector
        frame.n = nf;
        frame.kps_un = fv.kps_un;
        frame.desc = fv.desc;
        frame.n_nodes = (int32_t)node.size();
        frame.fv_node = node.data();
        frame.fv_offset = offset.data();
        frame.fv_index = index.data();
        const uint8_t* flags = usable.data();
        std::vector<int32_t> match(nf > 0 ? nf : 1, -1);
        int32_t n = 0;
        if (Failed(orb_search_by_bow(Handle(), &kv.view, &flags, 1, &frame, match.data(), &n), "orb_search_by_bow"))
            return 0;  // every entry NULL
        for (int i = 0; i < nf; ++i)
            if (match[i] >= 0) vpMapPointMatches[i] = vpMapPointsKF[match[i]];  // vpMapPointMatches[bestIdxF] = pMP (:391)
        return n;
    }

    // src/ORBmatcher.cc:893-1044 (LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:845).  vpMatches12 is
    // set to pKF1's map-point count of NULL entries first (:907); entry idx1 then receives pKF2's map point of the
    // feature matched to pKF1's feature idx1.  A library failure: 0, every entry NULL.
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
        std::vector<std::vector<MapPoint*>> vv;
        std::vector<int> n;
        SearchByBoWPairs(pKF1, std::vector<KeyFrame*>(1, pKF2), vv, n);
        vpMatches12.swap(vv[0]);
        return n[0];
    }

    // The window loop of src/LoopClosing.cc:840-851 in one library call: vvpMatches12[j] and vnMatches[j] are
    // what SearchByBoW(pKF1, vpKF2s[j], vvpMatches12[j]) gives; a keyframe that is NULL or isBad() is skipped as at
    // :842 (its vector stays empty, its count 0).  Returns false when the library failed (every count 0).
    bool SearchByBoW(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2s,
                     std::vector<std::vector<MapPoint*>>& vvpMatches12, std::vector<int>& vnMatches) {
        std::vector<KeyFrame*> live;
        std::vector<size_t> at;
        for (size_t j = 0; j < vpKF2s.size(); ++j)
            if (vpKF2s[j] && !A::IsBad(vpKF2s[j])) {
                live.push_back(vpKF2s[j]);
                at.push_back(j);
            }
        std::vector<std::vector<MapPoint*>> vv;
        std::vector<int> n;
        const bool ok = SearchByBoWPairs(pKF1, live, vv, n);
        vvpMatches12.assign(vpKF2s.size(), std::vector<MapPoint*>());
        vnMatches.assign(vpKF2s.size(), 0);
        for (size_t k = 0; k < live.size(); ++k) {
            vvpMatches12[at[k]].swap(vv[k]);
            vnMatches[at[k]] = n[k];
        }
        return ok;
    }

    // The same search as feature indices: rows[p * N1 + idx1] = the matched feature of kfs[p] or -1, N1 = pKF1's
    // feature count (every keyframe non-NULL).  What orbgpu::LoopBowProblems (orbgpu_sim3.hpp) merges.
    bool SearchByBoWIndices(KeyFrame* pKF1, const std::vector<KeyFrame*>& kfs, std::vector<int32_t>& rows,
                            std::vector<int32_t>& counts) {
        const size_t P = kfs.size();
        detail::KfViewStore<A> v1(pKF1);
        const int n1 = v1.view.n > 0 ? v1.view.n : 0;
        rows.assign(P * (size_t)n1 + 1, -1);
        counts.assign(P + 1, 0);
        if (P == 0) return true;
        // ok = pMP && !pMP->isBad() on either side (:939-943, :960-967)
        auto usable = [](KeyFrame* k, int n) {
            const std::vector<MapPoint*> mps = A::MapPointMatches(k);
            std::vector<uint8_t> ok(n > 0 ? n : 1, 0);
            for (int i = 0; i < n && i < (int)mps.size(); ++i) ok[i] = (mps[i] && !A::IsBad(mps[i])) ? 1 : 0;
            return ok;
        };
        const std::vector<uint8_t> ok1 = usable(pKF1, n1);
        std::vector<std::unique_ptr<detail::KfViewStore<A>>> stores;
        std::vector<orb_kf_view_t> views;
        std::vector<std::vector<uint8_t>> ok2(P);
        std::vector<const uint8_t*> ok2p(P);
        for (size_t p = 0; p < P; ++p) {
            stores.emplace_back(new detail::KfViewStore<A>(kfs[p]));
            views.push_back(stores.back()->view);
            ok2[p] = usable(kfs[p], views[p].n);
            ok2p[p] = ok2[p].data();
        }
        if (Failed(orb_search_by_bow_kf(Handle(), &v1.view, ok1.data(), views.data(), ok2p.data(), (int)P, rows.data(),
                                        counts.data()),
                   "orb_search_by_bow_kf")) {
            rows.assign(P * (size_t)n1 + 1, -1);
            counts.assign(P + 1, 0);
            return false;
        }
        return true;
    }

    // (for orbgpu::LoopBowProblems: the merge and the gather run through this matcher's handle)
    orb_matcher_t LibraryHandle() const { return Handle(); }

    // src/ORBmatcher.cc:1326-1534 without bRight (two-camera rigs keep the CPU body: Supports(pKF) is false
    // for NLeft != -1).  One orb_fuse call for the search (steps 1-6), then step 7 (:1506-1527) here, in
    // index order, with the skip tests evaluated again at apply time.
    static bool Supports(KeyFrame* k) { return A::SingleCamera(k); }
    int Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th = 3.0f) {
        std::vector<int> n;
        Fuse(std::vector<KeyFrame*>{pKF}, vpMapPoints, th, n);
        return n[0];
    }

    // The forward loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:991-1001) in one launch:
    // vnFused[k] = what Fuse(vpKFs[k], vpMapPoints, th) returns when the calls are made one after another,
    // and the map ends in the same state.  Inside one call a point's search does not depend on what earlier
    // points did to the map; across calls it does in one way: pMPinKF->Replace(pMP) ends in
    // pMP->ComputeDistinctiveDescriptors() (src/MapPoint.cc:377), so a survivor may search the later
    // keyframes with another descriptor.  Before a keyframe is applied, every live point whose descriptor
    // is no longer the one sent is searched again against that keyframe (one small orb_fuse call per
    // keyframe at most).  Failures: the first call failing mutates nothing and every count is 0; a failing
    // re-search stops there (the keyframes already applied stay applied, the rest count 0).
    void Fuse(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMapPoints, const float th,
              std::vector<int>& vnFused) {
        const size_t K = vpKFs.size(), n = vpMapPoints.size();
        vnFused.assign(K, 0);
        if (K == 0 || n == 0) return;
        std::vector<detail::FuseKfStore<A>> kfs;
        kfs.reserve(K);
        for (KeyFrame* k : vpKFs) kfs.emplace_back(k);
        std::vector<orb_fuse_kf_t> views(K);
        for (size_t k = 0; k < K; ++k) views[k] = kfs[k].view;
        detail::FusePointStore<A> sent(vpMapPoints);
        std::vector<uint8_t> skip(K * n);
        for (size_t k = 0; k < K; ++k)
            for (size_t i = 0; i < n; ++i) skip[k * n + i] = sent.dead[i] || A::IsInKeyFrame(vpMapPoints[i], vpKFs[k]);
        std::vector<int32_t> best(K * n, -1);
        if (Failed(orb_fuse(Handle(), views.data(), (int)K, &sent.view, skip.data(), th, best.data(), nullptr), "orb_fuse"))
            return;
        for (size_t k = 0; k < K; ++k) {
            KeyFrame* pKF = vpKFs[k];
            // the points whose descriptor changed since it was sent: their results for this keyframe are stale
            std::vector<MapPoint*> again;
            std::vector<size_t> again_i;
            for (size_t i = 0; k > 0 && i < n; ++i) {
                MapPoint* pMP = vpMapPoints[i];
                if (sent.dead[i] || A::IsBad(pMP) || A::IsInKeyFrame(pMP, pKF)) continue;
                uint8_t d[32];
                A::Descriptor(pMP, d);
                if (std::memcmp(d, &sent.desc[32 * i], 32) == 0) continue;
                again.push_back(pMP);
                again_i.push_back(i);
            }
            if (!again.empty()) {
                detail::FusePointStore<A> now(again);
                std::vector<int32_t> b(again.size(), -1);
                if (Failed(orb_fuse(Handle(), &views[k], 1, &now.view, nullptr, th, b.data(), nullptr), "orb_fuse"))
                    return;
                for (size_t j = 0; j < again.size(); ++j) best[k * n + again_i[j]] = b[j];
            }
            int nFused = 0;
            for (size_t i = 0; i < n; ++i) {  // step 7 (:1506-1527)
                MapPoint* pMP = vpMapPoints[i];
                if (!pMP || A::IsBad(pMP) || A::IsInKeyFrame(pMP, pKF)) continue;  // (:1361-1376, at apply time)
                const int32_t bestIdx = best[k * n + i];
                if (bestIdx < 0) continue;
                MapPoint* pMPinKF = A::GetMapPoint(pKF, bestIdx);
                if (pMPinKF) {
                    if (!A::IsBad(pMPinKF)) {
                        if (A::Observations(pMPinKF) > A::Observations(pMP)) A::Replace(pMP, pMPinKF);
                        else A::Replace(pMPinKF, pMP);
                    }
                } else {
                    A::AddObservation(pMP, pKF, bestIdx);
                    A::AddMapPoint(pKF, pMP, bestIdx);
                }
                ++nFused;
            }
            vnFused[k] = nFused;
        }
    }

    // ---- Loop closing's Sim3 searches (src/ORBmatcher.cc:496-619, :621-733, :1547-1676; called from
    // src/LoopClosing.cc:976, :1005, :1265, :2712, :2765), through orb_sim3_projection.  S is the Sim3 type
    // (Sophus::Sim3f); accessor members used besides those of Fuse:
    //   static void Sim3Pose(const S& Scw, float Tcw[12], float Ow[3]);   // the reference's two Sophus lines,
    //       verbatim: Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) as 3x4 row-major
    //       [R | t], Ow = Tcw.inverse().translation() -- so that Sophus's arithmetic stays the reference's
    //   static std::set<MapPoint*> MapPointSet(KeyFrame*);                // GetMapPoints() (Fuse's spAlreadyFound)
    // The shim builds skip = isBad() || spAlreadyFound.count(pMP) and taken0 = vpMatched[idx] != NULL, writes
    // vpMatched / vpMatchedKF from matched[] and returns nmatches.  On a failure: 0, nothing written.
    template <class S>
    int SearchByProjection(KeyFrame* pKF, S& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched,
                           int th, float ratioHamming = 1.0f) {
        std::vector<Sim3Call> calls{MakeCall(pKF, Scw, &vpPoints, &vpMatched, ORB_S3P_CLAIM_PROJECT, (float)th, ratioHamming)};
        Sim3Result r;
        if (!RunSim3(calls, r)) return 0;
        for (size_t j = 0; j < vpMatched.size(); ++j)
            if (r.Matched(0, j) >= 0) vpMatched[j] = vpPoints[r.Matched(0, j)];
        return r.nmatches[0];
    }
    template <class S>
    int SearchByProjection(KeyFrame* pKF, S& Scw, const std::vector<MapPoint*>& vpPoints,
                           const std::vector<KeyFrame*>& vpPointsKFs, std::vector<MapPoint*>& vpMatched,
                           std::vector<KeyFrame*>& vpMatchedKF, int th, float ratioHamming = 1.0f) {
        if (vpPointsKFs.size() != vpPoints.size() || vpMatchedKF.size() != vpMatched.size())
            return ShimArgError("SearchByProjection: vpPointsKFs / vpMatchedKF sizes differ from vpPoints / vpMatched");
        std::vector<Sim3Call> calls{MakeCall(pKF, Scw, &vpPoints, &vpMatched, ORB_S3P_CLAIM_INVZ, (float)th, ratioHamming)};
        Sim3Result r;
        if (!RunSim3(calls, r)) return 0;
        for (size_t j = 0; j < vpMatched.size(); ++j)
            if (r.Matched(0, j) >= 0) {
                vpMatched[j] = vpPoints[r.Matched(0, j)];
                vpMatchedKF[j] = vpPointsKFs[r.Matched(0, j)];
            }
        return r.nmatches[0];
    }
    // B calls of the first form in one launch (the candidate loop of DetectCommonRegionsFromBoW, the covisible
    // keyframes of FindMatchesByProjection's verification): job b is SearchByProjection(vJobs[b].first,
    // vJobs[b].second, vvpPoints[b], vvpMatched[b], th, ratioHamming).  The calls read no state another call
    // writes (each has its own vpMatched), so the batch equals the sequence.  vnMatches[b] = its return value.
    template <class S>
    void SearchByProjection(const std::vector<std::pair<KeyFrame*, S>>& vJobs, const std::vector<std::vector<MapPoint*>>& vvpPoints,
                            std::vector<std::vector<MapPoint*>>& vvpMatched, int th, float ratioHamming,
                            std::vector<int>& vnMatches) {
        SearchByProjectionBatch<S>(vJobs, vvpPoints, nullptr, vvpMatched, nullptr, th, ratioHamming, vnMatches);
    }
    // The same for the second form (vvpPointsKFs[b], vvpMatchedKF[b]).
    template <class S>
    void SearchByProjection(const std::vector<std::pair<KeyFrame*, S>>& vJobs, const std::vector<std::vector<MapPoint*>>& vvpPoints,
                            const std::vector<std::vector<KeyFrame*>>& vvpPointsKFs, std::vector<std::vector<MapPoint*>>& vvpMatched,
                            std::vector<std::vector<KeyFrame*>>& vvpMatchedKF, int th, float ratioHamming,
                            std::vector<int>& vnMatches) {
        SearchByProjectionBatch<S>(vJobs, vvpPoints, &vvpPointsKFs, vvpMatched, &vvpMatchedKF, th, ratioHamming, vnMatches);
    }

    // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1547-1676): the search on the device, then step 7
    // (:1655-1672) here in point order with GetMapPoint(bestIdx) as it stands at that moment -- a keypoint an
    // earlier point's AddMapPoint filled makes a later point a replacement, as upstream.
    template <class S>
    int Fuse(KeyFrame* pKF, S& Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint) {
        std::vector<std::vector<MapPoint*>*> rep{&vpReplacePoint};
        std::vector<int> n;
        FuseBatch<S>({{pKF, Scw}}, vpPoints, th, rep, n);
        return n[0];
    }
    // SearchAndFuse's loop over the corrected keyframes (src/LoopClosing.cc:2697-2740) in one launch: job b is
    // Fuse(vJobs[b].first, vJobs[b].second, vpPoints, th, vvpReplacePoint[b]).  The keyframes must be distinct:
    // a call's search reads, of the state a Fuse call writes, only its own keyframe's map points.
    template <class S>
    void Fuse(const std::vector<std::pair<KeyFrame*, S>>& vJobs, const std::vector<MapPoint*>& vpPoints, float th,
              std::vector<std::vector<MapPoint*>>& vvpReplacePoint, std::vector<int>& vnFused) {
        std::vector<std::vector<MapPoint*>*> rep;
        if (vvpReplacePoint.size() != vJobs.size()) {
            vnFused.assign(vJobs.size(), 0);
            ShimArgError("Fuse: one vpReplacePoint per job");
            return;
        }
        for (auto& v : vvpReplacePoint) rep.push_back(&v);
        FuseBatch<S>(vJobs, vpPoints, th, rep, vnFused);
    }

    // The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:603-910) for the neighbours
    // that passed the caller's baseline / median-depth pre-tests (:575-601): the batched
    // orb_search_for_triangulation, then orb_create_new_map_points on its matches, then step 6 (:888-909)
    // here, through the access policy, in the order of the records (upstream's creation order):
    //   pass 1, per record: NewMapPoint(x3d, pKF1), AddObservation(pMP, pKF1, idx1), AddObservation(pMP, pKF2,
    //           idx2), AddMapPoint(pKF1, pMP, idx1), AddMapPoint(pKF2, pMP, idx2) -- two records of one
    //           neighbour may share idx2: the later AddMapPoint overwrites, as upstream's does;
    //   one batched ComputeDistinctiveDescriptors for all new points (a point's result depends on its own
    //           observations only, so the batch equals upstream's per-point calls);
    //   pass 2, per record: SetNormalAndDepth(pMP, normal, min_dist, max_dist) -- UpdateNormalAndDepth's
    //           result for the two observations, from the record -- then `added(pMP)`, the caller's
    //           mpAtlas->AddMapPoint(pMP) and mlpRecentAddedMapPoints.push_back(pMP).
    // Returns the new map points in creation order (`records`, when given, receives their records).  A
    // failing entry mutates nothing and returns no points.  A caller that honours CheckNewKeyFrames() (:568)
    // between neighbours passes the neighbours it is willing to finish.  Accessor members used besides
    // those of SearchForTriangulation:
    //   static void NewPointsGeometry(KeyFrame*, orb_newpoints_kf_extra_t*);  // pose, Ow, mb, mbf, invfx/y, mvDepth, mvKeys
    //   static MapPoint* NewMapPoint(const float x3d[3], KeyFrame* pRefKF);   // new MapPoint(x3D, pKF, map)
    //   static void SetNormalAndDepth(MapPoint*, const float normal[3], float min_dist, float max_dist);
    struct NewPointsParams {
        bool inertial = false;        // mbInertial
        bool far_points = false;      // mbFarPoints
        float th_far_points = 0.f;    // mThFarPoints
        float ratio_factor = 1.8f;    // 1.5f * pKF1->mfScaleFactor
        bool coarse = false;          // bCoarse of the search (:607)
    };
    std::vector<MapPoint*> CreateNewMapPoints(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2,
                                              const NewPointsParams& prm,
                                              const std::function<void(MapPoint*)>& added = nullptr,
                                              std::vector<orb_newpoint_t>* records = nullptr) {
        std::vector<MapPoint*> created;
        if (records) records->clear();
        const size_t p = vpKF2.size();
        if (p == 0) return created;
        detail::KfViewStore<A> v1(pKF1);
        std::vector<std::unique_ptr<detail::KfViewStore<A>>> v2;
        std::vector<orb_kf_view_t> views(p);
        std::vector<orb_kf_pair_geom_t> geoms(p);
        std::vector<orb_newpoints_kf_t> nk(p);
        orb_newpoints_kf_t nk1{};
        nk1.view = v1.view;
        A::NewPointsGeometry(pKF1, &nk1.extra);
        for (size_t i = 0; i < p; ++i) {
            v2.emplace_back(new detail::KfViewStore<A>(vpKF2[i]));
            views[i] = v2.back()->view;
            geoms[i] = A::PairGeometry(pKF1, vpKF2[i]);
            nk[i] = orb_newpoints_kf_t{};
            nk[i].view = views[i];
            A::NewPointsGeometry(vpKF2[i], &nk[i].extra);
        }
        const int n1 = v1.view.n;
        const size_t C = n1 > 0 ? (size_t)n1 : 1;
        std::vector<int32_t> m12(p * C, -1), cnt(p, 0);
        if (Failed(orb_search_for_triangulation(Handle(), &v1.view, views.data(), geoms.data(), (int)p, 0,
                                                prm.coarse ? 1 : 0, m12.data(), cnt.data()),
                   "orb_search_for_triangulation"))
            return created;
        std::vector<int32_t> status(p * C), taken(C);
        std::vector<float> x3d(3 * p * C);
        std::vector<uint8_t> from_stereo(p * C);
        std::vector<orb_newpoint_t> rec(C);
        int32_t n_new = 0;
        const orb_newpoints_params_t prms{prm.inertial ? 1 : 0, prm.far_points ? 1 : 0, prm.th_far_points, prm.ratio_factor};
        const orb_newpoints_out_t out{status.data(), x3d.data(), from_stereo.data(), taken.data(), rec.data(), &n_new};
        if (Failed(orb_create_new_map_points(Handle(), &nk1, nk.data(), (int)p, &prms, m12.data(), cnt.data(), &out),
                   "orb_create_new_map_points"))
            return created;
        if (n_new < 0 || (size_t)n_new > C) return created;
        for (int r = 0; r < n_new; ++r) {  // (a conforming library reports none of these: nothing is mutated)
            const orb_newpoint_t& q = rec[r];
            if (q.p < 0 || (size_t)q.p >= p || q.idx1 < 0 || q.idx1 >= n1 || q.idx2 < 0 || q.idx2 >= views[q.p].n) {
                Failed(ORB_ERR_INTERNAL, "orb_create_new_map_points (record out of range)");
                return created;
            }
        }
        created.reserve(n_new);
        for (int r = 0; r < n_new; ++r) {  // pass 1 (:888-898)
            const orb_newpoint_t& q = rec[r];
            KeyFrame* pKF2 = vpKF2[q.p];
            MapPoint* pMP = A::NewMapPoint(q.x3d, pKF1);
            A::AddObservation(pMP, pKF1, q.idx1);
            A::AddObservation(pMP, pKF2, q.idx2);
            A::AddMapPoint(pKF1, pMP, q.idx1);
            A::AddMapPoint(pKF2, pMP, q.idx2);
            created.push_back(pMP);
        }
        orbgpu::ComputeDistinctiveDescriptors<A>(created);  // (:901), one launch
        for (int r = 0; r < n_new; ++r) {  // pass 2 (:904-909)
            A::SetNormalAndDepth(created[r], rec[r].normal, rec[r].min_dist, rec[r].max_dist);
            if (added) added(created[r]);
        }
        if (records) records->assign(rec.begin(), rec.begin() + n_new);
        return created;
    }

    float mfNNratio;
    bool mbCheckOrientation;

private:
    orb_matcher_t Handle() const { return detail::ThreadHandle(mfNNratio, mbCheckOrientation); }

    // SearchByBoW(pKF1, kfs[p], vv[p]) for every p (all non-NULL): vpMatches12[idx1] = vpMapPoints2[bestIdx2] (:990)
    bool SearchByBoWPairs(KeyFrame* pKF1, const std::vector<KeyFrame*>& kfs, std::vector<std::vector<MapPoint*>>& vv,
                          std::vector<int>& n) {
        const size_t n_mp1 = A::MapPointMatches(pKF1).size();  // :907
        vv.assign(kfs.size(), std::vector<MapPoint*>(n_mp1, static_cast<MapPoint*>(nullptr)));
        n.assign(kfs.size(), 0);
        std::vector<int32_t> rows, counts;
        if (!SearchByBoWIndices(pKF1, kfs, rows, counts)) return false;
        const int n1 = A::N(pKF1);
        for (size_t p = 0; p < kfs.size(); ++p) {
            const std::vector<MapPoint*> mps2 = A::MapPointMatches(kfs[p]);
            for (int i = 0; i < n1 && i < (int)n_mp1; ++i) {
                const int32_t j = rows[p * (size_t)n1 + i];
                if (j >= 0 && j < (int)mps2.size()) vv[p][i] = mps2[j];
            }
            n[p] = counts[p];
        }
        return true;
    }
    static bool Failed(int rc, const char* what) { return detail::Failed(rc, what); }

    // one call of a reference Sim3 search, as orb_sim3_projection takes it
    struct Sim3Call {
        KeyFrame* kf;
        const std::vector<MapPoint*>* points;
        const std::vector<MapPoint*>* matched;  // vpMatched (claim forms), NULL for Fuse
        orb_sim3_projection_job_t job;
    };
    struct Sim3Result {
        int stride = 1;
        std::vector<int32_t> matched, nmatches, best_idx, offsets;
        int32_t Matched(size_t b, size_t j) const { return j < (size_t)stride ? matched[b * stride + j] : -1; }
    };
    static int ShimArgError(const char* what) {
        detail::Failed(ORB_ERR_ARG, what);
        return 0;
    }
    template <class S>
    static Sim3Call MakeCall(KeyFrame* pKF, const S& Scw, const std::vector<MapPoint*>* points,
                             const std::vector<MapPoint*>* matched, int mode, float th, float ratio) {
        Sim3Call c{pKF, points, matched, {}};
        c.job.mode = mode;
        c.job.th = th;
        c.job.ratio_hamming = ratio;
        A::Sim3Pose(Scw, c.job.Tcw, c.job.Ow);
        return c;
    }
    // Distinct keyframes and point vectors are sent once; skip and taken0 as the reference's loops read them.
    bool RunSim3(std::vector<Sim3Call>& calls, Sim3Result& r) {
        const size_t B = calls.size();
        r.nmatches.assign(B, 0);
        r.offsets.assign(B + 1, 0);
        if (B == 0) return true;
        std::vector<KeyFrame*> kf_list;
        std::map<KeyFrame*, int> kf_index;
        std::vector<const std::vector<MapPoint*>*> pt_list;
        std::map<const std::vector<MapPoint*>*, int> pt_first;
        std::vector<MapPoint*> pool;
        for (Sim3Call& c : calls) {
            if (!c.kf || !A::SingleCamera(c.kf)) {
                ShimArgError("Sim3 search: null or two-camera keyframe");
                return false;
            }
            if (c.matched && (int)c.matched->size() != A::N(c.kf)) {
                ShimArgError("Sim3 search: vpMatched.size() != N");
                return false;
            }
            if (!kf_index.count(c.kf)) {
                kf_index[c.kf] = (int)kf_list.size();
                kf_list.push_back(c.kf);
            }
            if (!pt_first.count(c.points)) {
                pt_first[c.points] = (int)pool.size();
                pool.insert(pool.end(), c.points->begin(), c.points->end());
            }
            c.job.kf = kf_index[c.kf];
            c.job.first = pt_first[c.points];
            c.job.count = (int32_t)c.points->size();
            r.stride = std::max(r.stride, A::N(c.kf));
        }
        std::vector<orb_sim3_projection_kf_t> views(kf_list.size());
        for (size_t k = 0; k < kf_list.size(); ++k) {
            const detail::FuseKfStore<A> st(kf_list[k]);
            views[k].frame = st.view.frame;
            views[k].log_scale_factor = st.view.log_scale_factor;
        }
        const detail::FusePointStore<A> sent(pool);
        for (size_t b = 0; b < B; ++b) r.offsets[b + 1] = r.offsets[b] + calls[b].job.count;
        const size_t T = (size_t)r.offsets[B];
        std::vector<uint8_t> skip(std::max<size_t>(T, 1), 0), taken0(B * r.stride, 0);
        std::vector<orb_sim3_projection_job_t> jobs(B);
        for (size_t b = 0; b < B; ++b) {
            const Sim3Call& c = calls[b];
            jobs[b] = c.job;
            std::set<MapPoint*> found;                       // spAlreadyFound (:513-514 / :1562)
            if (c.matched) {
                found.insert(c.matched->begin(), c.matched->end());
                found.erase(static_cast<MapPoint*>(nullptr));
                for (size_t j = 0; j < c.matched->size(); ++j) taken0[b * r.stride + j] = (*c.matched)[j] ? 1 : 0;
            } else {
                found = A::MapPointSet(c.kf);
            }
            for (size_t i = 0; i < c.points->size(); ++i)    // :526 / :1576 (a NULL point is skipped, not dereferenced)
                skip[r.offsets[b] + i] = sent.dead[c.job.first + i] || found.count((*c.points)[i]) ? 1 : 0;
        }
        r.matched.assign(B * r.stride, -1);
        r.best_idx.assign(std::max<size_t>(T, 1), -1);
        return !Failed(orb_sim3_projection(Handle(), views.data(), (int)views.size(), jobs.data(), (int)B, &sent.view,
                                           skip.data(), taken0.data(), r.stride, r.matched.data(), r.nmatches.data(),
                                           r.best_idx.data(), nullptr),
                       "orb_sim3_projection");
    }
    template <class S>
    void SearchByProjectionBatch(const std::vector<std::pair<KeyFrame*, S>>& vJobs,
                                 const std::vector<std::vector<MapPoint*>>& vvpPoints,
                                 const std::vector<std::vector<KeyFrame*>>* vvpPointsKFs,
                                 std::vector<std::vector<MapPoint*>>& vvpMatched, std::vector<std::vector<KeyFrame*>>* vvpMatchedKF,
                                 int th, float ratioHamming, std::vector<int>& vnMatches) {
        const size_t B = vJobs.size();
        vnMatches.assign(B, 0);
        bool ok = vvpPoints.size() == B && vvpMatched.size() == B &&
                  (!vvpPointsKFs || (vvpPointsKFs->size() == B && vvpMatchedKF && vvpMatchedKF->size() == B));
        for (size_t b = 0; ok && vvpPointsKFs && b < B; ++b)
            ok = (*vvpPointsKFs)[b].size() == vvpPoints[b].size() && (*vvpMatchedKF)[b].size() == vvpMatched[b].size();
        if (!ok) {
            ShimArgError("SearchByProjection: one point / match vector per job, of matching sizes");
            return;
        }
        std::vector<Sim3Call> calls;
        for (size_t b = 0; b < B; ++b)
            calls.push_back(MakeCall(vJobs[b].first, vJobs[b].second, &vvpPoints[b], &vvpMatched[b],
                                     vvpPointsKFs ? ORB_S3P_CLAIM_INVZ : ORB_S3P_CLAIM_PROJECT, (float)th, ratioHamming));
        Sim3Result r;
        if (!RunSim3(calls, r)) return;
        for (size_t b = 0; b < B; ++b) {
            for (size_t j = 0; j < vvpMatched[b].size(); ++j) {
                const int32_t i = r.Matched(b, j);
                if (i < 0) continue;
                vvpMatched[b][j] = vvpPoints[b][i];
                if (vvpPointsKFs) (*vvpMatchedKF)[b][j] = (*vvpPointsKFs)[b][i];
            }
            vnMatches[b] = r.nmatches[b];
        }
    }
    template <class S>
    void FuseBatch(const std::vector<std::pair<KeyFrame*, S>>& vJobs, const std::vector<MapPoint*>& vpPoints, float th,
                   const std::vector<std::vector<MapPoint*>*>& rep, std::vector<int>& vnFused) {
        const size_t B = vJobs.size(), n = vpPoints.size();
        vnFused.assign(B, 0);
        std::set<KeyFrame*> distinct;
        for (size_t b = 0; b < B; ++b) {
            distinct.insert(vJobs[b].first);
            if (rep[b]->size() != n) {
                ShimArgError("Fuse: vpReplacePoint.size() != vpPoints.size()");
                return;
            }
        }
        if (distinct.size() != B) {
            ShimArgError("Fuse: the keyframes of a batch must be distinct");
            return;
        }
        std::vector<Sim3Call> calls;
        for (size_t b = 0; b < B; ++b) calls.push_back(MakeCall(vJobs[b].first, vJobs[b].second, &vpPoints, nullptr, ORB_S3P_FUSE, th, 1.0f));
        Sim3Result r;
        if (!RunSim3(calls, r)) return;
        for (size_t b = 0; b < B; ++b) {
            KeyFrame* pKF = vJobs[b].first;
            int nFused = 0;
            for (size_t iMP = 0; iMP < n; ++iMP) {  // step 7 (:1655-1672)
                const int32_t bestIdx = r.best_idx[r.offsets[b] + iMP];
                if (bestIdx < 0) continue;
                MapPoint* pMP = vpPoints[iMP];
                MapPoint* pMPinKF = A::GetMapPoint(pKF, bestIdx);
                if (pMPinKF) {
                    if (!A::IsBad(pMPinKF)) (*rep[b])[iMP] = pMPinKF;
                } else {
                    A::AddObservation(pMP, pKF, bestIdx);
                    A::AddMapPoint(pKF, pMP, bestIdx);
                }
                ++nFused;
            }
            vnFused[b] = nFused;
        }
    }
};

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-529) for a batch of map points in one
// launch, e.g. the loops of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1045-1060) and
// ProcessNewKeyFrame (:400-416): each point's result depends only on its own observations, so the
// batch equals the per-point calls.  Per point, as the reference: skipped when bad or without
// observations; rows = the observations in std::map order, left then right index, bad keyframes
// skipped; skipped when no row; otherwise mDescriptor = the row with the least median distance.
// Accessor members used (besides those above):
//   static std::map<KeyFrame*, std::tuple<int, int>> ObservationMap(MapPoint*); // GetObservations()
//   static bool IsBad(KeyFrame*);
//   static const uint8_t* DescriptorRow(KeyFrame*, int idx);                    // mDescriptors.row(idx)
//   static void SetDescriptor(MapPoint*, const uint8_t d[32]);                  // mDescriptor = row.clone()
template <class A>
void ComputeDistinctiveDescriptors(const std::vector<typename A::MapPoint*>& points) {
    std::vector<uint8_t> rows;
    std::vector<int32_t> offsets{0};
    std::vector<typename A::MapPoint*> todo;
    for (auto* pMP : points) {
        if (!pMP || A::IsBad(pMP)) continue;
        const auto observations = A::ObservationMap(pMP);
        if (observations.empty()) continue;
        const size_t before = rows.size();
        for (const auto& ob : observations) {
            if (A::IsBad(ob.first)) continue;
            const int l = std::get<0>(ob.second), r = std::get<1>(ob.second);
            if (l != -1) rows.insert(rows.end(), A::DescriptorRow(ob.first, l), A::DescriptorRow(ob.first, l) + 32);
            if (r != -1) rows.insert(rows.end(), A::DescriptorRow(ob.first, r), A::DescriptorRow(ob.first, r) + 32);
        }
        if (rows.size() == before) continue;
        offsets.push_back((int32_t)(rows.size() / 32));
        todo.push_back(pMP);
    }
    if (todo.empty()) return;
    std::vector<int32_t> best(todo.size());
    std::vector<uint8_t> out(32 * todo.size());
    if (detail::Failed(orb_compute_distinctive_descriptors(detail::ThreadHandle(0.6f, false), rows.data(), offsets.data(),
                                                           (int)todo.size(), best.data(), out.data()),
                       "orb_compute_distinctive_descriptors"))
        return;  // descriptors left as they were
    for (size_t p = 0; p < todo.size(); ++p) A::SetDescriptor(todo[p], &out[32 * p]);
}

}  // namespace orbgpu

// ---- the reference's own types (compile inside the ORB-SLAM3 build: define ORBGPU_WITH_ORBSLAM3 and
// include after Frame.h, KeyFrame.h and MapPoint.h) ------------------------------------------------
#ifdef ORBGPU_WITH_ORBSLAM3
namespace orbgpu {

struct ORBSLAM3MatcherAccess {
    using KeyFrame = ORB_SLAM3::KeyFrame;
    using Frame = ORB_SLAM3::Frame;
    using MapPoint = ORB_SLAM3::MapPoint;
    static_assert(sizeof(cv::KeyPoint) == sizeof(orb_keypoint_t), "cv::KeyPoint layout");

    static int N(KeyFrame* k) { return k->N; }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return reinterpret_cast<const orb_keypoint_t*>(k->mvKeysUn.data()); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->mDescriptors.empty() ? nullptr : k->mDescriptors.ptr<uint8_t>(); }
    static const float* URight(KeyFrame* k) { return k->mvuRight.data(); }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->GetMapPointMatches(); }
    static const DBoW2::FeatureVector& FeatVec(KeyFrame* k) { return k->mFeatVec; }
    static void Pinhole(KeyFrame* k, float K[4]) {
        for (int i = 0; i < 4; ++i) K[i] = k->mpCamera->getParameter(i);  // Pinhole mvParameters: fx, fy, cx, cy
    }
    static int Levels(KeyFrame* k) { return k->mnScaleLevels; }
    static const float* ScaleFactors(KeyFrame* k) { return k->mvScaleFactors.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->mvLevelSigma2.data(); }
    static bool SingleCamera(KeyFrame* k) { return k->mpCamera2 == nullptr && k->NLeft == -1; }
    static orb_kf_pair_geom_t PairGeometry(KeyFrame* pKF1, KeyFrame* pKF2) {  // src/ORBmatcher.cc:1054-1072
        const Sophus::SE3f T1w = pKF1->GetPose(), T2w = pKF2->GetPose(), Tw2 = pKF2->GetPoseInverse();
        const Eigen::Vector3f C2 = T2w * pKF1->GetCameraCenter();
        const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
        const Sophus::SE3f T12 = T1w * Tw2;
        const Eigen::Matrix3f R12 = T12.rotationMatrix();
        const Eigen::Vector3f t12 = T12.translation();
        orb_kf_pair_geom_t g;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) g.R12[3 * r + c] = R12(r, c);
            g.t12[r] = t12(r);
        }
        g.ep[0] = ep(0);
        g.ep[1] = ep(1);
        return g;
    }

    static orb_frame_view_t View(const Frame& f) {
        orb_frame_view_t v{};
        v.n = f.N;
        v.kps_un = reinterpret_cast<const orb_keypoint_t*>(f.mvKeysUn.data());
        v.desc = f.mDescriptors.empty() ? nullptr : f.mDescriptors.ptr<uint8_t>();
        v.u_right = f.mvuRight.data();
        v.min_x = Frame::mnMinX; v.max_x = Frame::mnMaxX; v.min_y = Frame::mnMinY; v.max_y = Frame::mnMaxY;
        v.grid_inv_w = Frame::mfGridElementWidthInv;
        v.grid_inv_h = Frame::mfGridElementHeightInv;
        v.fx = f.fx; v.fy = f.fy; v.cx = f.cx; v.cy = f.cy;
        v.bf = f.mbf; v.b = f.mb;
        v.nlevels = f.mnScaleLevels;
        v.scale_factors = f.mvScaleFactors.data();
        const Eigen::Matrix<float, 3, 4> T = f.GetPose().matrix3x4();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) v.Tcw[4 * r + c] = T(r, c);
        return v;
    }
    static bool SingleCamera(const Frame& f) { return f.Nleft == -1 && f.mpCamera2 == nullptr; }
    static std::vector<MapPoint*>& MapPoints(Frame& f) { return f.mvpMapPoints; }
    static const std::vector<MapPoint*>& MapPoints(const Frame& f) { return f.mvpMapPoints; }
    static bool Outlier(const Frame& f, int i) { return f.mvbOutlier[i]; }
    static const DBoW2::FeatureVector& FeatVec(const Frame& f) { return f.mFeatVec; }

    static int Observations(MapPoint* p) { return p->Observations(); }
    static bool IsBad(MapPoint* p) { return p->isBad(); }
    static void WorldPos(MapPoint* p, float X[3]) {
        const Eigen::Vector3f x = p->GetWorldPos();
        X[0] = x(0); X[1] = x(1); X[2] = x(2);
    }
    static void Descriptor(MapPoint* p, uint8_t d[32]) {
        const cv::Mat m = p->GetDescriptor();
        for (int i = 0; i < 32; ++i) d[i] = m.ptr<uint8_t>()[i];
    }
    static std::map<KeyFrame*, std::tuple<int, int>> ObservationMap(MapPoint* p) { return p->GetObservations(); }
    static bool IsBad(KeyFrame* k) { return k->isBad(); }
    static const uint8_t* DescriptorRow(KeyFrame* k, int idx) { return k->mDescriptors.ptr<uint8_t>(idx); }
    // mDescriptor is protected in MapPoint: the integration adds `friend struct orbgpu::ORBSLAM3MatcherAccess;`
    static void SetDescriptor(MapPoint* p, const uint8_t d[32]) {
        std::unique_lock<std::mutex> lock(p->mMutexFeatures);
        p->mDescriptor = cv::Mat(1, 32, CV_8U, const_cast<uint8_t*>(d)).clone();
    }
    // Fuse (KeyFrame's bounds and grid inverses are public members; MapPoint's raw distances are
    // protected: the integration's friend declaration covers them, as for SetDescriptor)
    static void FuseGeometry(KeyFrame* k, orb_fuse_kf_t* v) {
        orb_frame_view_t& f = v->frame;
        f.min_x = k->mnMinX; f.max_x = k->mnMaxX; f.min_y = k->mnMinY; f.max_y = k->mnMaxY;
        f.grid_inv_w = k->mfGridElementWidthInv;
        f.grid_inv_h = k->mfGridElementHeightInv;
        f.bf = k->mbf; f.b = k->mb;
        const Eigen::Matrix<float, 3, 4> T = k->GetPose().matrix3x4();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) f.Tcw[4 * r + c] = T(r, c);
        const Eigen::Vector3f Ow = k->GetCameraCenter();
        for (int r = 0; r < 3; ++r) v->Ow[r] = Ow(r);
        v->inv_level_sigma2 = k->mvInvLevelSigma2.data();
        v->log_scale_factor = k->mfLogScaleFactor;
    }
    static MapPoint* GetMapPoint(KeyFrame* k, int idx) { return k->GetMapPoint(idx); }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->AddMapPoint(p, idx); }
    static bool IsInKeyFrame(MapPoint* p, KeyFrame* k) { return p->IsInKeyFrame(k); }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) { p->AddObservation(k, idx); }
    static void Replace(MapPoint* p, MapPoint* by) { p->Replace(by); }
    static void Normal(MapPoint* p, float n[3]) {
        const Eigen::Vector3f v = p->GetNormal();
        n[0] = v(0); n[1] = v(1); n[2] = v(2);
    }
    static float MinDistance(MapPoint* p) {
        std::unique_lock<std::mutex> lock(p->mMutexPos);
        return p->mfMinDistance;
    }
    static float MaxDistance(MapPoint* p) {
        std::unique_lock<std::mutex> lock(p->mMutexPos);
        return p->mfMaxDistance;
    }
    // Loop closing's Sim3 searches: the reference's two lines (src/ORBmatcher.cc:508-509), verbatim
    static void Sim3Pose(const Sophus::Sim3f& Scw, float Tcw[12], float Ow[3]) {
        Sophus::SE3f T = Sophus::SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
        Eigen::Vector3f O = T.inverse().translation();
        const Eigen::Matrix<float, 3, 4> M = T.matrix3x4();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) Tcw[4 * r + c] = M(r, c);
        for (int r = 0; r < 3; ++r) Ow[r] = O(r);
    }
    static std::set<MapPoint*> MapPointSet(KeyFrame* k) { return k->GetMapPoints(); }
    // CreateNewMapPoints (mfMinDistance / mfMaxDistance through the friend declaration, as above)
    static void NewPointsGeometry(KeyFrame* k, orb_newpoints_kf_extra_t* e) {
        const Eigen::Matrix<float, 3, 4> T = k->GetPose().matrix3x4();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) e->Tcw[4 * r + c] = T(r, c);
        const Eigen::Vector3f Ow = k->GetCameraCenter();
        for (int r = 0; r < 3; ++r) e->Ow[r] = Ow(r);
        e->mb = k->mb; e->mbf = k->mbf; e->invfx = k->invfx; e->invfy = k->invfy;
        e->depth = k->mvDepth.empty() ? nullptr : k->mvDepth.data();
        e->kps_raw = k->mvKeys.empty() ? nullptr : reinterpret_cast<const orb_keypoint_t*>(k->mvKeys.data());
    }
    static MapPoint* NewMapPoint(const float x3d[3], KeyFrame* pRefKF) {
        return new MapPoint(Eigen::Vector3f(x3d[0], x3d[1], x3d[2]), pRefKF, pRefKF->GetMap());
    }
    static void SetNormalAndDepth(MapPoint* p, const float n[3], float min_dist, float max_dist) {
        std::unique_lock<std::mutex> lock(p->mMutexPos);
        p->mfMaxDistance = max_dist;
        p->mfMinDistance = min_dist;
        p->mNormalVector = Eigen::Vector3f(n[0], n[1], n[2]);
    }
    static void Track(MapPoint* p, TrackFields* t) {
        t->in_view = p->mbTrackInView;
        t->proj[0] = p->mTrackProjX; t->proj[1] = p->mTrackProjY; t->proj[2] = p->mTrackProjXR;
        t->view_cos = p->mTrackViewCos;
        t->depth = p->mTrackDepth;
        t->level = p->mnTrackScaleLevel;
    }
};

using GpuORBmatcher = ORBmatcher<ORBSLAM3MatcherAccess>;

}  // namespace orbgpu
#endif  // ORBGPU_WITH_ORBSLAM3

#endif  // ORBGPU_MATCHER_HPP
