/*
 * orbgpu_sim3.hpp -- header-only drop-in for ORB_SLAM3::Sim3Solver (include/Sim3Solver.h:34-50,
 * src/Sim3Solver.cc) over the C ABI (orbgpu.h: orb_sim3_ransac):
 *
 *   Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, bool bFixScale = true,
 *              vector<KeyFrame*> vpKeyFrameMatchedMP = {})                                   (:31-121)
 *   void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)  (:123-147)
 *   Matrix4f iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)          (:149-216)
 *   Matrix4f iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers, bool& bConverge)
 *                                                                                                      (:218-294)
 *   Matrix4f find(vector<bool>& vbInliers12, int& nInliers)                                            (:296-300)
 *   GetEstimatedTransformation / Rotation / Translation / Scale                                        (:441-459)
 *   static void Batch(const vector<Sim3Solver*>&)   several constructed solvers in one library call: the
 *                                                   candidate loop of LoopClosing::DetectCommonRegionsFromBoW
 *   orbgpu::LoopBowProblems<A>(matcherBoW, pCurrentKF, vpCandidates, vvpCovKFi, bFixScale, out)
 *                                                   src/LoopClosing.cc:840-881 and the constructor's gather for a
 *                                                   list of candidates on the GPU (orb_search_by_bow_kf +
 *                                                   orb_loop_bow_problems): per candidate vpMatchedPoints,
 *                                                   vpKeyFrameMatchedMP, numBoWMatches and a ready Sim3Solver<A>
 *                                                   (needs A::IsBad(KeyFrame*))
 *
 * The hypotheses of a RANSAC do not depend on each other, so the first iterate() evaluates all mRansacMaxIts of
 * them in one library call; every iterate(n) then replays the reference's control flow over the returned counts:
 * it consumes the next n hypotheses, mnBestInliers and mnIterations persist across calls, and the bConverge
 * overload returns its own chunk's last best-so-far.
 *
 * ONE DIFFERENCE from the reference: all mRansacMaxIts triples are drawn up front, through A::RandomInt with the
 * reference's swap-with-back removal, three draws per iteration, in order.  Hypothesis h is therefore the
 * reference's iteration h for the same generator state, but a run that converges early has consumed more random
 * numbers than the reference would have: code that shares the generator sees a different stream afterwards.
 *
 * The object graph is reached through an accessor type A, so that the same code runs on the reference's classes
 * (orbgpu::ORBSLAM3Sim3Access below, compiled inside the reference build) and on a mock graph in this
 * repository's tests (tests/native/sim3_shim_check.cpp):
 *
 *   struct A {
 *     using KeyFrame = ...; using MapPoint = ...;
 *     using Matrix4f = ...; using Matrix3f = ...; using Vector3f = ...;     // what the reference returns
 *     static Matrix4f Matrix4(const float m[16]);  static Matrix3f Matrix3(const float m[9]);   // row-major
 *     static Vector3f Vector3(const float v[3]);
 *     static std::vector<MapPoint*> MapPointMatches(KeyFrame*);           // GetMapPointMatches()
 *     static bool IsBad(MapPoint*);   static bool IsBad(KeyFrame*);       // (the KeyFrame form: LoopBowProblems only)
 *     static int IndexInKeyFrame(MapPoint*, KeyFrame*);                   // get<0>(GetIndexInKeyFrame(pKF))
 *     static const orb_keypoint_t* KeysUn(KeyFrame*);  static const float* LevelSigma2(KeyFrame*);
 *     static void Pose(KeyFrame*, float Rcw[9], float tcw[3]);            // GetRotation(), GetTranslation()
 *     static void WorldPos(MapPoint*, float X[3]);
 *     static void Pinhole(KeyFrame*, float K[4]);                         // fx, fy, cx, cy of mpCamera
 *     static int RandomInt(int min, int max);                             // DUtils::Random::RandomInt
 *   };
 *
 * Scope: pinhole cameras.  GetEstimatedRotation returns [s R] / s in float (the library reports s R and s),
 * within an ulp of the reference's mR12i.
 *
 * Failures (orbgpu_status.hpp): nothing here throws.  When the library call fails, iterate() returns what the
 * reference returns when its iterations run out without a model -- the identity, bNoMore = true, nInliers = 0,
 * vbInliers all false -- and orbgpu::LastShimError() reports the code.  Fewer than three correspondences (the
 * reference would index an empty list) are treated the same way without an error.
 */
#ifndef ORBGPU_SIM3_HPP
#define ORBGPU_SIM3_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <vector>

#include "orbgpu.h"
#include "orbgpu_status.hpp"

namespace orbgpu {

template <class A>
class Sim3Solver {
public:
    using KeyFrame = typename A::KeyFrame;
    using MapPoint = typename A::MapPoint;
    using Matrix4f = typename A::Matrix4f;
    using Matrix3f = typename A::Matrix3f;
    using Vector3f = typename A::Vector3f;

    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true,
               std::vector<KeyFrame*> vpKeyFrameMatchedMP = std::vector<KeyFrame*>())
        : mbFixScale(bFixScale) {
        // The reference names this flag bDifferentKFs and sets it when NO list was passed, then reads the list
        // only under the flag: a list that was passed is never read, and every match is looked up in pKF2.
        bool use_list = false;
        if (vpKeyFrameMatchedMP.empty()) {
            use_list = true;
            vpKeyFrameMatchedMP.assign(vpMatched12.size(), pKF2);
        }
        const std::vector<MapPoint*> vpKeyFrameMP1 = A::MapPointMatches(pKF1);
        mN1 = (int)vpMatched12.size();
        float R1[9], t1[3], R2[9], t2[3];
        A::Pose(pKF1, R1, t1);
        A::Pose(pKF2, R2, t2);
        KeyFrame* pKFm = pKF2;
        for (int i1 = 0; i1 < mN1; ++i1) {
            MapPoint* pMP2 = vpMatched12[i1];
            if (!pMP2) continue;
            MapPoint* pMP1 = vpKeyFrameMP1[i1];
            if (!pMP1) continue;
            if (A::IsBad(pMP1) || A::IsBad(pMP2)) continue;
            if (use_list) pKFm = vpKeyFrameMatchedMP[i1];
            const int indexKF1 = A::IndexInKeyFrame(pMP1, pKF1), indexKF2 = A::IndexInKeyFrame(pMP2, pKFm);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            const float sigma1 = A::LevelSigma2(pKF1)[A::KeysUn(pKF1)[indexKF1].octave];
            const float sigma2 = A::LevelSigma2(pKFm)[A::KeysUn(pKFm)[indexKF2].octave];
            mvnMaxError1.push_back((float)(9.210 * sigma1));
            mvnMaxError2.push_back((float)(9.210 * sigma2));
            mvnIndices1.push_back(i1);
            float X[3];
            A::WorldPos(pMP1, X);
            PushCamera(R1, t1, X, mvX3Dc1);
            A::WorldPos(pMP2, X);
            PushCamera(R2, t2, X, mvX3Dc2);
        }
        A::Pinhole(pKF1, mCam1);
        A::Pinhole(pKF2, mCam2);
        SetRansacParameters();
    }

    // A solver over correspondences the library gathered (orb_loop_bow_problems; LoopBowProblems below): n1 =
    // vpMatched12.size(), then the n entries of mvnIndices1, mvX3Dc1 / 2 and mvnMaxError1 / 2 in order.
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, int n1, int n, const int32_t* idx1, const float* x3dc1, const float* x3dc2,
               const float* max_err1, const float* max_err2, const bool bFixScale)
        : mbFixScale(bFixScale), mN1(n1) {
        mvnIndices1.assign(idx1, idx1 + n);
        mvX3Dc1.assign(x3dc1, x3dc1 + 3 * (size_t)n);
        mvX3Dc2.assign(x3dc2, x3dc2 + 3 * (size_t)n);
        mvnMaxError1.assign(max_err1, max_err1 + n);
        mvnMaxError2.assign(max_err2, max_err2 + n);
        A::Pinhole(pKF1, mCam1);
        A::Pinhole(pKF2, mCam2);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        const float epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) nIterations = 1;
        else {
            // (N < minInliers gives a NaN here, which the reference's cast turns into a negative count and the
            // clamp below into 1; such a solver never iterates anyway)
            const double its = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3)));
            nIterations = std::isnan(its) ? 1 : its > (double)mRansacMaxIts ? mRansacMaxIts : (int)its;
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
        mState = kPending;  // (the hypotheses follow mRansacMaxIts and the minimum: evaluated again)
    }

    Matrix4f iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bool bConverge;
        int chunk_best;
        const int h = Replay(nIterations, bNoMore, vbInliers, nInliers, bConverge, chunk_best);
        return h >= 0 ? Transformation(h) : Identity();
    }

    Matrix4f iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
        int chunk_best;
        const int h = Replay(nIterations, bNoMore, vbInliers, nInliers, bConverge, chunk_best);
        if (h >= 0) return Transformation(h);
        // the reference returns its local bestSim3, uninitialised when the chunk improved on nothing (and on the
        // early bNoMore return the identity): the identity stands in for both
        return chunk_best >= 0 ? Transformation(chunk_best) : Identity();
    }

    Matrix4f find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // mBestT12 and its parts: of the last hypothesis that set the best so far (zero-initialised before one did,
    // where the reference's members are uninitialised)
    Matrix4f GetEstimatedTransformation() { return mnBest >= 0 ? Transformation(mnBest) : A::Matrix4(kZero16()); }
    Matrix3f GetEstimatedRotation() {
        float R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (mnBest >= 0)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) R[3 * r + c] = mT12[12 * mnBest + 4 * r + c] / mScale[mnBest];
        return A::Matrix3(R);
    }
    Vector3f GetEstimatedTranslation() {
        float t[3] = {0, 0, 0};
        if (mnBest >= 0)
            for (int r = 0; r < 3; ++r) t[r] = mT12[12 * mnBest + 4 * r + 3];
        return A::Vector3(t);
    }
    float GetEstimatedScale() { return mnBest >= 0 ? mScale[mnBest] : 0.f; }

    // Evaluate every solver of the list that has not been evaluated yet in ONE library call (the triples are
    // drawn solver by solver, in list order).  Their iterate() calls then only replay.
    static void Batch(const std::vector<Sim3Solver*>& solvers) {
        std::vector<Sim3Solver*> todo;
        for (Sim3Solver* s : solvers)
            if (s && s->mState == kPending && s->Prepare()) todo.push_back(s);
        if (todo.empty()) return;
        std::vector<orb_sim3_problem_t> probs(todo.size());
        std::vector<orb_sim3_out_t> outs(todo.size());
        for (size_t k = 0; k < todo.size(); ++k) todo[k]->Describe(&probs[k], &outs[k]);
        const bool failed = detail::Failed(orb_sim3_ransac(probs.data(), (int)todo.size(), outs.data()), "orb_sim3_ransac");
        for (Sim3Solver* s : todo) s->mState = failed ? kFailed : kReady;
    }

    // (for tests and callers that want the whole table)
    int Iterations() const { return mnIterations; }
    int MaxIterations() const { return mRansacMaxIts; }
    int Correspondences() const { return N; }
    const std::vector<int>& Indices1() const { return mvnIndices1; }
    const std::vector<float>& X3Dc1() const { return mvX3Dc1; }
    const std::vector<float>& X3Dc2() const { return mvX3Dc2; }
    const std::vector<float>& MaxError1() const { return mvnMaxError1; }
    const std::vector<float>& MaxError2() const { return mvnMaxError2; }
    const std::vector<int32_t>& Samples() const { return mSamples; }
    const std::vector<int32_t>& HypothesisInliers() const { return mCounts; }

private:
    enum State { kPending, kReady, kFailed, kEmpty };

    static const float* kZero16() {
        static const float z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        return z;
    }
    static Matrix4f Identity() {
        const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        return A::Matrix4(I);
    }
    Matrix4f Transformation(int h) const {
        float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        for (int k = 0; k < 12; ++k) T[k] = mT12[12 * h + k];
        return A::Matrix4(T);
    }
    // Rcw * X + tcw as Eigen's fixed-size product evaluates it: each row's three products summed in order
    static void PushCamera(const float R[9], const float t[3], const float X[3], std::vector<float>& out) {
        for (int r = 0; r < 3; ++r) out.push_back(((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r]);
    }

    // Draw the triples and size the outputs; false when there is nothing to evaluate.
    bool Prepare() {
        if (N < mRansacMinInliers || N < 3) {
            mState = kEmpty;
            return false;
        }
        const int H = mRansacMaxIts;
        mSamples.resize(3 * (size_t)H);
        std::vector<int> all(N), avail;
        for (int i = 0; i < N; ++i) all[i] = i;
        for (int h = 0; h < H; ++h) {
            avail = all;
            for (int k = 0; k < 3; ++k) {
                const int randi = A::RandomInt(0, (int)avail.size() - 1);
                mSamples[3 * h + k] = avail[randi];
                avail[randi] = avail.back();
                avail.pop_back();
            }
        }
        mWords = (N + 63) / 64;
        mCounts.assign(H, 0);
        mT12.assign(12 * (size_t)H, 0.f);
        mScale.assign(H, 0.f);
        mMask.assign((size_t)H * mWords, 0);
        mWinnerMask.assign(N, 0);
        return true;
    }
    void Describe(orb_sim3_problem_t* p, orb_sim3_out_t* o) {
        p->n = N;
        p->x3dc1 = mvX3Dc1.data(); p->x3dc2 = mvX3Dc2.data();
        p->max_err1 = mvnMaxError1.data(); p->max_err2 = mvnMaxError2.data();
        for (int k = 0; k < 4; ++k) {
            p->cam1[k] = mCam1[k];
            p->cam2[k] = mCam2[k];
        }
        p->fix_scale = mbFixScale ? 1 : 0;
        p->min_inliers = mRansacMinInliers;
        p->n_hyp = mRansacMaxIts;
        p->samples = mSamples.data();
        o->hyp_inliers = mCounts.data(); o->hyp_t12 = mT12.data(); o->hyp_scale = mScale.data();
        o->winner = &mWinner; o->best = &mBestOfAll;
        o->inlier_mask = mWinnerMask.data();
        // the whole table: iterate() may be called again after a convergence, and the replay then needs the
        // rows of later hypotheses (300 x 4 words for 200 correspondences)
        o->hyp_mask = mMask.data();
    }

    // The reference's loop over the counts.  Returns the converged hypothesis or -1.
    int Replay(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge,
               int& chunk_best) {
        bNoMore = false;
        bConverge = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        chunk_best = -1;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return -1;
        }
        if (mState == kPending) Batch(std::vector<Sim3Solver*>(1, this));
        if (mState != kReady) {  // the library failed, or fewer than three correspondences
            bNoMore = true;
            return -1;
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            const int h = mnIterations;
            nCurrentIterations++;
            mnIterations++;
            const int mnInliersi = mCounts[h];
            if (mnInliersi >= mnBestInliers) {
                mnBestInliers = mnInliersi;
                mnBest = h;
                if (mnInliersi > mRansacMinInliers) {
                    nInliers = mnInliersi;
                    for (int i = 0; i < N; ++i)
                        if ((mMask[(size_t)h * mWords + (i >> 6)] >> (i & 63)) & 1u) vbInliers[mvnIndices1[i]] = true;
                    bConverge = true;
                    return h;
                }
                chunk_best = h;
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return -1;
    }

    // the gather (names as the reference's members)
    bool mbFixScale;
    int mN1 = 0, N = 0;
    std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
    std::vector<int> mvnIndices1;
    float mCam1[4], mCam2[4];
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    int mnIterations = 0, mnBestInliers = 0, mnBest = -1;
    // the evaluation
    State mState = kPending;
    int mWords = 0;
    std::vector<int32_t> mSamples, mCounts;
    std::vector<float> mT12, mScale;
    std::vector<uint64_t> mMask;
    std::vector<uint8_t> mWinnerMask;
    int32_t mWinner = -1, mBestOfAll = -1;
};

// What src/LoopClosing.cc:817-899 builds for one candidate.
template <class A>
struct LoopBowCandidate {
    std::vector<typename A::MapPoint*> vpMatchedPoints;      // :831, by the current keyframe's feature
    std::vector<typename A::KeyFrame*> vpKeyFrameMatchedMP;  // :833
    int numBoWMatches = 0;                                   // :822: distinct points, not filled slots
    std::vector<int> vnMatches;                              // SearchByBoW's return value per window keyframe (:845)
    std::unique_ptr<Sim3Solver<A>> solver;  // Sim3Solver(mpCurrentKF, pKFi, vpMatchedPoints, bFixScale,
                                            // vpKeyFrameMatchedMP) (:899), gathered on the GPU; NULL on a failure
};

// src/LoopClosing.cc:840-881 and the Sim3Solver constructor's gather (src/Sim3Solver.cc:71-118) for every
// candidate of the current keyframe in two library calls: vvpCovKFi[c] is candidate c's window (entries NULL or
// isBad() are skipped as at :842), vpCandidates[c] the keyframe whose pose and camera the solver takes
// (pMostBoWMatchesKF = pKFi, :825).  Every candidate gets a solver, whatever numBoWMatches is: the gate of :889
// stays with the caller, who then calls SetRansacParameters and iterate (or Sim3Solver::Batch first).  Unlike
// the constructor above, the matched point's keyframe is the window keyframe it came through (what the reference
// intends with vpKeyFrameMatchedMP); GetIndexInKeyFrame < 0 on either side drops the slot as at :90.
// Matcher: orbgpu::ORBmatcher<MA> over the same KeyFrame / MapPoint types (matcherBoW of :795).
// Never throws; returns false when a library call failed (orbgpu::LastShimError()): every candidate then has
// numBoWMatches 0, all-NULL vectors and no solver.
template <class A, class Matcher>
bool LoopBowProblems(Matcher& matcherBoW, typename A::KeyFrame* pCurrentKF,
                     const std::vector<typename A::KeyFrame*>& vpCandidates,
                     const std::vector<std::vector<typename A::KeyFrame*>>& vvpCovKFi, const bool bFixScale,
                     std::vector<LoopBowCandidate<A>>& out) {
    using KeyFrame = typename A::KeyFrame;
    using MapPoint = typename A::MapPoint;
    const size_t nc = vpCandidates.size();
    const std::vector<MapPoint*> mps1 = A::MapPointMatches(pCurrentKF);
    const int n1 = (int)mps1.size();
    out.clear();
    out.resize(nc);
    for (size_t c = 0; c < nc; ++c) {
        out[c].vpMatchedPoints.assign(n1, static_cast<MapPoint*>(nullptr));
        out[c].vpKeyFrameMatchedMP.assign(n1, static_cast<KeyFrame*>(nullptr));
        out[c].vnMatches.assign(c < vvpCovKFi.size() ? vvpCovKFi[c].size() : 0, 0);
    }
    if (nc == 0 || vvpCovKFi.size() != nc) return nc == 0;
    // the pairs, candidate after candidate; a skipped window keyframe keeps its place with pair_ok = 0
    std::vector<KeyFrame*> pair_kf, live;
    std::vector<uint8_t> pair_ok;
    std::vector<int32_t> group(1, 0);
    for (size_t c = 0; c < nc; ++c) {
        for (KeyFrame* k : vvpCovKFi[c]) {
            const bool ok = k && !A::IsBad(k);
            pair_kf.push_back(k);
            pair_ok.push_back(ok ? 1 : 0);
            if (ok) live.push_back(k);
        }
        group.push_back((int32_t)pair_kf.size());
    }
    const size_t P = pair_kf.size();
    std::vector<int32_t> live_rows, live_counts;
    if (!matcherBoW.SearchByBoWIndices(pCurrentKF, live, live_rows, live_counts)) return false;  // :840-851
    const int C = n1 > 0 ? n1 : 1;
    std::vector<int32_t> rows(P * (size_t)C + 1, -1);
    // (the search's rows are as long as the keyframe's feature count, which is the map-point vector's length)
    const size_t ls = live.empty() ? 0 : (live_rows.size() - 1) / live.size();
    for (size_t p = 0, l = 0; p < P; ++p) {
        if (!pair_ok[p]) continue;
        std::copy(live_rows.begin() + l * ls, live_rows.begin() + l * ls + std::min(ls, (size_t)n1), rows.begin() + p * (size_t)C);
        for (size_t c = 0; c < nc; ++c)
            if ((int32_t)p >= group[c] && (int32_t)p < group[c + 1]) out[c].vnMatches[p - group[c]] = live_counts[l];
        ++l;
    }
    // the map points as indices into one pool
    std::map<MapPoint*, int32_t> ids;
    std::vector<MapPoint*> pool;
    std::vector<float> xyz;
    std::vector<uint8_t> bad;
    auto id_of = [&](MapPoint* p) -> int32_t {
        if (!p) return -1;
        auto it = ids.find(p);
        if (it != ids.end()) return it->second;
        const int32_t id = (int32_t)pool.size();
        ids[p] = id;
        pool.push_back(p);
        float X[3];
        A::WorldPos(p, X);
        xyz.insert(xyz.end(), X, X + 3);
        bad.push_back(A::IsBad(p) ? 1 : 0);
        return id;
    };
    struct Store {
        std::vector<int32_t> mp_id;
        std::vector<uint8_t> obs_ok;
    };
    auto describe = [&](KeyFrame* k, const std::vector<MapPoint*>& mps, Store& s, orb_loop_bow_kf_t& r) {
        const int n = (int)mps.size();
        s.mp_id.assign(n > 0 ? n : 1, -1);
        s.obs_ok.assign(n > 0 ? n : 1, 0);
        for (int i = 0; i < n; ++i) {
            s.mp_id[i] = id_of(mps[i]);
            s.obs_ok[i] = (mps[i] && A::IndexInKeyFrame(mps[i], k) >= 0) ? 1 : 0;  // Sim3Solver.cc:87-91
        }
        r.n = n;
        r.mp_id = s.mp_id.data();
        r.kps = A::KeysUn(k);
        r.obs_ok = s.obs_ok.data();
        r.nlevels = 1;
        for (int l = 0; l < 12; ++l) r.level_sigma2[l] = 0.f;
    };
    orb_loop_bow_in_t in{};
    Store s1;
    describe(pCurrentKF, mps1, s1, in.kf1);
    std::vector<Store> s2(P);
    std::vector<orb_loop_bow_kf_t> kf2s(P + 1);
    auto sigma = [](KeyFrame* k, const std::vector<MapPoint*>& mps, orb_loop_bow_kf_t& r) {
        int top = 0;  // mvLevelSigma2's length is not known here: the levels the keyframe's keypoints use (<= 12)
        for (int i = 0; i < (int)mps.size(); ++i) top = std::max(top, std::min(11, std::max(0, (int)A::KeysUn(k)[i].octave)));
        for (int l = 0; l <= top; ++l) r.level_sigma2[l] = A::LevelSigma2(k)[l];
        r.nlevels = top + 1;
    };
    sigma(pCurrentKF, mps1, in.kf1);
    for (size_t p = 0; p < P; ++p) {
        kf2s[p].nlevels = 1;
        if (!pair_ok[p]) continue;
        const std::vector<MapPoint*> mps = A::MapPointMatches(pair_kf[p]);
        describe(pair_kf[p], mps, s2[p], kf2s[p]);
        sigma(pair_kf[p], mps, kf2s[p]);
    }
    std::vector<uint8_t> ok1(C, 0);
    for (int i = 0; i < n1; ++i) ok1[i] = (mps1[i] && !A::IsBad(mps1[i])) ? 1 : 0;
    in.ok1 = ok1.data();
    float R[9], t[3];
    A::Pose(pCurrentKF, R, t);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) in.Tcw1[4 * r + c] = R[3 * r + c];
        in.Tcw1[4 * r + 3] = t[r];
    }
    std::vector<float> Tcw2(12 * nc);
    for (size_t c = 0; c < nc; ++c) {
        A::Pose(vpCandidates[c], R, t);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) Tcw2[12 * c + 4 * r + k] = R[3 * r + k];
            Tcw2[12 * c + 4 * r + 3] = t[r];
        }
    }
    if (xyz.empty()) xyz.assign(3, 0.f);
    in.n_pairs = (int32_t)P;
    in.n_cand = (int32_t)nc;
    in.kf2s = kf2s.data();
    in.pair_ok = pair_ok.empty() ? nullptr : pair_ok.data();
    in.group = group.data();
    in.Tcw2 = Tcw2.data();
    in.n_points = (int32_t)pool.size();
    in.xyz = xyz.data();
    in.bad = bad.empty() ? nullptr : bad.data();
    in.matches12 = rows.data();
    in.stride = C;
    std::vector<int32_t> mpt(nc * (size_t)C), mpr(nc * (size_t)C), idx1(nc * (size_t)C), num_bow(nc), n(nc);
    std::vector<float> x1(3 * nc * (size_t)C), x2(3 * nc * (size_t)C), e1(nc * (size_t)C), e2(nc * (size_t)C);
    orb_loop_bow_out_t o{mpt.data(), mpr.data(), num_bow.data(), n.data(), idx1.data(), x1.data(), x2.data(), e1.data(),
                         e2.data()};
    if (detail::Failed(orb_loop_bow_problems(matcherBoW.LibraryHandle(), &in, &o), "orb_loop_bow_problems")) return false;
    for (size_t c = 0; c < nc; ++c) {
        const size_t row = c * (size_t)C;
        for (int k = 0; k < n1; ++k) {
            const int32_t id = mpt[row + k], j = mpr[row + k];
            if (id < 0 || id >= (int32_t)pool.size() || j < 0 || j >= group[c + 1] - group[c]) continue;
            out[c].vpMatchedPoints[k] = pool[id];                  // :876
            out[c].vpKeyFrameMatchedMP[k] = vvpCovKFi[c][j];       // :878
        }
        out[c].numBoWMatches = num_bow[c];
        out[c].solver.reset(new Sim3Solver<A>(pCurrentKF, vpCandidates[c], n1, n[c], &idx1[row], &x1[3 * row], &x2[3 * row],
                                              &e1[row], &e2[row], bFixScale));
    }
    return true;
}

}  // namespace orbgpu

/* ---- the accessor for the reference's own classes (compiled inside the reference build) ---------------------- */
#ifdef ORBGPU_WITH_ORBSLAM3
namespace orbgpu {

struct ORBSLAM3Sim3Access {
    using KeyFrame = ORB_SLAM3::KeyFrame;
    using MapPoint = ORB_SLAM3::MapPoint;
    using Matrix4f = Eigen::Matrix4f;
    using Matrix3f = Eigen::Matrix3f;
    using Vector3f = Eigen::Vector3f;
    static Matrix4f Matrix4(const float m[16]) { return Eigen::Map<const Eigen::Matrix<float, 4, 4, Eigen::RowMajor>>(m); }
    static Matrix3f Matrix3(const float m[9]) { return Eigen::Map<const Eigen::Matrix<float, 3, 3, Eigen::RowMajor>>(m); }
    static Vector3f Vector3(const float v[3]) { return Vector3f(v[0], v[1], v[2]); }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->GetMapPointMatches(); }
    static bool IsBad(MapPoint* p) { return p->isBad(); }
    static bool IsBad(KeyFrame* k) { return k->isBad(); }
    static int IndexInKeyFrame(MapPoint* p, KeyFrame* k) { return std::get<0>(p->GetIndexInKeyFrame(k)); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return reinterpret_cast<const orb_keypoint_t*>(k->mvKeysUn.data()); }
    static const float* LevelSigma2(KeyFrame* k) { return k->mvLevelSigma2.data(); }
    static void Pose(KeyFrame* k, float R[9], float t[3]) {
        const Eigen::Matrix3f Rcw = k->GetRotation();
        const Eigen::Vector3f tcw = k->GetTranslation();
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[3 * r + c] = Rcw(r, c);
            t[r] = tcw(r);
        }
    }
    static void WorldPos(MapPoint* p, float X[3]) {
        const Eigen::Vector3f x = p->GetWorldPos();
        X[0] = x(0); X[1] = x(1); X[2] = x(2);
    }
    static void Pinhole(KeyFrame* k, float K[4]) {
        for (int i = 0; i < 4; ++i) K[i] = k->mpCamera->getParameter(i);
    }
    static int RandomInt(int min, int max) { return DUtils::Random::RandomInt(min, max); }
};

using GpuSim3Solver = Sim3Solver<ORBSLAM3Sim3Access>;

}  // namespace orbgpu
#endif  // ORBGPU_WITH_ORBSLAM3

#endif  // ORBGPU_SIM3_HPP
