// CPU check of orbgpu::Sim3Solver<A> (include/orbgpu_sim3.hpp, reference src/Sim3Solver.cc) on a mock KeyFrame /
// MapPoint graph.  orb_sim3_ransac is a test double: by default it evaluates the problems for real with the
// kernel's own per-lane arithmetic compiled for the host (csrc/orb_sim3_math.h), or, when g_counts is set, it
// reports scripted counts (hypothesis h's first g_counts[h] correspondences as its inliers), so the replay of
// iterate() can be pinned count by count.  The HIP kernels are compared with the restatement in
// tests/test_sim3_gpu.py, the shim against the real library in tests/native/sim3_shim_gpu.cpp.  Checked:
//   * the gather (:71-118): every skip, mvnIndices1's mapping back to vpMatched12's rows, a passed keyframe list
//     that is never read, the camera-frame points and the thresholds;
//   * SetRansacParameters' arithmetic;
//   * the order and the arguments of the A::RandomInt calls and the swap-with-back triples;
//   * the replay: chunks of iterate(20), the best persisting across calls, a later tie winning, bNoMore at the
//     cap, the bConverge overload's chunk best, find(), the getters;
//   * Batch: one library call for several solvers, none for solvers already evaluated;
//   * every ORB_ERR_* from the library: the identity, bNoMore, the code in orbgpu::LastShimError().
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../orb-slam3_byzyh_amd/csrc/orb_sim3_math.h"
#include "orbgpu_sim3.hpp"

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
            ++g_fail;                                                         \
        }                                                                     \
    } while (0)

// ---- mock reference objects ------------------------------------------------------------------------
struct MockKF;
struct MockMP {
    float pos[3] = {0, 0, 0};
    bool bad = false;
    std::map<MockKF*, int> index;  // GetIndexInKeyFrame
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<MockMP*> mps;
    std::vector<float> sigma2{1.f, 1.44f, 2.0736f};
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    float K[4] = {458.654f, 457.296f, 367.215f, 248.375f};
};

static std::vector<std::pair<int, int>> g_rand_calls;
static std::vector<int> g_rand_script;  // empty: always 0
static size_t g_rand_pos = 0;

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    using Matrix4f = std::array<float, 16>;
    using Matrix3f = std::array<float, 9>;
    using Vector3f = std::array<float, 3>;
    static Matrix4f Matrix4(const float m[16]) { Matrix4f o; std::memcpy(o.data(), m, 64); return o; }
    static Matrix3f Matrix3(const float m[9]) { Matrix3f o; std::memcpy(o.data(), m, 36); return o; }
    static Vector3f Vector3(const float v[3]) { Vector3f o; std::memcpy(o.data(), v, 12); return o; }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static int IndexInKeyFrame(MapPoint* p, KeyFrame* k) { return p->index.count(k) ? p->index[k] : -1; }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2.data(); }
    static void Pose(KeyFrame* k, float R[9], float t[3]) { std::memcpy(R, k->R, 36); std::memcpy(t, k->t, 12); }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static int RandomInt(int lo, int hi) {
        g_rand_calls.emplace_back(lo, hi);
        const int v = g_rand_script.empty() ? 0 : g_rand_script[g_rand_pos++ % g_rand_script.size()];
        return lo + v % (hi - lo + 1);
    }
};
using Solver = orbgpu::Sim3Solver<Access>;
static const Access::Matrix4f kIdentity{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// ---- the C ABI's test doubles ----------------------------------------------------------------------
static int g_rc = 0, g_calls = 0, g_last_problems = 0;
static std::string g_err = "injected";
static std::vector<int> g_counts;
static std::vector<orb_sim3_problem_t> g_seen;

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_sim3_ransac(const orb_sim3_problem_t* probs, int n_problems, const orb_sim3_out_t* outs) {
    ++g_calls;
    g_last_problems = n_problems;
    if (g_rc != 0) return g_rc;
    g_seen.assign(probs, probs + n_problems);
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = probs[k];
        const orb_sim3_out_t& o = outs[k];
        const int W = (p.n + 63) / 64;
        *o.winner = *o.best = -1;
        int best_count = -1;
        for (int h = 0; h < p.n_hyp; ++h) {
            float p1[3][3], p2[3][3], T12[12], T21[12];
            for (int j = 0; j < 3; ++j) {
                const int idx = p.samples[3 * h + j];
                if (idx < 0 || idx >= p.n) return ORB_ERR_ARG;
                for (int c = 0; c < 3; ++c) {
                    p1[j][c] = p.x3dc1[3 * idx + c];
                    p2[j][c] = p.x3dc2[3 * idx + c];
                }
            }
            orbgpu::sim3_closed_form(p1, p2, p.fix_scale != 0, T12, T21, &o.hyp_scale[h]);
            std::memcpy(&o.hyp_t12[12 * h], T12, 48);
            int count = 0;
            for (int w = 0; w < W; ++w) o.hyp_mask[(size_t)h * W + w] = 0;
            for (int i = 0; i < p.n; ++i) {
                bool in;
                if (!g_counts.empty()) {
                    in = i < g_counts[h];
                } else {
                    const float* X1 = &p.x3dc1[3 * i];
                    const float* X2 = &p.x3dc2[3 * i];
                    const float im1[2] = {p.cam1[0] * X1[0] / X1[2] + p.cam1[2], p.cam1[1] * X1[1] / X1[2] + p.cam1[3]};
                    const float im2[2] = {p.cam2[0] * X2[0] / X2[2] + p.cam2[2], p.cam2[1] * X2[1] / X2[2] + p.cam2[3]};
                    in = orbgpu::sim3_inlier(T12, T21, X1, X2, im1, im2, p.cam1, p.cam2, p.max_err1[i], p.max_err2[i]);
                }
                if (in) {
                    o.hyp_mask[(size_t)h * W + (i >> 6)] |= 1ull << (i & 63);
                    ++count;
                }
            }
            o.hyp_inliers[h] = count;
            if (*o.winner < 0 && count > p.min_inliers) *o.winner = h;
            if (count >= best_count) {
                best_count = count;
                *o.best = h;
            }
        }
    }
    return ORB_OK;
}
}  // extern "C"

// ---- the scene: keyframe 2 sees n points 4 m ahead; keyframe 1 is keyframe 2 moved by a known Sim3 --------
struct Scene {
    MockKF kf1, kf2, other;
    std::vector<MockMP> mp1, mp2;
    std::vector<MockMP*> matched;

    explicit Scene(int n) : mp1(n), mp2(n) {
        const float c = 0.9553365f, s = 0.2955202f;  // 0.3 rad about y
        const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
        std::memcpy(kf1.R, R, 36);
        kf1.t[0] = 0.2f; kf1.t[2] = 0.4f;
        for (int i = 0; i < n; ++i) {
            const float x = -1.5f + 0.37f * (i % 9), y = -1.f + 0.29f * (i % 7), z = 3.f + 0.21f * (i % 11);
            mp1[i].pos[0] = mp2[i].pos[0] = x;
            mp1[i].pos[1] = mp2[i].pos[1] = y;
            mp1[i].pos[2] = mp2[i].pos[2] = z;
            orb_keypoint_t kp{};
            kp.octave = i % 3;
            kf1.kps.push_back(kp);
            kp.octave = (i + 1) % 3;
            kf2.kps.push_back(kp);
            kf1.mps.push_back(&mp1[i]);
            mp1[i].index[&kf1] = i;
            mp2[i].index[&kf2] = i;
            matched.push_back(&mp2[i]);
        }
    }
};

int main() {
    // ---- the gather ---------------------------------------------------------------------------------
    {
        Scene s(12);
        s.matched[0] = nullptr;            // no match
        s.kf1.mps[1] = nullptr;            // no map point in keyframe 1
        s.mp1[2].bad = true;
        s.mp2[3].bad = true;
        s.mp1[4].index.clear();            // indexKF1 < 0
        s.mp2[5].index.clear();            // indexKF2 < 0
        s.mp2[6].index[&s.other] = 0;      // observed by another keyframe too: still looked up in pKF2
        Solver a(&s.kf1, &s.kf2, s.matched, false);
        CHECK(a.Correspondences() == 6);
        // a list that is passed is never read (the reference's flag is set only when the list is empty)
        Solver b(&s.kf1, &s.kf2, s.matched, false, std::vector<MockKF*>(12, &s.other));
        CHECK(b.Correspondences() == 6);
        // all six are exact inliers of any triple: converges at the first hypothesis with 6 > 5
        a.SetRansacParameters(0.99, 5, 300);
        g_calls = 0;
        g_counts.clear();
        bool no_more = true;
        std::vector<bool> inl;
        int n_inl = -1;
        const auto T = a.iterate(5, no_more, inl, n_inl);
        CHECK(g_calls == 1 && g_last_problems == 1 && !no_more && n_inl == 6 && inl.size() == 12);
        const std::vector<bool> want{false, false, false, false, false, false, true, true, true, true, true, true};
        CHECK(inl == want);
        // T12 maps keyframe 2's camera frame (= the world here) to keyframe 1's: [R1 | t1], scale 1
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) CHECK(std::fabs(T[4 * r + c] - s.kf1.R[3 * r + c]) < 1e-5f);
            CHECK(std::fabs(T[4 * r + 3] - s.kf1.t[r]) < 1e-5f);
        }
        CHECK(T[12] == 0 && T[13] == 0 && T[14] == 0 && T[15] == 1);
        CHECK(std::fabs(a.GetEstimatedScale() - 1.f) < 1e-5f && a.GetEstimatedTransformation() == T);
        CHECK(std::fabs(a.GetEstimatedRotation()[2] - s.kf1.R[2]) < 1e-5f && a.GetEstimatedTranslation()[2] == T[11]);
        // what the library was given: point 6 (the first survivor), thresholds from the two keyframes' octaves
        const orb_sim3_problem_t& p = g_seen[0];
        CHECK(p.n == 6 && p.fix_scale == 0 && p.min_inliers == 5 && p.cam1[0] == 458.654f && p.cam2[3] == 248.375f);
        CHECK(p.x3dc2[0] == s.mp2[6].pos[0] && p.x3dc2[2] == s.mp2[6].pos[2]);
        const float* R = s.kf1.R;
        const float* X = s.mp1[6].pos;
        CHECK(p.x3dc1[0] == ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + s.kf1.t[0]);
        CHECK(p.max_err1[0] == (float)(9.210 * s.kf1.sigma2[6 % 3]) && p.max_err2[0] == (float)(9.210 * s.kf2.sigma2[7 % 3]));
    }
    // ---- SetRansacParameters -----------------------------------------------------------------------------
    {
        Scene s20(20), s100(100);
        Solver a(&s20.kf1, &s20.kf2, s20.matched);
        a.SetRansacParameters(0.99, 20, 300);
        CHECK(a.MaxIterations() == 1);
        a.SetRansacParameters(0.99, 15, 300);
        CHECK(a.MaxIterations() == 9);
        a.SetRansacParameters(0.99, 15, 5);
        CHECK(a.MaxIterations() == 5);
        a.SetRansacParameters(0.99, 15, 0);
        CHECK(a.MaxIterations() == 1);
        Solver b(&s100.kf1, &s100.kf2, s100.matched);
        CHECK(b.MaxIterations() == 300);   // the constructor's defaults: 6 / 100
        b.SetRansacParameters(0.99, 15, 300);
        CHECK(b.MaxIterations() == 300);
        // n < minInliers: bNoMore at once, nothing drawn, nothing called
        a.SetRansacParameters(0.99, 21, 300);
        g_calls = 0;
        g_rand_calls.clear();
        bool no_more = false, conv = true;
        std::vector<bool> inl;
        int n_inl = -1;
        CHECK(a.iterate(20, no_more, inl, n_inl, conv) == kIdentity && no_more && !conv && n_inl == 0);
        CHECK(g_calls == 0 && g_rand_calls.empty() && inl == std::vector<bool>(20, false));
    }
    // ---- the draws --------------------------------------------------------------------------------------
    {
        Scene s(6);
        Solver a(&s.kf1, &s.kf2, s.matched);
        a.SetRansacParameters(0.99, 3, 2);
        CHECK(a.MaxIterations() == 2);
        g_rand_script = {5, 0, 0, 2, 2, 3};
        g_rand_pos = 0;
        g_rand_calls.clear();
        g_counts = {0, 0};
        bool no_more;
        std::vector<bool> inl;
        int n_inl;
        a.iterate(1, no_more, inl, n_inl);
        // all draws up front, three per iteration over a shrinking range; each list starts full again
        const std::vector<std::pair<int, int>> want{{0, 5}, {0, 4}, {0, 3}, {0, 5}, {0, 4}, {0, 3}};
        CHECK(g_rand_calls == want);
        CHECK((a.Samples() == std::vector<int32_t>{5, 0, 4, 2, 5, 3}));
        a.iterate(1, no_more, inl, n_inl);
        CHECK(g_rand_calls.size() == 6 && no_more);   // nothing drawn again
        g_rand_script.clear();
    }
    // ---- the replay ---------------------------------------------------------------------------------------
    {
        Scene s(30);
        Solver a(&s.kf1, &s.kf2, s.matched);
        a.SetRansacParameters(0.99, 10, 50);
        CHECK(a.MaxIterations() == 50);
        g_counts.assign(50, 0);
        g_counts[3] = 4; g_counts[7] = 6; g_counts[12] = 6;   // chunk 0: 3, then 7, then 12 (a later tie wins)
        g_counts[25] = 5;                                      // chunk 1: below the best carried over
        g_counts[45] = 11; g_counts[47] = 30;                  // chunk 2 converges at 45
        g_calls = 0;
        bool no_more, conv;
        std::vector<bool> inl;
        int n_inl;
        auto T = a.iterate(20, no_more, inl, n_inl, conv);
        CHECK(!no_more && !conv && n_inl == 0 && a.Iterations() == 20 && T == a.GetEstimatedTransformation());
        CHECK(a.HypothesisInliers()[12] == 6 && T[15] == 1);
        const auto best0 = a.GetEstimatedTransformation();
        T = a.iterate(20, no_more, inl, n_inl, conv);
        CHECK(!no_more && !conv && T == kIdentity && a.GetEstimatedTransformation() == best0 && a.Iterations() == 40);
        T = a.iterate(20, no_more, inl, n_inl, conv);
        CHECK(conv && !no_more && n_inl == 11 && a.Iterations() == 46 && T == a.GetEstimatedTransformation());
        int set = 0;
        for (int i = 0; i < 30; ++i) set += inl[i] ? 1 : 0;
        CHECK(set == 11 && inl[10] && !inl[11]);
        // called again after a convergence: hypothesis 47 (30 >= 11) converges next
        T = a.iterate(20, no_more, inl, n_inl, conv);
        CHECK(conv && n_inl == 30 && a.Iterations() == 48);
        T = a.iterate(20, no_more, inl, n_inl);
        CHECK(no_more && n_inl == 0 && T == kIdentity && a.Iterations() == 50);
        CHECK(g_calls == 1);
        // find(): all iterations in one go; nothing converges, the cap sets bNoMore inside, identity returned
        Solver b(&s.kf1, &s.kf2, s.matched);
        b.SetRansacParameters(0.99, 10, 50);
        g_counts[45] = g_counts[47] = 0;
        CHECK(b.find(inl, n_inl) == kIdentity && n_inl == 0 && b.Iterations() == 50);
        CHECK(b.GetEstimatedTransformation() != kIdentity);   // hypothesis 12's
        g_counts.clear();
    }
    // ---- Batch ----------------------------------------------------------------------------------------------
    {
        Scene s(30), t(12);
        Solver a(&s.kf1, &s.kf2, s.matched), b(&t.kf1, &t.kf2, t.matched, false), c(&t.kf1, &t.kf2, t.matched);
        a.SetRansacParameters(0.99, 10, 40);
        b.SetRansacParameters(0.99, 8, 30);
        c.SetRansacParameters(0.99, 13, 30);   // n < minInliers: left out of the call
        g_calls = 0;
        Solver::Batch({&a, &b, nullptr, &c});
        CHECK(g_calls == 1 && g_last_problems == 2 && g_seen[0].n == 30 && g_seen[1].n == 12 && g_seen[1].fix_scale == 0);
        bool no_more;
        std::vector<bool> inl;
        int n_inl;
        a.iterate(20, no_more, inl, n_inl);
        b.iterate(20, no_more, inl, n_inl);
        CHECK(n_inl == 12);
        c.iterate(20, no_more, inl, n_inl);
        CHECK(no_more && g_calls == 1);
        Solver::Batch({&a, &b});
        CHECK(g_calls == 1);                   // already evaluated
    }
    // ---- failures -------------------------------------------------------------------------------------------
    for (int rc : {ORB_ERR_ARG, ORB_ERR_CAPACITY, ORB_ERR_DEVICE, ORB_ERR_ABORTED, ORB_ERR_INTERNAL}) {
        Scene s(30);
        Solver a(&s.kf1, &s.kf2, s.matched), b(&s.kf1, &s.kf2, s.matched);
        g_rc = rc;
        orbgpu::ClearShimError();
        bool no_more = false, conv = true;
        std::vector<bool> inl;
        int n_inl = -1;
        CHECK(a.iterate(20, no_more, inl, n_inl, conv) == kIdentity && no_more && !conv && n_inl == 0);
        CHECK(inl == std::vector<bool>(30, false) && orbgpu::LastShimError() == rc);
        CHECK(orbgpu::LastShimMessage().find("orb_sim3_ransac") != std::string::npos);
        orbgpu::ClearShimError();
        Solver::Batch({&b});
        CHECK(orbgpu::LastShimError() == rc && b.find(inl, n_inl) == kIdentity && n_inl == 0);
        g_rc = 0;
    }
    orbgpu::ClearShimError();
    if (g_fail) return 1;
    std::printf("OK sim3_shim_check\n");
    return 0;
}
