// CPU check of orbgpu::OptimizeSim3<S> / OptimizeSim3Batch<S> (include/orbgpu_optimizer.hpp, reference
// src/Optimizer.cc:4195-4494) on a mock KeyFrame / MapPoint graph.  orb_optimize_sim3 is a scripted test double: it
// keeps a deep copy of every problem it is given and answers with scripted outputs.  The kernel is compared with the
// restatement in tests/test_optsim3_gpu.py, the shim against the real library in tests/native/optsim3_shim_gpu.cpp.
// Checked:
//   * the gather (:4254-4407): every skip rule, vnIndexEdge's mapping back to vpMatches1's rows, the float32
//     camera-frame points cast to double, the observations and informations, the i2 < 0 rule (normalised
//     observation, information of level 0), bAllPoints;
//   * the write-back: vpMatches1 cleared where inlier is 0, g2oS12 and mAcumHessian set, the return value;
//   * the < 10 exit: vpMatches1 culled, g2oS12 and mAcumHessian untouched, 0 returned;
//   * the batch: one library call for several candidates;
//   * every ORB_ERR_* from the library: arguments untouched, 0 returned, the code in orbgpu::LastShimError().
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "orbgpu_optimizer.hpp"

static int g_fail = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                \
        }                                                            \
    } while (0)

struct MockKF;
struct MockMP {
    float pos[3] = {0, 0, 0};
    bool bad = false;
    std::map<MockKF*, int> index;
};
struct KeyUn {
    float x, y;
    int octave;
};
struct MockKF {
    std::vector<KeyUn> kps;
    std::vector<MockMP*> mps;
    std::vector<float> inv_sigma2{1.f, 0.69444f, 0.48225f};
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    float K[4] = {458.654f, 457.296f, 367.215f, 248.375f};
};
using Mat7 = std::array<double, 49>;
using Sim3v = std::array<double, 8>;

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    using Sim3 = Sim3v;
    using Matrix7d = Mat7;
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static int IndexInKeyFrame(MapPoint* p, KeyFrame* k) { return p->index.count(k) ? p->index[k] : -1; }
    static void Pose(KeyFrame* k, float R[9], float t[3]) { std::memcpy(R, k->R, 36); std::memcpy(t, k->t, 12); }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void KeyUn(KeyFrame* k, int i, float* x, float* y, int* o) { *x = k->kps[i].x; *y = k->kps[i].y; *o = k->kps[i].octave; }
    static float InvLevelSigma2(KeyFrame* k, int o) { return k->inv_sigma2[o]; }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static void GetSim3(const Sim3& s, double v[8]) { std::memcpy(v, s.data(), 64); }
    static void SetSim3(Sim3& s, const double v[8]) { std::memcpy(s.data(), v, 64); }
    static void SetZero(Matrix7d& m) { m.fill(0.0); }
};

// ---- the C ABI's test double -----------------------------------------------------------------------------------
struct Seen {
    int n;
    std::vector<double> p1c, p2c, obs1, obs2;
    std::vector<float> is1, is2;
    float cam1[4], cam2[4], th2;
    double s12[8];
    int fix_scale;
};
static int g_rc = 0, g_calls = 0;
static std::string g_err = "injected";
static std::vector<Seen> g_seen;
// the scripted answer to problem k: pairs listed in g_out[k] are outliers; n_bad, n_in and s12_out as given
struct Script {
    std::vector<int> outliers;
    int n_bad, n_in;
    double s12[8];
};
static std::vector<Script> g_script;

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_optimize_sim3(const orb_optsim3_problem_t* probs, int n_problems, const orb_optsim3_out_t* outs) {
    ++g_calls;
    if (g_rc != 0) return g_rc;
    g_seen.clear();
    for (int k = 0; k < n_problems; ++k) {
        const orb_optsim3_problem_t& p = probs[k];
        Seen s;
        s.n = p.n;
        s.p1c.assign(p.p1c, p.p1c + 3 * p.n); s.p2c.assign(p.p2c, p.p2c + 3 * p.n);
        s.obs1.assign(p.obs1, p.obs1 + 2 * p.n); s.obs2.assign(p.obs2, p.obs2 + 2 * p.n);
        s.is1.assign(p.inv_sigma2_1, p.inv_sigma2_1 + p.n); s.is2.assign(p.inv_sigma2_2, p.inv_sigma2_2 + p.n);
        std::memcpy(s.cam1, p.cam1, 16); std::memcpy(s.cam2, p.cam2, 16); std::memcpy(s.s12, p.s12, 64);
        s.th2 = p.th2; s.fix_scale = p.fix_scale;
        g_seen.push_back(s);
        const Script& sc = g_script[k];
        for (int i = 0; i < p.n; ++i) outs[k].inlier[i] = 1;
        for (int i : sc.outliers) outs[k].inlier[i] = 0;
        *outs[k].n_bad = sc.n_bad; *outs[k].n_in = sc.n_in;
        std::memcpy(outs[k].s12_out, sc.s12, 64);
        if (outs[k].chi2_12 || outs[k].chi2_21) return ORB_ERR_ARG;  // the shim does not ask for them
    }
    return ORB_OK;
}
}  // extern "C"

// ---- a graph: 16 rows of vpMatches1, 4 of them skipped one way each, one by the i2 < 0 rule ------------------------
struct Graph {
    MockKF kf1, kf2;
    std::vector<MockMP> mp1, mp2;
    std::vector<MockMP*> matches;
    static constexpr int N = 16;
    Graph() : mp1(N), mp2(N), matches(N) {
        const float R2[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
        std::memcpy(kf2.R, R2, 36);
        kf2.t[0] = 0.5f; kf2.t[1] = -0.25f; kf2.t[2] = 1.0f;
        kf1.t[0] = 0.125f; kf1.t[2] = 0.5f;
        kf2.K[0] = 500.f;
        kf1.kps.resize(N); kf2.kps.resize(N + 4); kf1.mps.resize(N);
        for (int i = 0; i < N; ++i) {
            mp1[i].pos[0] = 0.1f * i; mp1[i].pos[1] = -0.05f * i; mp1[i].pos[2] = 3.f + 0.25f * i;
            mp2[i].pos[0] = 0.3f + 0.1f * i; mp2[i].pos[1] = 0.2f; mp2[i].pos[2] = 2.f + 0.5f * i;
            kf1.kps[i] = {100.5f + i, 50.25f + 2 * i, i % 3};
            kf1.mps[i] = &mp1[i];
            mp2[i].index[&kf2] = i + 4;
            kf2.kps[i + 4] = {300.f - i, 200.f + i, (i + 1) % 3};
            matches[i] = &mp2[i];
        }
        matches[1] = nullptr;          // no match
        kf1.mps[3] = nullptr;          // no pMP1 (vPoint2 alone in the reference: no edge)
        mp1[5].bad = true;             // a bad point on either side
        mp2[6].bad = true;
        mp2[8].index.clear();          // i2 < 0: skipped unless bAllPoints
        mp2[10].pos[2] = -5.f;         // behind camera 2 (P3D2c(2) = pos z + 1 < 0)
    }
};

static void expect_rows(const Seen& s, const std::vector<int>& rows, Graph& g, int normalised_row) {
    CHECK(s.n == (int)rows.size());
    for (size_t k = 0; k < rows.size() && (int)k < s.n; ++k) {
        const int i = rows[k];
        float a[3], b[3];
        orbgpu::OptimizeSim3Candidate<Access>::ToCamera(g.kf1.R, g.kf1.t, g.mp1[i].pos, a);
        orbgpu::OptimizeSim3Candidate<Access>::ToCamera(g.kf2.R, g.kf2.t, g.mp2[i].pos, b);
        for (int c = 0; c < 3; ++c) {
            CHECK(s.p1c[3 * k + c] == (double)a[c]);
            CHECK(s.p2c[3 * k + c] == (double)b[c]);
        }
        CHECK(s.obs1[2 * k] == (double)g.kf1.kps[i].x && s.obs1[2 * k + 1] == (double)g.kf1.kps[i].y);
        CHECK(s.is1[k] == g.kf1.inv_sigma2[i % 3]);
        if (i == normalised_row) {
            const float invz = 1 / b[2];
            CHECK(s.obs2[2 * k] == (double)(b[0] * invz) && s.obs2[2 * k + 1] == (double)(b[1] * invz));
            CHECK(s.is2[k] == g.kf2.inv_sigma2[0]);
        } else {
            CHECK(s.obs2[2 * k] == (double)g.kf2.kps[i + 4].x && s.obs2[2 * k + 1] == (double)g.kf2.kps[i + 4].y);
            CHECK(s.is2[k] == g.kf2.inv_sigma2[(i + 1) % 3]);
        }
    }
}

int main() {
    const Sim3v start{0.01, 0.02, 0.03, 0.9993, 0.1, 0.2, 0.3, 1.25};
    const Script refined{{2, 9}, 1, 8, {0.5, 0.5, 0.5, 0.5, 1, 2, 3, 4}};
    Mat7 H;
    // ---- the gather without bAllPoints, the write-back past the < 10 exit
    {
        Graph g;
        Sim3v s12 = start;
        H.fill(7.0);
        g_script = {Script{{0, 7}, 0, 8, {0.5, 0.5, 0.5, 0.5, 1, 2, 3, 4}}};   // pairs 0 and 7 of the gathered graph
        g_calls = 0;
        orbgpu::ClearShimError();
        const int n = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 10.f, true, H, false);
        const std::vector<int> rows{0, 2, 4, 7, 9, 11, 12, 13, 14, 15};
        CHECK(g_calls == 1 && g_seen.size() == 1);
        expect_rows(g_seen[0], rows, g, -1);
        CHECK(g_seen[0].th2 == 10.f && g_seen[0].fix_scale == 1 && g_seen[0].cam2[0] == 500.f && g_seen[0].cam1[0] == 458.654f);
        CHECK(std::memcmp(g_seen[0].s12, start.data(), 64) == 0);
        CHECK(n == 8 && orbgpu::LastShimError() == ORB_OK);
        CHECK(g.matches[0] == nullptr && g.matches[13] == nullptr);           // gathered pairs 0 and 7
        for (int i : {2, 4, 7, 9, 11, 12, 14, 15}) CHECK(g.matches[i] == &g.mp2[i]);
        for (int i : {3, 5, 6, 8, 10}) CHECK(g.matches[i] == &g.mp2[i]);     // skipped rows are left alone
        CHECK(s12 == (Sim3v{0.5, 0.5, 0.5, 0.5, 1, 2, 3, 4}));
        for (double v : H) CHECK(v == 0.0);
    }
    // ---- bAllPoints: row 8 joins with the normalised observation and level 0's information; free scale
    {
        Graph g;
        Sim3v s12 = start;
        H.fill(7.0);
        g_script = {Script{{}, 0, 11, {0, 0, 0, 1, 0, 0, 0, 2}}};
        const int n = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 7.5f, false, H, true);
        expect_rows(g_seen[0], {0, 2, 4, 7, 8, 9, 11, 12, 13, 14, 15}, g, 8);
        CHECK(g_seen[0].th2 == 7.5f && g_seen[0].fix_scale == 0 && n == 11 && s12[7] == 2.0);
    }
    // ---- the < 10 exit: 10 gathered, 1 bad at the first cull: vpMatches1 culled, nothing else written, 0 returned
    {
        Graph g;
        Sim3v s12 = start;
        H.fill(7.0);
        g_script = {Script{{4}, 1, 0, {9, 9, 9, 9, 9, 9, 9, 9}}};
        const int n = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 10.f, true, H, false);
        CHECK(n == 0 && s12 == start && g.matches[9] == nullptr && g.matches[0] == &g.mp2[0]);
        for (double v : H) CHECK(v == 7.0);
        CHECK(orbgpu::LastShimError() == ORB_OK);
    }
    // ---- an empty graph: the call is still made, 0 returned
    {
        Graph g;
        for (auto& m : g.matches) m = nullptr;
        Sim3v s12 = start;
        g_script = {Script{{}, 0, 0, {9, 9, 9, 9, 9, 9, 9, 9}}};
        CHECK(orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 10.f, true, H, false) == 0);
        CHECK(g_seen[0].n == 0 && s12 == start);
    }
    // ---- the batch: one library call, each candidate written back from its own record
    {
        Graph g1, g2;
        Sim3v a = start, b = start;
        Mat7 Ha, Hb;
        Ha.fill(1.0); Hb.fill(1.0);
        std::vector<orbgpu::OptimizeSim3Candidate<Access>> c(2);
        c[0].pKF1 = &g1.kf1; c[0].pKF2 = &g1.kf2; c[0].vpMatches1 = &g1.matches; c[0].g2oS12 = &a; c[0].mAcumHessian = &Ha;
        c[1].pKF1 = &g2.kf1; c[1].pKF2 = &g2.kf2; c[1].vpMatches1 = &g2.matches; c[1].g2oS12 = &b; c[1].mAcumHessian = &Hb;
        c[1].bAllPoints = true; c[1].bFixScale = false; c[1].th2 = 20.f;
        g_script = {Script{{1}, 1, 0, {9, 9, 9, 9, 9, 9, 9, 9}}, refined};
        g_calls = 0;
        orbgpu::OptimizeSim3Batch<Access>(c);
        CHECK(g_calls == 1 && g_seen.size() == 2 && g_seen[0].n == 10 && g_seen[1].n == 11 && g_seen[1].th2 == 20.f);
        CHECK(c[0].result == 0 && a == start && Ha[0] == 1.0 && g1.matches[2] == nullptr);
        CHECK(c[1].result == 8 && b[7] == 4.0 && Hb[48] == 0.0 && g2.matches[4] == nullptr && g2.matches[14] == nullptr);
        std::vector<orbgpu::OptimizeSim3Candidate<Access>> none;
        orbgpu::OptimizeSim3Batch<Access>(none);
        CHECK(g_calls == 1);
    }
    // ---- every library failure: nothing written, 0 returned, the code reported
    for (int rc : {ORB_ERR_EMPTY, ORB_ERR_ARG, ORB_ERR_CAPACITY, ORB_ERR_DEVICE, ORB_ERR_ABORTED, ORB_ERR_INTERNAL}) {
        Graph g;
        const std::vector<MockMP*> before = g.matches;
        Sim3v s12 = start;
        H.fill(7.0);
        g_rc = rc;
        orbgpu::ClearShimError();
        int n = -1;
        try {
            n = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 10.f, true, H, false);
        } catch (...) {
            CHECK(!"the shim threw");
        }
        CHECK(n == 0 && g.matches == before && s12 == start && orbgpu::LastShimError() == rc);
        for (double v : H) CHECK(v == 7.0);
        CHECK(orbgpu::LastShimMessage().find("injected") != std::string::npos);
        g_rc = 0;
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK optsim3_shim_check\n");
    return 0;
}
