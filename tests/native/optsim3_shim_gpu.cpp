// orbgpu::OptimizeSim3<S> and OptimizeSim3Batch<S> (include/orbgpu_optimizer.hpp) against the real liborbgpu.so on a
// two-keyframe graph read from a file (tests/test_optsim3_shim_gpu.py writes it, with what the library's Python
// entry returns for the same gathered graph): the return value, the bits of g2oS12 and the rows of vpMatches1 left
// set must be the same, for the single call and for the batch.
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
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
    float pos[3];
    bool bad = false;
    std::map<MockKF*, int> index;
};
struct MockKF {
    float R[9], t[3], K[4], inv_sigma2[8];
    std::vector<std::array<float, 3>> kps;  // x, y, octave
    std::vector<MockMP*> mps;
};
using Sim3v = std::array<double, 8>;
using Mat7 = std::array<double, 49>;

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
    static void KeyUn(KeyFrame* k, int i, float* x, float* y, int* o) { *x = k->kps[i][0]; *y = k->kps[i][1]; *o = (int)k->kps[i][2]; }
    static float InvLevelSigma2(KeyFrame* k, int o) { return k->inv_sigma2[o]; }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static void GetSim3(const Sim3& s, double v[8]) { std::memcpy(v, s.data(), 64); }
    static void SetSim3(Sim3& s, const double v[8]) { std::memcpy(s.data(), v, 64); }
    static void SetZero(Matrix7d& m) { m.fill(0.0); }
};

struct Graph {
    MockKF kf1, kf2;
    std::vector<MockMP> mp1, mp2;
    std::vector<MockMP*> matches;
};
struct Config {
    int32_t fix, all;
    float th2;
    int32_t ret;
    Sim3v s12;
    std::vector<uint8_t> kept;
};

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[3];
    if (!rd(f, head, 3) || head[0] != 0x4f533300) return 2;
    const int N = head[1], ncfg = head[2];
    Graph g0;
    for (MockKF* k : {&g0.kf1, &g0.kf2})
        if (!rd(f, k->R, 9) || !rd(f, k->t, 3) || !rd(f, k->K, 4) || !rd(f, k->inv_sigma2, 8)) return 2;
    std::vector<float> pos1(3 * N), pos2(3 * N), kp1(3 * N), kp2(3 * N);
    std::vector<int32_t> flags(N);
    Sim3v start;
    if (!rd(f, pos1.data(), 3 * N) || !rd(f, pos2.data(), 3 * N) || !rd(f, kp1.data(), 3 * N) || !rd(f, kp2.data(), 3 * N) ||
        !rd(f, flags.data(), N) || !rd(f, start.data(), 8))
        return 2;
    std::vector<Config> cfg(ncfg);
    for (Config& c : cfg) {
        c.kept.resize(N);
        if (!rd(f, &c.fix, 1) || !rd(f, &c.all, 1) || !rd(f, &c.th2, 1) || !rd(f, &c.ret, 1) || !rd(f, c.s12.data(), 8) ||
            !rd(f, c.kept.data(), N))
            return 2;
    }
    std::fclose(f);
    auto build = [&](Graph& g) {
        g = g0;
        g.mp1.resize(N); g.mp2.resize(N); g.matches.assign(N, nullptr);
        g.kf1.kps.resize(N); g.kf2.kps.resize(N); g.kf1.mps.assign(N, nullptr);
        for (int i = 0; i < N; ++i) {
            std::memcpy(g.mp1[i].pos, &pos1[3 * i], 12);
            std::memcpy(g.mp2[i].pos, &pos2[3 * i], 12);
            g.kf1.kps[i] = {kp1[3 * i], kp1[3 * i + 1], kp1[3 * i + 2]};
            g.kf2.kps[i] = {kp2[3 * i], kp2[3 * i + 1], kp2[3 * i + 2]};
            if (flags[i] & 1) g.matches[i] = &g.mp2[i];
            if (flags[i] & 2) g.kf1.mps[i] = &g.mp1[i];
            g.mp1[i].bad = (flags[i] & 4) != 0;
            g.mp2[i].bad = (flags[i] & 8) != 0;
            if (flags[i] & 16) g.mp2[i].index[&g.kf2] = i;
        }
    };
    auto verify = [&](const Config& c, int ret, const Sim3v& s12, const Graph& g, const Mat7& H) {
        CHECK(ret == c.ret);
        CHECK(std::memcmp(s12.data(), c.s12.data(), 64) == 0);
        for (int i = 0; i < N; ++i) CHECK((g.matches[i] != nullptr) == (c.kept[i] != 0));
        if (c.ret > 0)
            for (double v : H) CHECK(v == 0.0);
    };
    // one call per configuration
    for (const Config& c : cfg) {
        Graph g;
        build(g);
        Sim3v s12 = start;
        Mat7 H;
        H.fill(3.0);
        orbgpu::ClearShimError();
        const int ret = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, c.th2, c.fix != 0, H, c.all != 0);
        CHECK(orbgpu::LastShimError() == ORB_OK);
        std::printf("config fix=%d all=%d: returned %d (expected %d)\n", c.fix, c.all, ret, c.ret);
        verify(c, ret, s12, g, H);
    }
    // all configurations in one batch
    {
        std::vector<Graph> gs(ncfg);
        std::vector<Sim3v> s(ncfg, start);
        std::vector<Mat7> H(ncfg);
        std::vector<orbgpu::OptimizeSim3Candidate<Access>> cands(ncfg);
        for (int k = 0; k < ncfg; ++k) {
            build(gs[k]);
            H[k].fill(3.0);
            cands[k].pKF1 = &gs[k].kf1; cands[k].pKF2 = &gs[k].kf2; cands[k].vpMatches1 = &gs[k].matches;
            cands[k].g2oS12 = &s[k]; cands[k].th2 = cfg[k].th2; cands[k].bFixScale = cfg[k].fix != 0;
            cands[k].mAcumHessian = &H[k]; cands[k].bAllPoints = cfg[k].all != 0;
        }
        orbgpu::OptimizeSim3Batch<Access>(cands);
        CHECK(orbgpu::LastShimError() == ORB_OK);
        for (int k = 0; k < ncfg; ++k) verify(cfg[k], cands[k].result, s[k], gs[k], H[k]);
    }
    // a library rejection (th2 = 0): nothing written, 0 returned, the code reported
    {
        Graph g;
        build(g);
        const std::vector<MockMP*> before = g.matches;
        Sim3v s12 = start;
        Mat7 H;
        H.fill(3.0);
        const int ret = orbgpu::OptimizeSim3<Access>(&g.kf1, &g.kf2, g.matches, s12, 0.f, true, H, false);
        CHECK(ret == 0 && orbgpu::LastShimError() == ORB_ERR_ARG && g.matches == before && s12 == start && H[0] == 3.0);
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK optsim3_shim_gpu\n");
    return 0;
}
