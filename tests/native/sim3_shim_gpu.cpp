// orbgpu::Sim3Solver<A> (include/orbgpu_sim3.hpp) driven against the real liborbgpu.so on a mock graph read from
// a file written by tests/test_sim3_shim_gpu.py: two keyframes with poses, n matched map points with world
// positions and octaves, and a script for A::RandomInt.  The reference's caller loop
//     while (!bConverge && !bNoMore) T = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
// must end with the hypothesis, the transform (bit for bit), nInliers and vbInliers that the Python side got from
// the library's Python entry for the same draws and the replay of tests/sim3_ref.py.  Then Batch: two solvers
// evaluated in one call equal the two evaluated alone (counts, samples and the loop's results).
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbgpu_sim3.hpp"

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
            ++g_fail;                                                         \
        }                                                                     \
    } while (0)

struct MockKF;
struct MockMP {
    float pos[3];
    int idx;
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<MockMP*> mps;
    float sigma2[8], R[9], t[3], K[4];
};
static std::vector<int32_t> g_script;
static size_t g_pos = 0;

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
    static bool IsBad(MapPoint*) { return false; }
    static int IndexInKeyFrame(MapPoint* p, KeyFrame*) { return p->idx; }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2; }
    static void Pose(KeyFrame* k, float R[9], float t[3]) { std::memcpy(R, k->R, 36); std::memcpy(t, k->t, 12); }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static int RandomInt(int lo, int hi) { return lo + g_script[g_pos++ % g_script.size()] % (hi - lo + 1); }
};
using Solver = orbgpu::Sim3Solver<Access>;

struct Expected {
    int32_t max_its, hyp, n_inliers, iterations;
    float T[16];
    std::vector<uint8_t> inliers;
};
struct Result {
    Access::Matrix4f T;
    std::vector<bool> inliers;
    int n_inliers, iterations;
    bool converge, no_more;
};

static Result run_loop(Solver& s) {
    Result r{};
    while (!r.converge && !r.no_more) r.T = s.iterate(20, r.no_more, r.inliers, r.n_inliers, r.converge);
    r.iterations = s.Iterations();
    return r;
}

static bool read(std::FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];  // magic, n, script length, number of solver configurations (2)
    if (!read(f, hdr, sizeof(hdr)) || hdr[0] != 0x53696d33 || hdr[3] != 2) return 2;
    const int n = hdr[1];
    MockKF kf1, kf2;
    bool ok = true;
    for (MockKF* k : {&kf1, &kf2}) ok = ok && read(f, k->R, 36) && read(f, k->t, 12) && read(f, k->K, 16) && read(f, k->sigma2, 32);
    std::vector<MockMP> mp1(n), mp2(n);
    std::vector<int32_t> oct(n);
    for (auto* mps : {&mp1, &mp2}) {
        MockKF& k = mps == &mp1 ? kf1 : kf2;
        ok = ok && read(f, oct.data(), 4 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            ok = ok && read(f, (*mps)[i].pos, 12);
            (*mps)[i].idx = i;
            orb_keypoint_t kp{};
            kp.octave = oct[i];
            k.kps.push_back(kp);
        }
    }
    g_script.resize(hdr[2]);
    ok = ok && read(f, g_script.data(), 4 * (size_t)hdr[2]);
    int32_t cfg[2][3];  // fix_scale, min_inliers, max_iterations
    Expected want[2];
    for (int k = 0; k < 2; ++k) {
        want[k].inliers.resize(n);
        ok = ok && read(f, cfg[k], 12) && read(f, &want[k].max_its, 16) && read(f, want[k].T, 64) && read(f, want[k].inliers.data(), n);
    }
    std::fclose(f);
    if (!ok) return 2;
    for (int i = 0; i < n; ++i) kf1.mps.push_back(&mp1[i]);
    std::vector<MockMP*> matched;
    for (int i = 0; i < n; ++i) matched.push_back(&mp2[i]);

    // ---- each solver alone (solver 1's draws continue the script where solver 0's ended, as in the batch) -------
    Result alone[2];
    std::vector<int32_t> counts[2], samples[2];
    g_pos = 0;
    for (int k = 0; k < 2; ++k) {
        Solver s(&kf1, &kf2, matched, cfg[k][0] != 0);
        s.SetRansacParameters(0.99, cfg[k][1], cfg[k][2]);
        CHECK(s.Correspondences() == n && s.MaxIterations() == want[k].max_its);
        alone[k] = run_loop(s);
        const Result& r = alone[k];
        std::printf("solver %d: %d iterations, converge %d, %d inliers\n", k, r.iterations, (int)r.converge, r.n_inliers);
        CHECK(orbgpu::LastShimError() == ORB_OK);
        CHECK(r.converge == (want[k].hyp >= 0) && r.iterations == want[k].iterations && r.n_inliers == want[k].n_inliers);
        CHECK(std::memcmp(r.T.data(), want[k].T, 64) == 0);
        CHECK(r.inliers.size() == (size_t)n);
        for (int i = 0; i < n && i < (int)r.inliers.size(); ++i) CHECK(r.inliers[i] == (want[k].inliers[i] != 0));
        if (r.converge) CHECK(s.GetEstimatedTransformation() == r.T);
        counts[k] = s.HypothesisInliers();
        samples[k] = s.Samples();
    }
    CHECK(alone[0].iterations > 20);   // the loop took more than one chunk
    // ---- the two in one call ----------------------------------------------------------------------------------
    {
        Solver a(&kf1, &kf2, matched, cfg[0][0] != 0), b(&kf1, &kf2, matched, cfg[1][0] != 0);
        a.SetRansacParameters(0.99, cfg[0][1], cfg[0][2]);
        b.SetRansacParameters(0.99, cfg[1][1], cfg[1][2]);
        g_pos = 0;
        Solver::Batch({&a, &b});
        CHECK(orbgpu::LastShimError() == ORB_OK);
        Solver* both[2] = {&a, &b};
        for (int k = 0; k < 2; ++k) {
            CHECK(both[k]->HypothesisInliers() == counts[k] && both[k]->Samples() == samples[k]);
            const Result r = run_loop(*both[k]);
            CHECK(r.T == alone[k].T && r.inliers == alone[k].inliers && r.n_inliers == alone[k].n_inliers);
            CHECK(r.iterations == alone[k].iterations && r.converge == alone[k].converge && r.no_more == alone[k].no_more);
        }
    }
    if (g_fail) return 1;
    std::printf("OK sim3_shim_gpu\n");
    return 0;
}
