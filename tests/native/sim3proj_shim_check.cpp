// CPU check of the Sim3 search shims in include/orbgpu_matcher.hpp (SearchByProjection(KF, Scw, ...), its
// vpMatchedKF overload, Fuse(KF, Scw, ...) and their batched forms; reference src/ORBmatcher.cc:496-733,
// :1547-1676) on a mock KeyFrame / MapPoint graph.  orb_sim3_projection is a plain scalar test double (the
// sequential loops in ordinary float arithmetic, a window's keypoints scanned in INDEX order), so this runs
// without a GPU; the HIP kernels are compared with the restatement in tests/test_sim3_projection_gpu.py.  No
// case here depends on how a distance tie falls.  Checked:
//   * skip = isBad() || spAlreadyFound.count(pMP) and taken0 = vpMatched[idx] != NULL as the double receives
//     them; vpMatched / vpMatchedKF written from matched[]; the return value;
//   * Fuse's step 7 in point order: AddObservation + AddMapPoint for a free keypoint, then the next point with
//     the same best keypoint becomes a replacement (vpReplacePoint[iMP] = the point just added); a bad
//     pMPinKF is counted and not recorded; points already in the keyframe are skipped;
//   * the batched forms equal the sequence of single calls; one launch for B jobs;
//   * an ORB_ERR_* from the library: 0 returned, nothing written, the code in orbgpu::LastShimError().
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "orbgpu_matcher.hpp"

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
    float pos[3] = {0, 0, 4}, normal[3] = {0, 0, 1}, min_dist = 1, max_dist = 3.7f;  // predicted level 0
    uint8_t desc[32] = {};
    bool bad = false;
    std::map<MockKF*, int> obs;
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<MockMP*> mps;
    std::vector<float> scale{1.f, 1.2f}, inv_sigma2{1.f, 1.f / 1.44f};
    void add(float x, float y, uint8_t d0) {
        orb_keypoint_t k{};
        k.x = x; k.y = y; k.octave = 0;
        kps.push_back(k);
        desc.resize(desc.size() + 32, 0);
        desc[desc.size() - 32] = d0;
        mps.push_back(nullptr);
    }
};
struct MockSim3 {
    float s = 1.f, t[3] = {0, 0, 0};  // rotation: identity
};

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame*) { return nullptr; }
    static void Pinhole(KeyFrame*, float K[4]) { K[0] = K[1] = 128.f; K[2] = 320.f; K[3] = 240.f; }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static void FuseGeometry(KeyFrame* k, orb_fuse_kf_t* v) {
        orb_frame_view_t& f = v->frame;
        f.min_x = 0; f.max_x = 640; f.min_y = 0; f.max_y = 480;
        f.grid_inv_w = 0.1f; f.grid_inv_h = 0.1f;
        v->inv_level_sigma2 = k->inv_sigma2.data();
        v->log_scale_factor = std::log(1.2f);
    }
    static void Sim3Pose(const MockSim3& S, float Tcw[12], float Ow[3]) {
        const float T[12] = {1, 0, 0, S.t[0] / S.s, 0, 1, 0, S.t[1] / S.s, 0, 0, 1, S.t[2] / S.s};
        std::memcpy(Tcw, T, sizeof(T));
        for (int r = 0; r < 3; ++r) Ow[r] = -S.t[r] / S.s;
    }
    static std::set<MapPoint*> MapPointSet(KeyFrame* k) {
        std::set<MapPoint*> s(k->mps.begin(), k->mps.end());
        s.erase(nullptr);
        return s;
    }
    static MapPoint* GetMapPoint(KeyFrame* k, int idx) { return k->mps[idx]; }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->mps[idx] = p; }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) { p->obs[k] = idx; }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void Normal(MapPoint* p, float X[3]) { std::memcpy(X, p->normal, 12); }
    static float MinDistance(MapPoint* p) { return p->min_dist; }
    static float MaxDistance(MapPoint* p) { return p->max_dist; }
    static void Descriptor(MapPoint* p, uint8_t d[32]) { std::memcpy(d, p->desc, 32); }
};
using Matcher = orbgpu::ORBmatcher<Access>;

// ---- the C ABI's test doubles ----------------------------------------------------------------------
static int g_rc = 0, g_calls = 0, g_last_jobs = 0;
static std::string g_err = "injected";
static std::vector<uint8_t> g_skip, g_taken0;

static int popcount_dist(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount(a[i] ^ b[i]);
    return d;
}

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_descriptor_distance(const uint8_t* a, const uint8_t* b) { return popcount_dist(a, b); }
int orb_matcher_create(float, int, orb_matcher_t* out) {
    *out = reinterpret_cast<orb_matcher_t>(new int(0));
    return ORB_OK;
}
int orb_matcher_destroy(orb_matcher_t m) {
    delete reinterpret_cast<int*>(m);
    return ORB_OK;
}
// the three loops per job, scalar (src/ORBmatcher.cc:520-616, :640-730, :1570-1651)
int orb_sim3_projection(orb_matcher_t, const orb_sim3_projection_kf_t* kfs, int, const orb_sim3_projection_job_t* jobs,
                        int n_jobs, const orb_fuse_points_t* pool, const uint8_t* skip, const uint8_t* taken0, int stride,
                        int32_t* matched, int32_t* nmatches, int32_t* best_idx, int32_t* best_dist) {
    ++g_calls;
    g_last_jobs = n_jobs;
    if (g_rc != 0) return g_rc;
    int off = 0;
    for (int b = 0; b < n_jobs; ++b) off += jobs[b].count;
    g_skip.assign(skip, skip + off);
    g_taken0.assign(taken0, taken0 + (size_t)n_jobs * stride);
    off = 0;
    for (int b = 0; b < n_jobs; ++b) {
        const orb_sim3_projection_job_t& J = jobs[b];
        const orb_frame_view_t& f = kfs[J.kf].frame;
        const bool fuse = J.mode == ORB_S3P_FUSE;
        std::vector<char> claimed(f.n, 0);
        for (int j = 0; j < stride; ++j) matched[(size_t)b * stride + j] = -1;
        for (int j = 0; j < f.n && !fuse; ++j) claimed[j] = taken0[(size_t)b * stride + j];
        nmatches[b] = 0;
        for (int p = 0; p < J.count; ++p, ++off) {
            const int i = J.first + p;
            best_idx[off] = -1;
            if (best_dist) best_dist[off] = 256;
            if (skip[off]) continue;
            const float* P = &pool->pos[3 * i];
            float Pc[3];
            for (int r = 0; r < 3; ++r) Pc[r] = J.Tcw[4 * r] * P[0] + J.Tcw[4 * r + 1] * P[1] + J.Tcw[4 * r + 2] * P[2] + J.Tcw[4 * r + 3];
            if (Pc[2] < 0.0f) continue;
            const float u = f.fx * Pc[0] / Pc[2] + f.cx, v = f.fy * Pc[1] / Pc[2] + f.cy;
            if (!(u >= f.min_x && u < f.max_x && v >= f.min_y && v < f.max_y)) continue;
            const float radius = J.th * f.scale_factors[0];  // (the mock points predict level 0)
            int bestDist = 256, bestIdx = -1;
            for (int j = 0; j < f.n; ++j) {
                const orb_keypoint_t& kp = f.kps_un[j];
                if (!(std::fabs(kp.x - u) < radius && std::fabs(kp.y - v) < radius)) continue;
                if (claimed[j] || kp.octave > 0) continue;
                const int d = popcount_dist(&pool->desc[32 * i], &f.desc[32 * j]);
                if (d < bestDist) {
                    bestDist = d;
                    bestIdx = j;
                }
            }
            if (!((float)bestDist <= (fuse ? 50.f : 50 * J.ratio_hamming))) continue;
            best_idx[off] = bestIdx;
            ++nmatches[b];
            if (!fuse) {
                claimed[bestIdx] = 1;
                matched[(size_t)b * stride + bestIdx] = p;
            }
        }
    }
    return ORB_OK;
}
}

// a point projecting to (u, v) at the identity pose, descriptor byte 0 = d0
static MockMP* point(std::vector<MockMP>& store, float u, float v, uint8_t d0) {
    store.emplace_back();
    MockMP& p = store.back();
    p.pos[0] = (u - 320.f) * 4.f / 128.f;
    p.pos[1] = (v - 240.f) * 4.f / 128.f;
    p.desc[0] = d0;
    return &p;
}

int main() {
    Matcher m(0.75f, true);
    MockSim3 S;
    S.s = 2.f;  // t = 0: the pose is the identity whatever the scale
    std::vector<MockMP> store;
    store.reserve(64);
    MockKF kf, kfA, kfB;
    kf.add(100, 100, 0x01);   // 0
    kf.add(101, 100, 0x03);   // 1
    kf.add(300, 200, 0x00);   // 2
    kf.add(500, 400, 0x0f);   // 3
    MockMP* a = point(store, 100, 100, 0x01);   // -> keypoint 0 (distance 0)
    MockMP* b = point(store, 100, 100, 0x01);   // keypoint 0 claimed -> keypoint 1 (distance 1)
    MockMP* c = point(store, 300, 200, 0x00);   // bad: skipped
    c->bad = true;
    MockMP* d = point(store, 500, 400, 0x0f);   // already in vpMatched: skipped
    MockMP* e = point(store, 300, 200, 0x00);   // keypoint 2 holds a match before the call: taken0
    MockKF srcA, srcB;
    const std::vector<MockMP*> pts{a, b, c, d, e, nullptr};
    const std::vector<MockKF*> ptKFs{&srcA, &srcB, &srcA, &srcA, &srcB, &srcA};

    {   // the first form
        std::vector<MockMP*> matched(4, nullptr);
        matched[2] = d;
        const int n = m.SearchByProjection(&kf, S, pts, matched, 3, 1.0f);
        CHECK(n == 2 && matched[0] == a && matched[1] == b && matched[2] == d && matched[3] == nullptr);
        CHECK((g_skip == std::vector<uint8_t>{0, 0, 1, 1, 0, 1}));
        CHECK((std::vector<uint8_t>(g_taken0.begin(), g_taken0.begin() + 4) == std::vector<uint8_t>{0, 0, 1, 0}));
        CHECK(orbgpu::LastShimError() == ORB_OK);
    }
    {   // the second form: vpMatchedKF follows vpMatched
        std::vector<MockMP*> matched(4, nullptr);
        std::vector<MockKF*> matchedKF(4, nullptr);
        matched[2] = d;
        const int n = m.SearchByProjection(&kf, S, pts, ptKFs, matched, matchedKF, 3, 1.5f);
        CHECK(n == 2 && matched[0] == a && matched[1] == b && matchedKF[0] == &srcA && matchedKF[1] == &srcB);
        CHECK(matchedKF[2] == nullptr && matchedKF[3] == nullptr);
        std::vector<MockKF*> shortKF(3, nullptr);
        CHECK(m.SearchByProjection(&kf, S, pts, ptKFs, matched, shortKF, 3, 1.5f) == 0 && orbgpu::LastShimError() == ORB_ERR_ARG);
        orbgpu::ClearShimError();
    }
    {   // the batched form equals the single calls, in one launch
        std::vector<std::vector<MockMP*>> vpts{pts, {e, a}}, vm{std::vector<MockMP*>(4, nullptr), std::vector<MockMP*>(4, nullptr)};
        vm[0][2] = d;
        std::vector<int> n;
        const int before = g_calls;
        m.SearchByProjection(std::vector<std::pair<MockKF*, MockSim3>>{{&kf, S}, {&kf, S}}, vpts, vm, 3, 1.0f, n);
        CHECK(g_calls == before + 1 && g_last_jobs == 2);
        CHECK((n == std::vector<int>{2, 2}) && vm[0][0] == a && vm[0][1] == b && vm[1][2] == e && vm[1][0] == a);
        std::vector<MockMP*> single(4, nullptr);
        CHECK(m.SearchByProjection(&kf, S, vpts[1], single, 3, 1.0f) == 2 && single == vm[1]);
    }
    {   // Fuse: step 7 in point order
        MockMP* held = point(store, 0, 0, 0);      // the map point keypoint 3 holds
        MockMP* dead = point(store, 0, 0, 0);      // a bad map point in keypoint 2
        dead->bad = true;
        kf.mps = {nullptr, nullptr, dead, held};
        MockMP* f1 = point(store, 100, 100, 0x01); // keypoint 0 free: added
        MockMP* f2 = point(store, 100, 100, 0x01); // keypoint 0 again (no claims in Fuse): f1 is there now -> replacement
        MockMP* f3 = point(store, 500, 400, 0x0f); // keypoint 3 holds `held` -> replacement
        MockMP* f4 = point(store, 300, 200, 0x00); // keypoint 2 holds a bad point: counted, not recorded
        MockMP* far = point(store, 100, 100, 0xf1);// distance 4 to keypoint 0 (5 to keypoint 1): replacement by f1
        const std::vector<MockMP*> fp{f1, f2, held, f3, f4, far};
        std::vector<MockMP*> rep(fp.size(), nullptr);
        const int n = m.Fuse(&kf, S, fp, 4.0f, rep);
        CHECK(n == 5);
        CHECK(kf.mps[0] == f1 && f1->obs.count(&kf) && f1->obs[&kf] == 0);
        CHECK(rep[0] == nullptr && rep[1] == f1 && rep[2] == nullptr && rep[3] == held && rep[4] == nullptr && rep[5] == f1);
        CHECK((g_skip == std::vector<uint8_t>{0, 0, 1, 0, 0, 0}));   // `held` is already in the keyframe
        CHECK(f2->obs.empty() && kf.mps[3] == held);
        // batched over two distinct keyframes equals the single calls; the same keyframe twice is refused
        kfA.add(100, 100, 0x01);
        kfB.add(500, 400, 0x0f);
        kfB.mps[0] = held;
        std::vector<std::vector<MockMP*>> vrep(2, std::vector<MockMP*>(fp.size(), nullptr));
        std::vector<int> vn;
        const int before = g_calls;
        m.Fuse(std::vector<std::pair<MockKF*, MockSim3>>{{&kfA, S}, {&kfB, S}}, fp, 4.0f, vrep, vn);
        CHECK(g_calls == before + 1 && (vn == std::vector<int>{3, 1}));
        CHECK(kfA.mps[0] == f1 && vrep[0][1] == f1 && vrep[0][5] == f1 && vrep[1][3] == held);
        m.Fuse(std::vector<std::pair<MockKF*, MockSim3>>{{&kfA, S}, {&kfA, S}}, fp, 4.0f, vrep, vn);
        CHECK((vn == std::vector<int>{0, 0}) && orbgpu::LastShimError() == ORB_ERR_ARG);
        orbgpu::ClearShimError();
    }
    for (int rc : {ORB_ERR_DEVICE, ORB_ERR_CAPACITY, ORB_ERR_ARG}) {   // error injection
        g_rc = rc;
        std::vector<MockMP*> matched(4, nullptr);
        std::vector<MockKF*> matchedKF(4, nullptr);
        CHECK(m.SearchByProjection(&kf, S, pts, matched, 3, 1.0f) == 0 && orbgpu::LastShimError() == rc);
        orbgpu::ClearShimError();
        CHECK(m.SearchByProjection(&kf, S, pts, ptKFs, matched, matchedKF, 3, 1.0f) == 0 && orbgpu::LastShimError() == rc);
        CHECK(matched == std::vector<MockMP*>(4, nullptr) && matchedKF == std::vector<MockKF*>(4, nullptr));
        orbgpu::ClearShimError();
        MockKF fresh;
        fresh.add(100, 100, 0x01);
        std::vector<MockMP*> fp{pts[0]}, rep(1, nullptr);
        const size_t obs_before = pts[0]->obs.size();
        CHECK(m.Fuse(&fresh, S, fp, 4.0f, rep) == 0 && orbgpu::LastShimError() == rc);
        CHECK(fresh.mps[0] == nullptr && rep[0] == nullptr && pts[0]->obs.size() == obs_before);
        orbgpu::ClearShimError();
        g_rc = 0;
    }
    if (g_fail) return 1;
    std::printf("OK sim3proj_shim_check\n");
    return 0;
}
