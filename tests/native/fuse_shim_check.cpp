// CPU check of ORBmatcher::Fuse in include/orbgpu_matcher.hpp (src/ORBmatcher.cc:1326-1534) on a mock
// KeyFrame / MapPoint graph.  orb_fuse is a plain scalar test double (the search of :1378-1506 in ordinary
// float arithmetic, windows scanned in index order), so this runs without a GPU; the HIP kernels are compared
// with the reference restatement in tests/test_fuse_gpu.py.  The mock MapPoint::Replace moves the
// observations and recomputes the survivor's descriptor, as src/MapPoint.cc:330-378 does.  The double scans a
// window's keypoints in INDEX order, not in GetFeaturesInArea's order (grid columns outer, rows inner): no case
// here depends on how a distance tie falls, and none may be added that does -- tie order is pinned in
// tests/fuse_cases.py against the restatement and the kernel.  Checked:
//   * step 7 of a single call: no map point -> AddObservation + AddMapPoint; a map point with more
//     observations -> pMP->Replace(pMPinKF); otherwise pMPinKF->Replace(pMP); a bad pMPinKF -> nothing, still
//     counted; the skip tests evaluated again at apply time (a point listed twice that went bad meanwhile);
//   * the batched overload against the sequence of single calls on a copy of the graph: vnFused and the
//     final graph state equal, on a scene that holds a survivor whose descriptor changed and whose stale
//     result differs from the fresh one, and a point that entered a later keyframe through a Replace;
//   * an ORB_ERR_* from the library: 0 returned, the graph untouched, the code in orbgpu::LastShimError().
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <sstream>
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

// ---- mock reference objects ------------------------------------------------------------------------
struct MockKF;
struct ById {
    bool operator()(const MockKF* a, const MockKF* b) const;
};
struct MockMP {
    int id = 0;
    float pos[3] = {0, 0, 4}, normal[3] = {0, 0, 1}, min_dist = 1, max_dist = 3.7f;
    uint8_t desc[32] = {};
    bool bad = false;
    std::map<MockKF*, int, ById> obs;
    bool InKF(MockKF* k) const { return obs.count(k) != 0; }
    void ComputeDistinctiveDescriptors();
    void Replace(MockMP* by);
};
struct MockKF {
    int id = 0;
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<float> ur;
    std::vector<MockMP*> mps;
    std::vector<float> scale{1.f, 1.2f}, inv_sigma2{1.f, 1.f / 1.44f};
    bool cam2 = false;
};
bool ById::operator()(const MockKF* a, const MockKF* b) const { return a->id < b->id; }
// (stands in for the median-distance choice: the row of the observation in the keyframe with the lowest id)
void MockMP::ComputeDistinctiveDescriptors() {
    if (obs.empty()) return;
    std::memcpy(desc, &obs.begin()->first->desc[32 * obs.begin()->second], 32);
}
void MockMP::Replace(MockMP* by) {  // src/MapPoint.cc:330-378
    if (by == this) return;
    bad = true;
    const auto mine = obs;
    obs.clear();
    for (const auto& o : mine) {
        if (!by->InKF(o.first)) {
            o.first->mps[o.second] = by;
            by->obs[o.first] = o.second;
        } else {
            o.first->mps[o.second] = nullptr;
        }
    }
    by->ComputeDistinctiveDescriptors();
}

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame* k) { return k->ur.data(); }
    static void Pinhole(KeyFrame*, float K[4]) { K[0] = K[1] = 128.f; K[2] = 320.f; K[3] = 240.f; }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static bool SingleCamera(KeyFrame* k) { return !k->cam2; }
    static void FuseGeometry(KeyFrame* k, orb_fuse_kf_t* v) {
        orb_frame_view_t& f = v->frame;
        f.min_x = 0; f.max_x = 640; f.min_y = 0; f.max_y = 480;
        f.grid_inv_w = 0.1f; f.grid_inv_h = 0.1f;
        f.bf = 40.f;
        const float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        std::memcpy(f.Tcw, T, sizeof(T));
        v->Ow[0] = v->Ow[1] = v->Ow[2] = 0.f;
        v->inv_level_sigma2 = k->inv_sigma2.data();
        v->log_scale_factor = std::log(1.2f);
    }
    static MapPoint* GetMapPoint(KeyFrame* k, int idx) { return k->mps[idx]; }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->mps[idx] = p; }
    static bool IsInKeyFrame(MapPoint* p, KeyFrame* k) { return p->InKF(k); }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) { p->obs[k] = idx; }
    static void Replace(MapPoint* p, MapPoint* by) { p->Replace(by); }
    static int Observations(MapPoint* p) { return (int)p->obs.size(); }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void Normal(MapPoint* p, float X[3]) { std::memcpy(X, p->normal, 12); }
    static float MinDistance(MapPoint* p) { return p->min_dist; }
    static float MaxDistance(MapPoint* p) { return p->max_dist; }
    static void Descriptor(MapPoint* p, uint8_t d[32]) { std::memcpy(d, p->desc, 32); }
};
using Matcher = orbgpu::ORBmatcher<Access>;

// ---- the C ABI's test doubles ----------------------------------------------------------------------
static int g_rc = 0, g_calls = 0, g_fail_at_call = -1, g_stale_differs = 0;
static std::string g_err = "injected";
// the first (batched) call's result per (keyframe keypoint array, point position), to compare re-searches with
static std::map<std::pair<const void*, std::pair<float, float>>, int> g_first;
static bool g_record = false;

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
// src/ORBmatcher.cc:1378-1506 per job, scalar
int orb_fuse(orb_matcher_t, const orb_fuse_kf_t* kfs, int n_kfs, const orb_fuse_points_t* pts, const uint8_t* skip,
             float th, int32_t* best_idx, int32_t* best_dist) {
    const int call = g_calls++;
    if (g_rc != 0 && (g_fail_at_call < 0 || call == g_fail_at_call)) return g_rc;
    const int n = pts->n;
    for (int k = 0; k < n_kfs; ++k) {
        const orb_fuse_kf_t& K = kfs[k];
        const orb_frame_view_t& f = K.frame;
        for (int i = 0; i < n; ++i) {
            int bestDist = 256, bestIdx = -1;
            do {
                if (skip && skip[(size_t)k * n + i]) break;
                const float* P = &pts->pos[3 * i];
                float Pc[3];
                for (int r = 0; r < 3; ++r) Pc[r] = f.Tcw[4 * r] * P[0] + f.Tcw[4 * r + 1] * P[1] + f.Tcw[4 * r + 2] * P[2] + f.Tcw[4 * r + 3];
                if (Pc[2] < 0.0f) break;
                const float invz = 1 / Pc[2], u = f.fx * Pc[0] / Pc[2] + f.cx, v = f.fy * Pc[1] / Pc[2] + f.cy;
                if (!(u >= f.min_x && u < f.max_x && v >= f.min_y && v < f.max_y)) break;
                const float ur = u - f.bf * invz;
                const float PO[3] = {P[0] - K.Ow[0], P[1] - K.Ow[1], P[2] - K.Ow[2]};
                const float dist = std::sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
                if (dist < 0.8f * pts->min_dist[i] || dist > 1.2f * pts->max_dist[i]) break;
                const float* Pn = &pts->normal[3 * i];
                if (PO[0] * Pn[0] + PO[1] * Pn[1] + PO[2] * Pn[2] < 0.5f * dist) break;
                int level = (int)std::ceil(std::log(pts->max_dist[i] / dist) / K.log_scale_factor);
                level = level < 0 ? 0 : level >= f.nlevels ? f.nlevels - 1 : level;
                const float radius = th * f.scale_factors[level];
                for (int j = 0; j < f.n; ++j) {
                    const orb_keypoint_t& kp = f.kps_un[j];
                    if (!(std::fabs(kp.x - u) < radius && std::fabs(kp.y - v) < radius)) continue;
                    if (kp.octave < level - 1 || kp.octave > level) continue;
                    const float ex = u - kp.x, ey = v - kp.y;
                    if (f.u_right && f.u_right[j] >= 0) {
                        const float er = ur - f.u_right[j];
                        if ((ex * ex + ey * ey + er * er) * K.inv_level_sigma2[kp.octave] > 7.8) continue;
                    } else if ((ex * ex + ey * ey) * K.inv_level_sigma2[kp.octave] > 5.99) {
                        continue;
                    }
                    const int d = popcount_dist(&pts->desc[32 * i], &f.desc[32 * j]);
                    if (d < bestDist) {
                        bestDist = d;
                        bestIdx = j;
                    }
                }
            } while (false);
            const int out = bestDist <= 50 ? bestIdx : -1;
            best_idx[(size_t)k * n + i] = out;
            if (best_dist) best_dist[(size_t)k * n + i] = bestDist;
            if (g_record && !(skip && skip[(size_t)k * n + i])) {
                const auto key = std::make_pair((const void*)f.kps_un, std::make_pair(pts->pos[3 * i], pts->pos[3 * i + 1]));
                if (call == 0) g_first[key] = out;
                else if (g_first.count(key) && g_first[key] != out) ++g_stale_differs;
            }
        }
    }
    return ORB_OK;
}
}  // extern "C"

// ---- the scene -------------------------------------------------------------------------------------
static void ones(uint8_t* d, int n) {  // n leading one bits: two of them differ by the difference of their counts
    std::memset(d, 0, 32);
    for (int b = 0; b < n; ++b) d[b / 8] |= (uint8_t)(0x80 >> (b % 8));
}

struct Graph {
    std::vector<std::unique_ptr<MockKF>> kfs;
    std::vector<std::unique_ptr<MockMP>> mps;
    MockKF* source = nullptr;           // the new keyframe, whose map points are fused into the targets
    std::vector<MockKF*> targets;
    std::vector<MockMP*> points;        // vpMapPoints
    int next_mp = 0;

    MockKF* kf(int id) {
        kfs.emplace_back(new MockKF);
        kfs.back()->id = id;
        return kfs.back().get();
    }
    MockMP* mp(float u, float v, int desc_ones) {
        mps.emplace_back(new MockMP);
        MockMP* p = mps.back().get();
        p->id = next_mp++;
        p->pos[0] = (u - 320.f) * 4.f / 128.f;
        p->pos[1] = (v - 240.f) * 4.f / 128.f;
        const float d = std::sqrt(p->pos[0] * p->pos[0] + p->pos[1] * p->pos[1] + 16.f);
        for (int r = 0; r < 3; ++r) p->normal[r] = p->pos[r] / d;
        p->max_dist = d * 0.92f;  // level 0
        p->min_dist = p->max_dist / 1.2f;
        ones(p->desc, desc_ones);
        return p;
    }
    int keypoint(MockKF* k, float u, float v, int desc_ones, MockMP* holds = nullptr) {
        orb_keypoint_t kp{};
        kp.x = u;
        kp.y = v;
        k->kps.push_back(kp);
        k->desc.resize(k->desc.size() + 32);
        ones(&k->desc[k->desc.size() - 32], desc_ones);
        k->ur.push_back(-1.f);
        k->mps.push_back(holds);
        const int idx = (int)k->kps.size() - 1;
        if (holds) holds->obs[k] = idx;
        return idx;
    }
    // a map point of the source keyframe at pixel (u, v)
    MockMP* source_point(float u, float v, int desc_ones) {
        MockMP* p = mp(u, v, desc_ones);
        keypoint(source, u, v, desc_ones, p);
        points.push_back(p);
        return p;
    }
    std::string dump() const {
        std::ostringstream s;
        for (const auto& k : kfs) {
            s << "K" << k->id << ":";
            for (MockMP* p : k->mps) s << (p ? p->id : -1) << ",";
        }
        for (const auto& p : mps) {
            s << " M" << p->id << (p->bad ? "b" : "") << "[";
            for (int b = 0; b < 32; ++b) s << (int)p->desc[b] << ".";
            for (const auto& o : p->obs) s << " " << o.first->id << ":" << o.second;
            s << "]";
        }
        return s.str();
    }
};

// Three targets (ids 0 .. 2) and the source keyframe (id 10).  Pixels 40 px apart: one situation each.
static Graph make_graph() {
    Graph g;
    for (int id = 0; id < 3; ++id) g.targets.push_back(g.kf(id));
    g.source = g.kf(10);
    MockKF *k0 = g.targets[0], *k1 = g.targets[1], *k2 = g.targets[2];
    // A: the stale case.  k0's keypoint holds Q (one observation): Q->Replace(A), A gains k0's observation and
    // its descriptor becomes k0's row (30 ones instead of 0).  In k1 two free keypoints: with the sent
    // descriptor the 10-ones one is nearer (10 < 35), with the new one the 35-ones one (5 < 20).
    g.source_point(100, 100, 0);
    g.keypoint(k0, 100, 100, 30, g.mp(100, 100, 30));
    g.keypoint(k1, 100, 100, 10);
    g.keypoint(k1, 101, 100, 35);
    g.keypoint(k2, 100, 100, 33);
    // B: enters k1 through a Replace in k0: k0's keypoint holds R, which k1 observes too; R->Replace(B) moves
    // both observations, so B is in k1 when k1 is applied although the batched search found a match there
    // (B has a second observation in a keyframe outside the call, so R does not outnumber it)
    g.keypoint(g.kf(11), 140, 100, 0, g.source_point(140, 100, 0));
    {
        MockMP* R = g.mp(140, 100, 4);
        g.keypoint(k0, 140, 100, 4, R);
        g.keypoint(k1, 141, 100, 4, R);
        g.keypoint(k1, 140, 100, 2);
    }
    // C: k0's map point has more observations: C->Replace(S), C is bad for k1 and k2
    g.source_point(180, 100, 0);
    {
        MockMP* S = g.mp(180, 100, 6);
        g.keypoint(k0, 180, 100, 6, S);
        g.keypoint(k2, 300, 300, 6, S);
        g.keypoint(k1, 180, 100, 1);
    }
    // D: free keypoints everywhere: an observation added in each target
    g.source_point(220, 100, 0);
    for (MockKF* k : g.targets) g.keypoint(k, 220, 100, 8);
    // E: a bad map point in k0's keypoint: nothing happens, still counted
    g.source_point(260, 100, 0);
    {
        MockMP* X = g.mp(260, 100, 3);
        X->bad = true;
        g.keypoint(k0, 260, 100, 3);
        k0->mps.back() = X;
    }
    // F: no keypoint nearby; G: the nearest descriptor is 51 bits away; a NULL and a bad entry
    g.source_point(300, 100, 0);
    g.source_point(340, 100, 0);
    for (MockKF* k : g.targets) g.keypoint(k, 340, 100, 51);
    g.points.push_back(nullptr);
    g.source_point(380, 100, 0)->bad = true;
    for (MockKF* k : g.targets) g.keypoint(k, 380, 100, 0);
    // C once more: bad by the time the loop reaches it in k0 (apply-time check)
    g.points.push_back(g.points[2]);
    return g;
}

int main() {
    // ---- a single call, rule by rule -----------------------------------------------------------------
    {
        Graph g = make_graph();
        MockKF* k0 = g.targets[0];
        MockMP *A = g.points[0], *B = g.points[1], *C = g.points[2], *D = g.points[3];
        MockMP *Q = k0->mps[0], *S = k0->mps[2], *X = k0->mps[4];
        CHECK(Matcher::Supports(k0));
        g_calls = 0;
        const int n = Matcher().Fuse(k0, g.points, 3.0f);
        CHECK(g_calls == 1);
        CHECK(n == 5);                                           // A, B, C, D, E (C's second entry is bad by then)
        CHECK(Q->bad && k0->mps[0] == A && A->InKF(k0) && A->obs.size() == 2);
        uint8_t want[32];
        ones(want, 30);
        CHECK(std::memcmp(A->desc, want, 32) == 0);              // recomputed by the Replace
        CHECK(k0->mps[1] == B && B->InKF(g.targets[1]));         // both of R's observations moved
        CHECK(C->bad && k0->mps[2] == S && g.source->mps[2] == S && S->obs.size() == 3);
        CHECK(k0->mps[3] == D && D->obs.size() == 2 && D->obs[k0] == 3);
        CHECK(k0->mps[4] == X && g.points[4]->obs.size() == 1);  // bad pMPinKF: untouched
        CHECK(orbgpu::LastShimError() == ORB_OK);
        k0->cam2 = true;
        CHECK(!Matcher::Supports(k0));
    }
    // ---- batched against the sequence of single calls -------------------------------------------------
    {
        Graph seq = make_graph(), bat = make_graph();
        std::vector<int> want;
        for (MockKF* k : seq.targets) want.push_back(Matcher().Fuse(k, seq.points, 3.0f));
        g_calls = 0;
        g_first.clear();
        g_stale_differs = 0;
        g_record = true;
        std::vector<int> got;
        Matcher().Fuse(bat.targets, bat.points, 3.0f, got);
        g_record = false;
        CHECK(got == want);
        CHECK(want.size() == 3 && want[0] == 5 && want[1] >= 2 && want[2] >= 2);
        CHECK(bat.dump() == seq.dump());
        CHECK(g_calls == 3);             // the launch, and one re-search for each later keyframe
        CHECK(g_stale_differs >= 1);     // a stale result that differs from the fresh one (point A in k1)
        // A took k1's 35-ones keypoint (index 1), not the 10-ones one the stale descriptor prefers
        CHECK(bat.targets[1]->mps[1] == bat.points[0] && bat.targets[1]->mps[0] == nullptr);
        // B was skipped in k1: the free keypoint next to R's stays free
        CHECK(bat.targets[1]->mps[4] == nullptr);
        CHECK(orbgpu::LastShimError() == ORB_OK);
    }
    // ---- failures ---------------------------------------------------------------------------------------
    for (int rc : {ORB_ERR_ARG, ORB_ERR_DEVICE, ORB_ERR_INTERNAL}) {
        Graph g = make_graph();
        const std::string before = g.dump();
        g_rc = rc;
        g_fail_at_call = -1;
        orbgpu::ClearShimError();
        CHECK(Matcher().Fuse(g.targets[0], g.points, 3.0f) == 0);
        CHECK(orbgpu::LastShimError() == rc && g.dump() == before);
        orbgpu::ClearShimError();
        std::vector<int> got{7};
        Matcher().Fuse(g.targets, g.points, 3.0f, got);
        CHECK(got == std::vector<int>(3, 0) && orbgpu::LastShimError() == rc && g.dump() == before);
        CHECK(orbgpu::LastShimMessage().find("orb_fuse") != std::string::npos);
        // a failing re-search: the first keyframe stays applied, the rest count 0
        g_calls = 0;
        g_fail_at_call = 1;
        orbgpu::ClearShimError();
        Matcher().Fuse(g.targets, g.points, 3.0f, got);
        CHECK(got[0] == 5 && got[1] == 0 && got[2] == 0 && orbgpu::LastShimError() == rc);
        g_rc = 0;
        g_fail_at_call = -1;
    }
    orbgpu::ClearShimError();
    {   // nothing to do
        Graph g = make_graph();
        std::vector<int> got{1};
        g_calls = 0;
        Matcher().Fuse(std::vector<MockKF*>{}, g.points, 3.0f, got);
        CHECK(got.empty() && g_calls == 0);
        CHECK(Matcher().Fuse(g.targets[0], std::vector<MockMP*>{}, 3.0f) == 0 && g_calls == 0);
    }
    if (g_fail) return 1;
    std::printf("OK fuse_shim_check\n");
    return 0;
}
