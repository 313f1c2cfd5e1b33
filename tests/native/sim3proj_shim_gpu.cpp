// The Sim3 search members of include/orbgpu_matcher.hpp -- SearchByProjection(KF, Scw, ...), its vpMatchedKF
// overload, Fuse(KF, Scw, ...) and the batched form -- against the real liborbgpu.so on the GPU
// (tests/test_sim3proj_shim_gpu.py; links only liborbgpu).  Input: a scene file written by the test -- one
// keyframe, a point set with each entry's state, the pre-filled vpMatched entries, a holder kind per keypoint,
// and what the Python restatement of src/ORBmatcher.cc:496-733 / :1547-1651 (tests/sim3_projection_ref.py)
// expects.  The program builds mock KeyFrame / MapPoint objects from it, runs the drop-ins as LoopClosing does,
// and checks return values, vpMatched / vpMatchedKF and, for Fuse, the graph against step 7 (:1655-1672) applied
// to the expected best_idx on a second copy.
//
// File: int32 header {magic 0x53335072, nK, nP, nlevels}; floats: Tcw[12], Ow[3] (the pose the mock adapter's
// Sim3Pose returns), fx, fy, cx, cy, min_x, max_x, min_y, max_y, grid_inv_w, grid_inv_h, log scale factor,
// scale[nlevels]; keyframe: keypoints (28 B each), descriptors (32 B each), holder kind (1 B each: 0 no map
// point, 1 a map point, 3 a bad one), prematch (int32 each: -2 vpMatched[j] NULL, -1 a map point outside
// vpPoints, >= 0 that entry of vpPoints); points: pos (3 floats each), normal, min_dist, max_dist, descriptors,
// state (1 B each: 0 live, 2 isBad, 3 already in the keyframe); expected: matched[nK] and nmatches of the first
// form (th 5, ratio 1.0), the same of the second form (th 8, ratio 1.5), best_idx[nP] of Fuse (th 4).
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
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
    float pos[3] = {0, 0, 0}, normal[3] = {0, 0, 0}, min_dist = 0, max_dist = 0;
    uint8_t desc[32] = {};
    bool bad = false;
    int slot = -1;  // its index in the keyframe after AddObservation, -1: none
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<float> scale, geom;  // geom: the 26 leading floats of the file
    std::vector<MockMP*> mps;
    int levels_override = 0;
};
struct MockSim3 {
    const float* pose;  // Tcw[12], Ow[3]
};

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame*) { return nullptr; }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, &k->geom[15], 16); }
    static int Levels(KeyFrame* k) { return k->levels_override ? k->levels_override : (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static void FuseGeometry(KeyFrame* k, orb_fuse_kf_t* v) {
        const float* g = k->geom.data();
        orb_frame_view_t& f = v->frame;
        f.min_x = g[19]; f.max_x = g[20]; f.min_y = g[21]; f.max_y = g[22];
        f.grid_inv_w = g[23]; f.grid_inv_h = g[24];
        v->log_scale_factor = g[25];
    }
    static void Sim3Pose(const MockSim3& S, float Tcw[12], float Ow[3]) {
        std::memcpy(Tcw, S.pose, 48);
        std::memcpy(Ow, S.pose + 12, 12);
    }
    static std::set<MapPoint*> MapPointSet(KeyFrame* k) {
        std::set<MapPoint*> s(k->mps.begin(), k->mps.end());
        s.erase(nullptr);
        return s;
    }
    static MapPoint* GetMapPoint(KeyFrame* k, int idx) { return k->mps[idx]; }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->mps[idx] = p; }
    static void AddObservation(MapPoint* p, KeyFrame*, int idx) { p->slot = idx; }
    static bool IsBad(MapPoint* p) { return p->bad; }
    static void WorldPos(MapPoint* p, float X[3]) { std::memcpy(X, p->pos, 12); }
    static void Normal(MapPoint* p, float X[3]) { std::memcpy(X, p->normal, 12); }
    static float MinDistance(MapPoint* p) { return p->min_dist; }
    static float MaxDistance(MapPoint* p) { return p->max_dist; }
    static void Descriptor(MapPoint* p, uint8_t d[32]) { std::memcpy(d, p->desc, 32); }
};
using Matcher = orbgpu::ORBmatcher<Access>;

template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

struct Scene {
    int nK = 0, nP = 0, nlevels = 0;
    std::vector<float> geom, scale, pos, normal, mn, mx;
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> kdesc, holder, pdesc, state;
    std::vector<int32_t> prematch, matched1, n1, matched2, n2, best;
};

// one copy of the object graph
struct Graph {
    MockKF kf;
    std::vector<std::unique_ptr<MockMP>> store;
    std::vector<MockMP*> points;
    MockMP foreign;                  // a map point outside vpPoints
    std::vector<MockMP*> prematched; // vpMatched before the call
    std::vector<MockKF> srcs;        // vpPointsKFs[i] = &srcs[i % 3]
    MockMP* make() {
        store.emplace_back(new MockMP());
        return store.back().get();
    }
    explicit Graph(const Scene& s) : srcs(3) {
        kf.kps = s.kps;
        kf.desc = s.kdesc;
        kf.scale = s.scale;
        kf.geom = s.geom;
        kf.mps.assign(s.nK, nullptr);
        for (int j = 0; j < s.nK; ++j) {
            if (!s.holder[j]) continue;
            MockMP* q = make();
            q->bad = s.holder[j] == 3;
            kf.mps[j] = q;
        }
        int free_slot = 0;
        for (int i = 0; i < s.nP; ++i) {
            MockMP* p = make();
            std::memcpy(p->pos, &s.pos[3 * i], 12);
            std::memcpy(p->normal, &s.normal[3 * i], 12);
            p->min_dist = s.mn[i];
            p->max_dist = s.mx[i];
            std::memcpy(p->desc, &s.pdesc[32 * i], 32);
            p->bad = s.state[i] == 2;
            if (s.state[i] == 3) {  // already in the keyframe, in a slot without a map point
                while (free_slot < s.nK && kf.mps[free_slot]) ++free_slot;
                if (free_slot < s.nK) kf.mps[free_slot] = p;
            }
            points.push_back(p);
        }
        prematched.assign(s.nK, nullptr);
        for (int j = 0; j < s.nK; ++j)
            if (s.prematch[j] != -2) prematched[j] = s.prematch[j] < 0 ? &foreign : points[s.prematch[j]];
    }
    std::vector<MockKF*> point_kfs() {
        std::vector<MockKF*> v;
        for (size_t i = 0; i < points.size(); ++i) v.push_back(&srcs[i % 3]);
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: sim3proj_shim_gpu <scene file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[4];
    if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] != 0x53335072) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    Scene s;
    s.nK = hdr[1];
    s.nP = hdr[2];
    s.nlevels = hdr[3];
    const bool ok = read_vec(f, s.geom, 26) && read_vec(f, s.scale, s.nlevels) && read_vec(f, s.kps, s.nK) &&
                    read_vec(f, s.kdesc, (size_t)s.nK * 32) && read_vec(f, s.holder, s.nK) && read_vec(f, s.prematch, s.nK) &&
                    read_vec(f, s.pos, (size_t)s.nP * 3) && read_vec(f, s.normal, (size_t)s.nP * 3) && read_vec(f, s.mn, s.nP) &&
                    read_vec(f, s.mx, s.nP) && read_vec(f, s.pdesc, (size_t)s.nP * 32) && read_vec(f, s.state, s.nP) &&
                    read_vec(f, s.matched1, s.nK) && read_vec(f, s.n1, 1) && read_vec(f, s.matched2, s.nK) &&
                    read_vec(f, s.n2, 1) && read_vec(f, s.best, s.nP);
    std::fclose(f);
    if (!ok) {
        std::printf("short scene file\n");
        return 2;
    }
    MockSim3 S{s.geom.data()};
    Matcher m(0.75f, true);
    orbgpu::ClearShimError();
    auto expect = [&](Graph& g, const std::vector<int32_t>& matched) {
        std::vector<MockMP*> v = g.prematched;
        for (int j = 0; j < s.nK; ++j)
            if (matched[j] >= 0) v[j] = g.points[matched[j]];
        return v;
    };
    {   // the first form (LoopClosing.cc:1005)
        Graph g(s);
        std::vector<MockMP*> vm = g.prematched;
        const int n = m.SearchByProjection(&g.kf, S, g.points, vm, 5, 1.0f);
        CHECK(orbgpu::LastShimError() == ORB_OK && n == s.n1[0] && n > 0);
        CHECK(vm == expect(g, s.matched1) && vm != g.prematched);
        std::printf("SearchByProjection: %d matches (expected %d)\n", n, s.n1[0]);
        // two jobs in one call equal the single call
        std::vector<std::vector<MockMP*>> vpts{g.points, g.points}, vvm{g.prematched, g.prematched};
        std::vector<int> vn;
        m.SearchByProjection(std::vector<std::pair<MockKF*, MockSim3>>{{&g.kf, S}, {&g.kf, S}}, vpts, vvm, 5, 1.0f, vn);
        CHECK((vn == std::vector<int>{n, n}) && vvm[0] == vm && vvm[1] == vm);
    }
    {   // the second form (LoopClosing.cc:976)
        Graph g(s);
        std::vector<MockMP*> vm = g.prematched;
        std::vector<MockKF*> vkf(s.nK, nullptr), pkfs = g.point_kfs();
        const int n = m.SearchByProjection(&g.kf, S, g.points, pkfs, vm, vkf, 8, 1.5f);
        CHECK(orbgpu::LastShimError() == ORB_OK && n == s.n2[0] && n > 0);
        CHECK(vm == expect(g, s.matched2));
        for (int j = 0; j < s.nK; ++j) CHECK(vkf[j] == (s.matched2[j] >= 0 ? pkfs[s.matched2[j]] : nullptr));
        std::printf("SearchByProjection with keyframes: %d matches (expected %d)\n", n, s.n2[0]);
    }
    {   // Fuse (LoopClosing.cc:2712): step 7 on a second copy with the expected best_idx
        Graph g(s), want(s);
        std::vector<MockMP*> rep(s.nP, nullptr), rep_want(s.nP, nullptr);
        int n_want = 0, added = 0, replaced = 0;
        for (int i = 0; i < s.nP; ++i) {
            if (s.best[i] < 0) continue;
            MockMP* in = want.kf.mps[s.best[i]];
            if (in) {
                if (!in->bad) {
                    rep_want[i] = in;
                    ++replaced;
                }
            } else {
                want.points[i]->slot = s.best[i];
                want.kf.mps[s.best[i]] = want.points[i];
                ++added;
            }
            ++n_want;
        }
        const int n = m.Fuse(&g.kf, S, g.points, 4.0f, rep);
        CHECK(orbgpu::LastShimError() == ORB_OK && n == n_want && added > 0 && replaced > 0 && n > added + replaced);
        auto index = [](const Graph& gr, const MockMP* p) {
            for (size_t i = 0; i < gr.store.size(); ++i)
                if (gr.store[i].get() == p) return (int)i;
            return -1;
        };
        for (int i = 0; i < s.nP; ++i) CHECK(index(g, rep[i]) == index(want, rep_want[i]));
        for (int j = 0; j < s.nK; ++j) CHECK(index(g, g.kf.mps[j]) == index(want, want.kf.mps[j]));
        for (int i = 0; i < s.nP; ++i) CHECK(g.points[i]->slot == want.points[i]->slot);
        std::printf("Fuse: %d fused (expected %d), %d added, %d to replace\n", n, n_want, added, replaced);
    }
    {   // an invalid view (13 levels): ORB_ERR_ARG from the library -> 0, nothing written
        Graph g(s);
        g.kf.levels_override = 13;
        std::vector<MockMP*> vm = g.prematched, rep(s.nP, nullptr);
        CHECK(m.SearchByProjection(&g.kf, S, g.points, vm, 5, 1.0f) == 0 && orbgpu::LastShimError() == ORB_ERR_ARG);
        CHECK(vm == g.prematched);
        orbgpu::ClearShimError();
        const std::vector<MockMP*> before = g.kf.mps;
        CHECK(m.Fuse(&g.kf, S, g.points, 4.0f, rep) == 0 && orbgpu::LastShimError() == ORB_ERR_ARG);
        CHECK(g.kf.mps == before && rep == std::vector<MockMP*>(s.nP, nullptr));
        orbgpu::ClearShimError();
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK sim3proj_shim_gpu\n");
    return 0;
}
