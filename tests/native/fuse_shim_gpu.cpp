// ORBmatcher::Fuse(pKF, vpMapPoints, th) of include/orbgpu_matcher.hpp against the real liborbgpu.so on the
// GPU (tests/test_fuse_shim_gpu.py; links only liborbgpu).  Input: a scene file written by the test -- one
// keyframe, a point set with each entry's state, a holder kind per keypoint, and the best_idx the Python
// restatement of src/ORBmatcher.cc:1356-1506 (tests/fuse_ref.py) expects for the unskipped points.  The
// program builds mock KeyFrame / MapPoint objects from it, runs the drop-in as LocalMapping::SearchInNeighbors
// does, and checks the return value and the graph against step 7 (:1506-1527) applied to the expected
// best_idx on a second copy of the graph.
//
// File: int32 header {magic 0x46757365, nK, nP, nlevels}; floats: Tcw[12], Ow[3], fx, fy, cx, cy, bf, min_x,
// max_x, min_y, max_y, grid_inv_w, grid_inv_h, log scale factor, scale[nlevels], inv_sigma2[nlevels]; keyframe:
// keypoints (28 B each), descriptors (32 B each), u_right (float each), holder kind (1 B each: 0 no map point,
// 1 a map point with one observation, 2 one with five, 3 a bad one); points: pos (3 floats each), normal,
// min_dist, max_dist, descriptors, state (1 B each: 0 live, 1 NULL, 2 isBad, 3 already in the keyframe);
// expected: best_idx[nP] (int32, -1 for the points not live).
#include <cstdio>
#include <cstring>
#include <memory>
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
    int nobs = 1;    // Observations()
    int slot = -1;   // its index in the keyframe, -1: not in it
    MockKF* kf = nullptr;
    MockMP* replaced = nullptr;
};
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<float> ur, scale, inv_sigma2, geom;  // geom: the 27 leading floats of the file
    std::vector<MockMP*> mps;
    int levels_override = 0;
};
// MapPoint::Replace (src/MapPoint.cc:330-378) as far as one keyframe shows it
static void replace(MockMP* p, MockMP* by) {
    if (p == by) return;
    p->bad = true;
    p->replaced = by;
    if (p->slot >= 0) {
        if (by->slot < 0) {
            p->kf->mps[p->slot] = by;
            by->slot = p->slot;
        } else {
            p->kf->mps[p->slot] = nullptr;
        }
    }
    by->nobs += p->nobs;
    p->nobs = 0;
    p->slot = -1;
}

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame* k) { return k->ur.data(); }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, &k->geom[15], 16); }
    static int Levels(KeyFrame* k) { return k->levels_override ? k->levels_override : (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static void FuseGeometry(KeyFrame* k, orb_fuse_kf_t* v) {
        const float* g = k->geom.data();
        orb_frame_view_t& f = v->frame;
        std::memcpy(f.Tcw, g, 48);
        std::memcpy(v->Ow, g + 12, 12);
        f.bf = g[19];
        f.b = g[19] / g[15];
        f.min_x = g[20]; f.max_x = g[21]; f.min_y = g[22]; f.max_y = g[23];
        f.grid_inv_w = g[24]; f.grid_inv_h = g[25];
        v->log_scale_factor = g[26];
        v->inv_level_sigma2 = k->inv_sigma2.data();
    }
    static MapPoint* GetMapPoint(KeyFrame* k, int idx) { return k->mps[idx]; }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->mps[idx] = p; }
    static bool IsInKeyFrame(MapPoint* p, KeyFrame*) { return p->slot >= 0; }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) {
        p->slot = idx;
        p->kf = k;
        ++p->nobs;
    }
    static void Replace(MapPoint* p, MapPoint* by) { replace(p, by); }
    static int Observations(MapPoint* p) { return p->nobs; }
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
    std::vector<float> geom, scale, inv_sigma2, ur, pos, normal, mn, mx;
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> kdesc, holder, pdesc, state;
    std::vector<int32_t> best;
};

// one copy of the object graph
struct Graph {
    MockKF kf;
    std::vector<std::unique_ptr<MockMP>> store;
    std::vector<MockMP*> points;
    MockMP* make() {
        store.emplace_back(new MockMP());
        store.back()->kf = &kf;
        return store.back().get();
    }
    explicit Graph(const Scene& s) {
        kf.kps = s.kps;
        kf.desc = s.kdesc;
        kf.ur = s.ur;
        kf.scale = s.scale;
        kf.inv_sigma2 = s.inv_sigma2;
        kf.geom = s.geom;
        kf.mps.assign(s.nK, nullptr);
        for (int j = 0; j < s.nK; ++j) {
            if (!s.holder[j]) continue;
            MockMP* q = make();
            q->slot = j;
            q->nobs = s.holder[j] == 2 ? 5 : 1;
            q->bad = s.holder[j] == 3;
            kf.mps[j] = q;
        }
        int free_slot = 0;
        for (int i = 0; i < s.nP; ++i) {
            if (s.state[i] == 1) {
                points.push_back(nullptr);
                continue;
            }
            MockMP* p = make();
            std::memcpy(p->pos, &s.pos[3 * i], 12);
            std::memcpy(p->normal, &s.normal[3 * i], 12);
            p->min_dist = s.mn[i];
            p->max_dist = s.mx[i];
            std::memcpy(p->desc, &s.pdesc[32 * i], 32);
            p->nobs = 2;
            p->bad = s.state[i] == 2;
            if (s.state[i] == 3) {  // already observed by the keyframe, in a slot without a map point
                while (free_slot < s.nK && kf.mps[free_slot]) ++free_slot;
                if (free_slot < s.nK) {
                    p->slot = free_slot;
                    kf.mps[free_slot] = p;
                } else {
                    p->slot = 0;
                }
            }
            points.push_back(p);
        }
    }
    // (slot, bad, observations, the replacement's index in the store) per object, and the keyframe's slots
    std::vector<int> dump() const {
        auto index = [&](const MockMP* p) {
            for (size_t i = 0; i < store.size(); ++i)
                if (store[i].get() == p) return (int)i;
            return -1;
        };
        std::vector<int> d;
        for (const auto& p : store) {
            d.push_back(p->slot);
            d.push_back(p->bad);
            d.push_back(p->nobs);
            d.push_back(index(p->replaced));
        }
        for (MockMP* p : kf.mps) d.push_back(index(p));
        return d;
    }
};

// step 7 (src/ORBmatcher.cc:1506-1527) with the search's answers given
static int apply_expected(Graph& g, const std::vector<int32_t>& best) {
    int nFused = 0;
    for (size_t i = 0; i < g.points.size(); ++i) {
        MockMP* pMP = g.points[i];
        if (!pMP || pMP->bad || pMP->slot >= 0 || best[i] < 0) continue;
        MockMP* in = g.kf.mps[best[i]];
        if (in) {
            if (!in->bad) {
                if (in->nobs > pMP->nobs) replace(pMP, in);
                else replace(in, pMP);
            }
        } else {
            pMP->slot = best[i];
            ++pMP->nobs;
            g.kf.mps[best[i]] = pMP;
        }
        ++nFused;
    }
    return nFused;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: fuse_shim_gpu <scene file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[4];
    if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] != 0x46757365) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    Scene s;
    s.nK = hdr[1];
    s.nP = hdr[2];
    s.nlevels = hdr[3];
    const bool ok = read_vec(f, s.geom, 27) && read_vec(f, s.scale, s.nlevels) && read_vec(f, s.inv_sigma2, s.nlevels) &&
                    read_vec(f, s.kps, s.nK) && read_vec(f, s.kdesc, (size_t)s.nK * 32) && read_vec(f, s.ur, s.nK) &&
                    read_vec(f, s.holder, s.nK) && read_vec(f, s.pos, (size_t)s.nP * 3) &&
                    read_vec(f, s.normal, (size_t)s.nP * 3) && read_vec(f, s.mn, s.nP) && read_vec(f, s.mx, s.nP) &&
                    read_vec(f, s.pdesc, (size_t)s.nP * 32) && read_vec(f, s.state, s.nP) && read_vec(f, s.best, s.nP);
    std::fclose(f);
    if (!ok) {
        std::printf("short scene file\n");
        return 2;
    }
    Graph want(s), got(s);
    const std::vector<int> before = got.dump();
    const int n_want = apply_expected(want, s.best);
    const std::vector<int> want_first = want.dump();
    orbgpu::ClearShimError();
    const int n = Matcher(0.6f, false).Fuse(&got.kf, got.points, 3.0f);
    CHECK(orbgpu::LastShimError() == ORB_OK);
    CHECK(n == n_want && n > 0);
    CHECK(got.dump() == want_first);
    CHECK(got.dump() != before);
    int points_replaced = 0, all_replaced = 0;
    for (MockMP* p : got.points) points_replaced += p && p->replaced;
    for (const auto& p : got.store) all_replaced += p->replaced != nullptr;
    // both directions of Replace occur, and observations are added to free keypoints
    CHECK(points_replaced > 0 && all_replaced > points_replaced && n > all_replaced);
    std::printf("Fuse: %d fused (expected %d), %d points replaced, %d keyframe map points replaced\n", n, n_want,
                points_replaced, all_replaced - points_replaced);
    // a second call on the fused graph: a fused point is now in the keyframe or bad and is skipped; what is
    // left are the points whose best keypoint holds a bad map point (counted again, nothing changes)
    {
        const int n2_want = apply_expected(want, s.best);
        CHECK(Matcher(0.6f, false).Fuse(&got.kf, got.points, 3.0f) == n2_want && n2_want < n_want);
        CHECK(got.dump() == want.dump() && orbgpu::LastShimError() == ORB_OK);
    }
    // an invalid view (13 levels): ORB_ERR_ARG from the library -> 0, nothing touched
    {
        Graph bad(s);
        bad.kf.levels_override = 13;
        CHECK(Matcher(0.6f, false).Fuse(&bad.kf, bad.points, 3.0f) == 0);
        CHECK(orbgpu::LastShimError() == ORB_ERR_ARG && bad.dump() == before);
        orbgpu::ClearShimError();
    }
    // the batched overload with the keyframe listed once equals the single call
    {
        Graph one(s);
        std::vector<int> v;
        Matcher(0.6f, false).Fuse(std::vector<MockKF*>{&one.kf}, one.points, 3.0f, v);
        CHECK(v.size() == 1 && v[0] == n_want && one.dump() == want_first);
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK fuse_shim_gpu\n");
    return 0;
}
