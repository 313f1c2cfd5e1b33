// CPU check of ORBmatcher::CreateNewMapPoints in include/orbgpu_matcher.hpp (step 6 of
// LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:888-909) on a mock KeyFrame / MapPoint graph.  The
// three C entries it calls are scripted test doubles (the kernels are compared with the restatement in
// tests/test_newpoints_gpu.py), so this runs without a GPU.  Checked:
//   * the arguments that reach the library: the views, the extra fields, the parameters, the search's
//     matches12 / counts handed to orb_create_new_map_points unchanged;
//   * step 6 in the order of the records: pass 1 (new MapPoint, both AddObservation, both AddMapPoint) for
//     every record, then ONE orb_compute_distinctive_descriptors call for all new points, then pass 2 (normal
//     and distances from the record, the caller's `added` hook) -- as an operation log;
//   * two records of one neighbour sharing idx2: the later AddMapPoint overwrites the keyframe's slot, the
//     earlier point keeps its observation, as upstream's does;
//   * an ORB_ERR_* from each of the three entries: no points and an untouched graph for the first two, the
//     points created with their descriptors left alone for the third; the code in orbgpu::LastShimError();
//     nothing throws.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
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

static std::vector<std::string> g_log;
static void Log(const char* what, int a = -1, int b = -1, int c = -1) {
    char buf[96];
    std::snprintf(buf, sizeof(buf), "%s %d %d %d", what, a, b, c);
    g_log.push_back(buf);
}

// ---- mock reference objects ------------------------------------------------------------------------
struct MockKF;
struct MockMP {
    int id = 0;
    float pos[3] = {}, normal[3] = {}, min_dist = 0, max_dist = 0;
    uint8_t desc[32] = {};
    MockKF* ref = nullptr;
    std::map<MockKF*, std::tuple<int, int>> obs;
};
struct MockKF {
    int id = 0;
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<float> ur, depth;
    std::vector<MockMP*> mps;
    std::vector<float> scale{1.f, 1.2f}, sigma2{1.f, 1.44f};
    std::map<uint32_t, std::vector<unsigned>> fv;
    explicit MockKF(int id_, int n) : id(id_), kps(n), desc(32 * n), ur(n, -1.f), depth(n, -1.f), mps(n, nullptr) {
        for (int i = 0; i < n; ++i) {
            kps[i] = orb_keypoint_t{};
            kps[i].x = 10.f * i;
            std::memset(&desc[32 * i], 16 * id + i, 32);
        }
    }
};
static std::vector<MockMP*> g_points;  // every MockMP made by NewMapPoint (owned here)

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame* k) { return k->ur.data(); }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static const std::map<uint32_t, std::vector<unsigned>>& FeatVec(KeyFrame* k) { return k->fv; }
    static void Pinhole(KeyFrame*, float K[4]) { K[0] = K[1] = 500.f; K[2] = 320.f; K[3] = 240.f; }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static orb_kf_pair_geom_t PairGeometry(KeyFrame* a, KeyFrame* b) {
        orb_kf_pair_geom_t g{};
        g.t12[0] = (float)(b->id - a->id);
        return g;
    }
    static void NewPointsGeometry(KeyFrame* k, orb_newpoints_kf_extra_t* e) {
        const float T[12] = {1, 0, 0, -(float)k->id, 0, 1, 0, 0, 0, 0, 1, 0};
        std::memcpy(e->Tcw, T, sizeof(T));
        e->Ow[0] = (float)k->id;
        e->mb = 0.1f; e->mbf = 50.f; e->invfx = e->invfy = 1.f / 500.f;
        e->depth = k->depth.data();
        e->kps_raw = nullptr;
    }
    static MapPoint* NewMapPoint(const float x3d[3], KeyFrame* ref) {
        MockMP* p = new MockMP();
        p->id = (int)g_points.size();
        std::memcpy(p->pos, x3d, 12);
        p->ref = ref;
        g_points.push_back(p);
        Log("new", p->id, ref->id);
        return p;
    }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) {
        p->obs[k] = std::make_tuple(idx, -1);
        Log("obs", p->id, k->id, idx);
    }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) {
        k->mps[idx] = p;
        Log("addmp", p->id, k->id, idx);
    }
    static void SetNormalAndDepth(MapPoint* p, const float n[3], float mn, float mx) {
        std::memcpy(p->normal, n, 12);
        p->min_dist = mn;
        p->max_dist = mx;
        Log("normal", p->id);
    }
    // ComputeDistinctiveDescriptors
    static bool IsBad(MapPoint*) { return false; }
    static bool IsBad(KeyFrame*) { return false; }
    static std::map<KeyFrame*, std::tuple<int, int>> ObservationMap(MapPoint* p) { return p->obs; }
    static const uint8_t* DescriptorRow(KeyFrame* k, int idx) { return &k->desc[32 * idx]; }
    static void SetDescriptor(MapPoint* p, const uint8_t d[32]) {
        std::memcpy(p->desc, d, 32);
        Log("desc", p->id);
    }
};
using Matcher = orbgpu::ORBmatcher<Access>;

// ---- the C ABI's test doubles ----------------------------------------------------------------------
static int g_rc_search = 0, g_rc_new = 0, g_rc_desc = 0;
static int g_calls_search = 0, g_calls_new = 0, g_calls_desc = 0, g_desc_points = 0;
static std::vector<std::vector<int32_t>> g_script_m12;   // per neighbour: matches12 row
static std::vector<orb_newpoint_t> g_script_rec;         // what orb_create_new_map_points reports
static std::vector<int32_t> g_seen_m12, g_seen_cnt;
static orb_newpoints_params_t g_seen_prm;
static orb_newpoints_kf_t g_seen_kf1, g_seen_kf2_last;
static int g_seen_coarse = -1, g_seen_only_stereo = -1;
static std::string g_err = "injected";

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_matcher_create(float, int, orb_matcher_t* out) {
    *out = reinterpret_cast<orb_matcher_t>(new int(0));
    return ORB_OK;
}
int orb_matcher_destroy(orb_matcher_t m) {
    delete reinterpret_cast<int*>(m);
    return ORB_OK;
}
int orb_search_for_triangulation(orb_matcher_t, const orb_kf_view_t* kf1, const orb_kf_view_t*, const orb_kf_pair_geom_t*,
                                 int n_pairs, int only_stereo, int coarse, int32_t* matches12, int32_t* n_matches) {
    ++g_calls_search;
    Log("search", n_pairs);
    if (g_rc_search) return g_rc_search;
    g_seen_only_stereo = only_stereo;
    g_seen_coarse = coarse;
    for (int p = 0; p < n_pairs; ++p) {
        int c = 0;
        for (int i = 0; i < kf1->n; ++i) {
            matches12[(size_t)p * kf1->n + i] = g_script_m12[p][i];
            c += g_script_m12[p][i] >= 0;
        }
        n_matches[p] = c;
    }
    return ORB_OK;
}
int orb_create_new_map_points(orb_matcher_t, const orb_newpoints_kf_t* kf1, const orb_newpoints_kf_t* kf2s, int n_pairs,
                              const orb_newpoints_params_t* prm, const int32_t* matches12, const int32_t* n_matches,
                              const orb_newpoints_out_t* out) {
    ++g_calls_new;
    Log("triangulate", n_pairs);
    if (g_rc_new) return g_rc_new;
    g_seen_m12.assign(matches12, matches12 + (size_t)n_pairs * kf1->view.n);
    g_seen_cnt.assign(n_matches, n_matches + n_pairs);
    g_seen_prm = *prm;
    g_seen_kf1 = *kf1;
    g_seen_kf2_last = kf2s[n_pairs - 1];
    for (size_t r = 0; r < g_script_rec.size(); ++r) out->records[r] = g_script_rec[r];
    *out->n_new = (int32_t)g_script_rec.size();
    return ORB_OK;
}
// (stands in for the median-distance choice: a point's first row)
int orb_compute_distinctive_descriptors(orb_matcher_t, const uint8_t* desc, const int32_t* offsets, int n_points,
                                        int32_t* best, uint8_t* out) {
    ++g_calls_desc;
    g_desc_points = n_points;
    Log("descriptors", n_points);
    if (g_rc_desc) return g_rc_desc;
    for (int p = 0; p < n_points; ++p) {
        best[p] = 0;
        std::memcpy(out + 32 * p, desc + 32 * (size_t)offsets[p], 32);
    }
    return ORB_OK;
}
}  // extern "C"

static orb_newpoint_t Rec(int p, int idx1, int idx2, float x, int stereo) {
    orb_newpoint_t r{};
    r.p = p; r.idx1 = idx1; r.idx2 = idx2;
    r.x3d[0] = x; r.x3d[1] = 2 * x; r.x3d[2] = 5.f;
    r.from_stereo = stereo;
    r.normal[2] = 1.f; r.normal[0] = 0.01f * x;
    r.min_dist = 1.f + x; r.max_dist = 4.f + x;
    return r;
}

struct Graph {
    MockKF kf1{1, 4}, a{2, 3}, b{3, 3};
    std::vector<MockKF*> nb{&a, &b};
};

static void Reset() {
    g_log.clear();
    for (MockMP* p : g_points) delete p;
    g_points.clear();
    g_rc_search = g_rc_new = g_rc_desc = 0;
    g_calls_search = g_calls_new = g_calls_desc = g_desc_points = 0;
    orbgpu::ClearShimError();
    // neighbour 0: idx1 0 -> 2, idx1 1 -> 2 (shared idx2), idx1 3 -> 0; neighbour 1: idx1 0 -> 1 (TAKEN), 2 -> 1
    g_script_m12 = {{2, 2, -1, 0}, {1, -1, 1, -1}};
    g_script_rec = {Rec(0, 0, 2, 1.f, 0), Rec(0, 1, 2, 2.f, 1), Rec(0, 3, 0, 3.f, 0), Rec(1, 2, 1, 4.f, 0)};
}

static void TestStep6() {
    Reset();
    Graph g;
    Matcher::NewPointsParams prm;
    prm.inertial = true; prm.far_points = true; prm.th_far_points = 20.f; prm.ratio_factor = 1.8f; prm.coarse = true;
    std::vector<int> hook;
    std::vector<orb_newpoint_t> rec;
    const auto made = Matcher(0.6f, false).CreateNewMapPoints(
        &g.kf1, g.nb, prm, [&](MockMP* p) { hook.push_back(p->id); Log("added", p->id); }, &rec);
    CHECK(orbgpu::LastShimError() == ORB_OK);
    CHECK(g_calls_search == 1 && g_calls_new == 1 && g_calls_desc == 1 && g_desc_points == 4);
    // what reached the library
    CHECK(g_seen_only_stereo == 0 && g_seen_coarse == 1);
    CHECK((g_seen_m12 == std::vector<int32_t>{2, 2, -1, 0, 1, -1, 1, -1}));
    CHECK((g_seen_cnt == std::vector<int32_t>{3, 2}));
    CHECK(g_seen_prm.inertial == 1 && g_seen_prm.far_points == 1 && g_seen_prm.th_far_points == 20.f &&
          g_seen_prm.ratio_factor == 1.8f);
    CHECK(g_seen_kf1.view.n == 4 && g_seen_kf1.view.kps_un == g.kf1.kps.data() && g_seen_kf1.extra.Ow[0] == 1.f &&
          g_seen_kf1.extra.Tcw[3] == -1.f && g_seen_kf1.extra.mbf == 50.f && g_seen_kf1.extra.depth == g.kf1.depth.data());
    CHECK(g_seen_kf2_last.view.n == 3 && g_seen_kf2_last.extra.Ow[0] == 3.f && g_seen_kf2_last.view.u_right == g.b.ur.data());
    // the result and the records
    CHECK(made.size() == 4 && rec.size() == 4 && rec[1].idx1 == 1 && rec[3].p == 1);
    CHECK((hook == std::vector<int>{0, 1, 2, 3}));
    // step 6 in order
    const std::vector<std::string> want = {
        "search 2 -1 -1", "triangulate 2 -1 -1",
        "new 0 1 -1", "obs 0 1 0", "obs 0 2 2", "addmp 0 1 0", "addmp 0 2 2",
        "new 1 1 -1", "obs 1 1 1", "obs 1 2 2", "addmp 1 1 1", "addmp 1 2 2",
        "new 2 1 -1", "obs 2 1 3", "obs 2 2 0", "addmp 2 1 3", "addmp 2 2 0",
        "new 3 1 -1", "obs 3 1 2", "obs 3 3 1", "addmp 3 1 2", "addmp 3 3 1",
        "descriptors 4 -1 -1", "desc 0 -1 -1", "desc 1 -1 -1", "desc 2 -1 -1", "desc 3 -1 -1",
        "normal 0 -1 -1", "added 0 -1 -1", "normal 1 -1 -1", "added 1 -1 -1", "normal 2 -1 -1", "added 2 -1 -1",
        "normal 3 -1 -1", "added 3 -1 -1"};
    CHECK(g_log == want);
    if (g_log != want)
        for (const auto& l : g_log) std::printf("  log: %s\n", l.c_str());
    // the graph: keyframe 1's slots, the shared idx2 overwritten by the later record, both points observing it
    CHECK(g.kf1.mps[0] == made[0] && g.kf1.mps[1] == made[1] && g.kf1.mps[3] == made[2] && g.kf1.mps[2] == made[3]);
    CHECK(g.a.mps[2] == made[1] && g.a.mps[0] == made[2] && g.a.mps[1] == nullptr);
    CHECK(std::get<0>(made[0]->obs[&g.a]) == 2 && std::get<0>(made[1]->obs[&g.a]) == 2);
    CHECK(g.b.mps[1] == made[3] && g.b.mps[0] == nullptr);
    for (size_t r = 0; r < made.size(); ++r) {
        const MockMP* p = made[r];
        CHECK(p->ref == &g.kf1 && p->obs.size() == 2);
        CHECK(p->pos[0] == g_script_rec[r].x3d[0] && p->pos[1] == g_script_rec[r].x3d[1] && p->pos[2] == 5.f);
        CHECK(p->normal[0] == g_script_rec[r].normal[0] && p->normal[2] == 1.f);
        CHECK(p->min_dist == g_script_rec[r].min_dist && p->max_dist == g_script_rec[r].max_dist);
        CHECK(p->desc[0] == 16 * 1 + g_script_rec[r].idx1);  // the first row: keyframe 1's (the map's first key)
    }
}

static void TestNoNeighbours() {
    Reset();
    Graph g;
    const auto made = Matcher(0.6f, false).CreateNewMapPoints(&g.kf1, {}, Matcher::NewPointsParams());
    CHECK(made.empty() && g_calls_search == 0 && g_calls_new == 0 && g_log.empty());
    // no record: no descriptor call either
    Reset();
    g_script_rec.clear();
    const auto none = Matcher(0.6f, false).CreateNewMapPoints(&g.kf1, g.nb, Matcher::NewPointsParams());
    CHECK(none.empty() && g_calls_new == 1 && g_calls_desc == 0 && orbgpu::LastShimError() == ORB_OK);
}

static bool Untouched(const Graph& g) {
    for (const MockKF* k : {&g.kf1, &g.a, &g.b})
        for (const MockMP* p : k->mps)
            if (p) return false;
    return true;
}

static void TestInjectedErrors() {
    const int codes[] = {ORB_ERR_ARG, ORB_ERR_CAPACITY, ORB_ERR_DEVICE, ORB_ERR_INTERNAL};
    for (int code : codes) {
        for (int where = 0; where < 3; ++where) {
            Reset();
            Graph g;
            (where == 0 ? g_rc_search : where == 1 ? g_rc_new : g_rc_desc) = code;
            std::vector<orb_newpoint_t> rec{Rec(0, 0, 0, 0.f, 0)};
            int hooks = 0;
            std::vector<MockMP*> made;
            bool threw = false;
            try {
                made = Matcher(0.6f, false).CreateNewMapPoints(&g.kf1, g.nb, Matcher::NewPointsParams(),
                                                               [&](MockMP*) { ++hooks; }, &rec);
            } catch (...) {
                threw = true;
            }
            CHECK(!threw);
            CHECK(orbgpu::LastShimError() == code);
            CHECK(orbgpu::LastShimMessage().find("injected") != std::string::npos);
            if (where < 2) {  // nothing created, nothing mutated
                CHECK(made.empty() && rec.empty() && hooks == 0 && g_points.empty() && Untouched(g));
                CHECK(g_calls_new == (where == 1 ? 1 : 0) && g_calls_desc == 0);
            } else {  // the points exist; their descriptors stay as constructed
                CHECK(made.size() == 4 && hooks == 4 && rec.size() == 4);
                for (const MockMP* p : made) CHECK(p->desc[0] == 0 && p->max_dist > 0);
            }
        }
    }
    // a record naming a neighbour or a keypoint that does not exist: nothing is created
    for (const orb_newpoint_t& bad : {Rec(7, 1, 0, 1.f, 0), Rec(0, 4, 0, 1.f, 0), Rec(1, 1, 3, 1.f, 0)}) {
        Reset();
        Graph g;
        g_script_rec = {Rec(0, 0, 2, 1.f, 0), bad};
        const auto made = Matcher(0.6f, false).CreateNewMapPoints(&g.kf1, g.nb, Matcher::NewPointsParams());
        CHECK(made.empty() && g_points.empty() && Untouched(g) && orbgpu::LastShimError() == ORB_ERR_INTERNAL);
    }
}

int main() {
    TestStep6();
    TestNoNeighbours();
    TestInjectedErrors();
    for (MockMP* p : g_points) delete p;
    if (g_fail) {
        std::printf("FAILED newpoints_shim_check: %d checks\n", g_fail);
        return 1;
    }
    std::printf("OK newpoints_shim_check\n");
    return 0;
}
