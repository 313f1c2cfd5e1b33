// ORBmatcher::CreateNewMapPoints of include/orbgpu_matcher.hpp against the real liborbgpu.so on the GPU (built
// by `make shims`, linking only liborbgpu; driven by tests/test_newpoints_shim_gpu.py).  A mock KeyFrame /
// MapPoint graph is built from a scene file; the member runs the batched search, the triangulation and step 6;
// the records and the graph after step 6 are compared with the records the Python entries gave for the same
// keyframes (themselves compared with the restatement by tests/test_newpoints_gpu.py).
//
// Scene file (little endian): int32 magic 0x4e657750, P, nlevels; float scale[nlevels], sigma2[nlevels];
// float th_far, ratio_factor; int32 inertial, far_points; then P + 1 keyframes (keyframe 1 first), each:
// int32 n, n_nodes, n_index; float Tcw[12], Ow[3], mb, mbf, fx, fy, cx, cy; orb_keypoint_t kps[n]; uint8
// desc[32 n]; float ur[n], depth[n]; uint32 node[n_nodes]; int32 offset[n_nodes + 1], index[n_index]; then
// int32 n_new and orb_newpoint_t expected[n_new].
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

struct MockKF;
struct MockMP {
    float pos[3] = {}, normal[3] = {}, min_dist = 0, max_dist = 0;
    uint8_t desc[32] = {};
    bool has_desc = false;
    MockKF* ref = nullptr;
    std::map<MockKF*, std::tuple<int, int>> obs;
};
struct MockKF {
    int n = 0;
    float Tcw[12], Ow[3], mb, mbf, K[4];
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<float> ur, depth;
    std::vector<MockMP*> mps;
    std::map<uint32_t, std::vector<unsigned>> fv;
    const std::vector<float>*scale, *sigma2;
};
static std::vector<MockMP*> g_points;

struct Access {
    using KeyFrame = MockKF;
    using MapPoint = MockMP;
    struct Frame {};
    static int N(KeyFrame* k) { return k->n; }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame* k) { return k->ur.data(); }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static const std::map<uint32_t, std::vector<unsigned>>& FeatVec(KeyFrame* k) { return k->fv; }
    static void Pinhole(KeyFrame* k, float K[4]) { std::memcpy(K, k->K, 16); }
    static int Levels(KeyFrame* k) { return (int)k->scale->size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale->data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2->data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static orb_kf_pair_geom_t PairGeometry(KeyFrame* a, KeyFrame* b) {
        orb_kf_pair_geom_t g{};
        orb_kf_pair_geometry(a->Tcw, b->Tcw, b->K[0], b->K[1], b->K[2], b->K[3], &g);
        return g;
    }
    static void NewPointsGeometry(KeyFrame* k, orb_newpoints_kf_extra_t* e) {
        std::memcpy(e->Tcw, k->Tcw, sizeof(k->Tcw));
        std::memcpy(e->Ow, k->Ow, sizeof(k->Ow));
        e->mb = k->mb; e->mbf = k->mbf; e->invfx = 1.0f / k->K[0]; e->invfy = 1.0f / k->K[1];
        e->depth = k->depth.data();
        e->kps_raw = nullptr;
    }
    static MapPoint* NewMapPoint(const float x3d[3], KeyFrame* ref) {
        MockMP* p = new MockMP();
        std::memcpy(p->pos, x3d, 12);
        p->ref = ref;
        g_points.push_back(p);
        return p;
    }
    static void AddObservation(MapPoint* p, KeyFrame* k, int idx) { p->obs[k] = std::make_tuple(idx, -1); }
    static void AddMapPoint(KeyFrame* k, MapPoint* p, int idx) { k->mps[idx] = p; }
    static void SetNormalAndDepth(MapPoint* p, const float n[3], float mn, float mx) {
        std::memcpy(p->normal, n, 12);
        p->min_dist = mn;
        p->max_dist = mx;
    }
    static bool IsBad(MapPoint*) { return false; }
    static bool IsBad(KeyFrame*) { return false; }
    static std::map<KeyFrame*, std::tuple<int, int>> ObservationMap(MapPoint* p) { return p->obs; }
    static const uint8_t* DescriptorRow(KeyFrame* k, int idx) { return &k->desc[32 * idx]; }
    static void SetDescriptor(MapPoint* p, const uint8_t d[32]) {
        std::memcpy(p->desc, d, 32);
        p->has_desc = true;
    }
};
using Matcher = orbgpu::ORBmatcher<Access>;

template <class T>
static bool Read(FILE* f, T* out, size_t n) {
    return n == 0 || std::fread(out, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (!Read(f, hdr, 3) || hdr[0] != 0x4e657750 || hdr[1] < 1 || hdr[2] < 1 || hdr[2] > 12) return 2;
    const int P = hdr[1], L = hdr[2];
    std::vector<float> scale(L), sigma2(L);
    float fprm[2];
    int32_t iprm[2];
    if (!Read(f, scale.data(), L) || !Read(f, sigma2.data(), L) || !Read(f, fprm, 2) || !Read(f, iprm, 2)) return 2;
    std::vector<MockKF> kfs(P + 1);
    for (MockKF& k : kfs) {
        int32_t h[3];
        float g[21];
        if (!Read(f, h, 3) || !Read(f, g, 21) || h[0] < 0 || h[1] < 0 || h[2] < 0) return 2;
        k.n = h[0];
        std::memcpy(k.Tcw, g, 48);
        std::memcpy(k.Ow, g + 12, 12);
        k.mb = g[15]; k.mbf = g[16];
        std::memcpy(k.K, g + 17, 16);
        k.kps.resize(k.n); k.desc.resize(32 * (size_t)k.n); k.ur.resize(k.n); k.depth.resize(k.n);
        k.mps.assign(k.n, nullptr);
        std::vector<uint32_t> node(h[1]);
        std::vector<int32_t> off(h[1] + 1), idx(h[2]);
        if (!Read(f, k.kps.data(), k.n) || !Read(f, k.desc.data(), 32 * (size_t)k.n) || !Read(f, k.ur.data(), k.n) ||
            !Read(f, k.depth.data(), k.n) || !Read(f, node.data(), node.size()) || !Read(f, off.data(), off.size()) ||
            !Read(f, idx.data(), idx.size()))
            return 2;
        for (int j = 0; j < h[1]; ++j)
            for (int q = off[j]; q < off[j + 1]; ++q) k.fv[node[j]].push_back((unsigned)idx[q]);
        k.scale = &scale;
        k.sigma2 = &sigma2;
    }
    int32_t n_new = 0;
    if (!Read(f, &n_new, 1) || n_new < 0) return 2;
    std::vector<orb_newpoint_t> want(n_new);
    if (!Read(f, want.data(), n_new)) return 2;
    std::fclose(f);

    std::vector<MockKF*> nb;
    for (int p = 0; p < P; ++p) nb.push_back(&kfs[1 + p]);
    Matcher::NewPointsParams prm;
    prm.inertial = iprm[0] != 0; prm.far_points = iprm[1] != 0; prm.th_far_points = fprm[0]; prm.ratio_factor = fprm[1];
    std::vector<orb_newpoint_t> rec;
    std::vector<MockMP*> added;
    const auto made = Matcher(0.6f, false).CreateNewMapPoints(&kfs[0], nb, prm, [&](MockMP* p) { added.push_back(p); }, &rec);
    CHECK(orbgpu::LastShimError() == ORB_OK);
    if (orbgpu::LastShimError() != ORB_OK) std::printf("shim error: %s\n", orbgpu::LastShimMessage().c_str());
    std::printf("%d neighbours, %d keypoints, %zu new points (expected %d)\n", P, kfs[0].n, made.size(), (int)n_new);
    CHECK((int)made.size() == n_new && rec.size() == made.size() && added == made);
    CHECK(rec.size() == want.size() && (rec.empty() || std::memcmp(rec.data(), want.data(), sizeof(orb_newpoint_t) * rec.size()) == 0));
    // the graph after step 6, replayed from the expected records
    std::vector<std::vector<int>> slot(P + 1);
    for (int k = 0; k <= P; ++k) slot[k].assign(kfs[k].n, -1);
    for (int r = 0; r < n_new && r < (int)made.size(); ++r) {
        slot[0][want[r].idx1] = r;
        slot[1 + want[r].p][want[r].idx2] = r;  // a shared idx2: the later record stays
    }
    int shared = 0;
    for (int k = 0; k <= P; ++k)
        for (int i = 0; i < kfs[k].n; ++i) CHECK(kfs[k].mps[i] == (slot[k][i] < 0 ? nullptr : made[slot[k][i]]));
    for (int r = 0; r < n_new && r < (int)made.size(); ++r) {
        MockMP* p = made[r];
        MockKF* k2 = &kfs[1 + want[r].p];
        CHECK(p->ref == &kfs[0] && p->obs.size() == 2);
        CHECK(std::get<0>(p->obs[&kfs[0]]) == want[r].idx1 && std::get<0>(p->obs[k2]) == want[r].idx2);
        CHECK(std::memcmp(p->pos, want[r].x3d, 12) == 0 && std::memcmp(p->normal, want[r].normal, 12) == 0);
        CHECK(p->min_dist == want[r].min_dist && p->max_dist == want[r].max_dist);
        // two observations: the median distance of either row is their distance, the first row wins the tie
        MockKF* first = p->obs.begin()->first;
        CHECK(p->has_desc && std::memcmp(p->desc, &first->desc[32 * (size_t)std::get<0>(p->obs.begin()->second)], 32) == 0);
        if (slot[1 + want[r].p][want[r].idx2] != r) ++shared;
    }
    std::printf("%d records lost their idx2 slot to a later record\n", shared);
    for (MockMP* p : g_points) delete p;
    if (g_fail) {
        std::printf("FAILED newpoints_shim_gpu: %d checks\n", g_fail);
        return 1;
    }
    std::printf("OK newpoints_shim_gpu\n");
    return 0;
}
