// CPU check of ORBmatcher::SearchByBoW in include/orbgpu_matcher.hpp (src/ORBmatcher.cc:260-494) on mock
// KeyFrame / Frame / MapPoint objects.  orb_search_by_bow is a test double that records the views the
// shim hands across the ABI and returns a chosen match row, so this runs without a GPU; the HIP kernel
// is compared with the reference restatement in tests/test_bow_search_gpu.py.  Checked:
//   * the keyframe view (keypoints, descriptors, FeatureVector as ascending node ids + CSR indices in
//     each node's order) and its usable flags: the map point is non-NULL and not isBad() (:307-313);
//   * the frame view: N, keypoints, descriptors and F.mFeatVec, as one orb_kf_view_t;
//   * the handle: ORBmatcher(0.7, true)'s ratio and orientation flag;
//   * vpMapPointMatches: F.N NULL entries first (:266), then pKF's map point for every matched keypoint,
//     whatever the vector held before;
//   * an ORB_ERR_* from the library: 0 returned, every entry NULL, the code in orbgpu::LastShimError();
//   * Supports(KeyFrame*, Frame): false for a two-camera keyframe or frame.
#include <cstdio>
#include <cstring>
#include <map>
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
struct MockMP {
    bool bad = false;
};
using FeatureVector = std::map<unsigned int, std::vector<unsigned int>>;
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<MockMP*> mps;
    FeatureVector fv;
    std::vector<float> scale{1.f, 1.2f}, sigma2{1.f, 1.44f};
    bool cam2 = false;
};
struct MockFrame {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    FeatureVector fv;
    std::vector<float> scale{1.f, 1.2f};
    int nleft = -1;
};

struct Access {
    using KeyFrame = MockKF;
    using Frame = MockFrame;
    using MapPoint = MockMP;
    static int N(KeyFrame* k) { return (int)k->kps.size(); }
    static const orb_keypoint_t* KeysUn(KeyFrame* k) { return k->kps.data(); }
    static const uint8_t* Descriptors(KeyFrame* k) { return k->desc.data(); }
    static const float* URight(KeyFrame*) { return nullptr; }
    static std::vector<MapPoint*> MapPointMatches(KeyFrame* k) { return k->mps; }
    static const FeatureVector& FeatVec(KeyFrame* k) { return k->fv; }
    static const FeatureVector& FeatVec(const Frame& f) { return f.fv; }
    static void Pinhole(KeyFrame*, float K[4]) { K[0] = K[1] = 450.f; K[2] = 370.f; K[3] = 240.f; }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2.data(); }
    static bool SingleCamera(KeyFrame* k) { return !k->cam2; }
    static orb_frame_view_t View(const Frame& f) {
        orb_frame_view_t v{};
        v.n = (int)f.kps.size();
        v.kps_un = f.kps.data();
        v.desc = f.desc.data();
        v.nlevels = (int)f.scale.size();
        v.scale_factors = f.scale.data();
        return v;
    }
    static bool SingleCamera(const Frame& f) { return f.nleft == -1; }
    static bool IsBad(MapPoint* p) { return p->bad; }
};
using Matcher = orbgpu::ORBmatcher<Access>;

// ---- test doubles of the C ABI -------------------------------------------------------------------
struct FakeHandle {
    float nnratio;
    int check_ori;
};
static int g_rc = 0, g_calls = 0;
static std::string g_err;
struct SeenView {
    int n = -1, n_nodes = -1;
    const orb_keypoint_t* kps = nullptr;
    const uint8_t* desc = nullptr;
    std::vector<uint32_t> nodes;
    std::vector<int32_t> offset, index;
    void take(const orb_kf_view_t* v) {
        n = v->n;
        n_nodes = v->n_nodes;
        kps = v->kps_un;
        desc = v->desc;
        nodes.assign(v->fv_node, v->fv_node + v->n_nodes);
        offset.assign(v->fv_offset, v->fv_offset + v->n_nodes + 1);
        index.assign(v->fv_index, v->fv_index + v->fv_offset[v->n_nodes]);
    }
};
static struct {
    FakeHandle* h = nullptr;
    int n_kfs = 0;
    SeenView kf, frame;
    std::vector<uint8_t> usable;
} g_seen;
static std::vector<int32_t> g_match;  // the row the double returns
static int g_count = 0;

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_descriptor_distance(const uint8_t*, const uint8_t*) { return 0; }
int orb_matcher_create(float nnratio, int check_orientation, orb_matcher_t* out) {
    *out = reinterpret_cast<orb_matcher_t>(new FakeHandle{nnratio, check_orientation});
    return ORB_OK;
}
int orb_matcher_destroy(orb_matcher_t m) {
    delete reinterpret_cast<FakeHandle*>(m);
    return ORB_OK;
}
int orb_search_by_bow(orb_matcher_t m, const orb_kf_view_t* kfs, const uint8_t* const* point_ok, int n_kfs,
                      const orb_kf_view_t* frame, int32_t* matches, int32_t* n_matches) {
    ++g_calls;
    if (g_rc) {
        g_err = "fake failure";
        return g_rc;
    }
    g_seen.h = reinterpret_cast<FakeHandle*>(m);
    g_seen.n_kfs = n_kfs;
    g_seen.kf.take(&kfs[0]);
    g_seen.frame.take(frame);
    g_seen.usable.assign(point_ok[0], point_ok[0] + kfs[0].n);
    std::memcpy(matches, g_match.data(), sizeof(int32_t) * frame->n);
    n_matches[0] = g_count;
    return ORB_OK;
}
}

static orb_keypoint_t kp(float x, float angle) {
    orb_keypoint_t k{};
    k.x = x;
    k.y = 2 * x;
    k.size = 31.f;
    k.angle = angle;
    k.class_id = -1;
    return k;
}

int main() {
    MockMP mp[4];
    mp[2].bad = true;
    MockKF kf;
    for (int i = 0; i < 5; ++i) kf.kps.push_back(kp(10.f + i, 30.f * i));
    kf.desc.assign(5 * 32, 0x5A);
    kf.mps = {&mp[0], nullptr, &mp[2], &mp[3], &mp[1]};
    kf.fv[40] = {3, 0};  // insertion order inside a node is kept
    kf.fv[12] = {4, 1, 2};
    MockFrame F;
    for (int i = 0; i < 4; ++i) F.kps.push_back(kp(100.f + i, 10.f * i));
    F.desc.assign(4 * 32, 0xA5);
    F.fv[12] = {2, 0};
    F.fv[77] = {1, 3};

    Matcher matcher(0.7f, true);
    CHECK(Matcher::Supports(&kf, F));

    // 1. views across the ABI, NULL fill and write-back
    MockMP stale;
    std::vector<MockMP*> out(9, &stale);  // whatever it held is replaced by F.N entries
    g_match = {4, -1, 0, -1};
    g_count = 2;
    int n = matcher.SearchByBoW(&kf, F, out);
    CHECK(n == 2 && g_calls == 1 && g_seen.n_kfs == 1);
    CHECK(g_seen.h && g_seen.h->nnratio == 0.7f && g_seen.h->check_ori == 1);
    CHECK(g_seen.kf.n == 5 && g_seen.kf.kps == kf.kps.data() && g_seen.kf.desc == kf.desc.data());
    CHECK((g_seen.kf.nodes == std::vector<uint32_t>{12, 40}));
    CHECK((g_seen.kf.offset == std::vector<int32_t>{0, 3, 5}));
    CHECK((g_seen.kf.index == std::vector<int32_t>{4, 1, 2, 3, 0}));
    CHECK((g_seen.usable == std::vector<uint8_t>{1, 0, 0, 1, 1}));  // NULL and isBad() are not usable
    CHECK(g_seen.frame.n == 4 && g_seen.frame.kps == F.kps.data() && g_seen.frame.desc == F.desc.data());
    CHECK((g_seen.frame.nodes == std::vector<uint32_t>{12, 77}));
    CHECK((g_seen.frame.offset == std::vector<int32_t>{0, 2, 4}));
    CHECK((g_seen.frame.index == std::vector<int32_t>{2, 0, 1, 3}));
    CHECK(out.size() == 4);
    CHECK(out[0] == &mp[1] && out[1] == nullptr && out[2] == &mp[0] && out[3] == nullptr);

    // 2. no match at all: F.N NULL entries
    g_match = {-1, -1, -1, -1};
    g_count = 0;
    out.assign(2, &stale);
    n = matcher.SearchByBoW(&kf, F, out);
    CHECK(n == 0 && out.size() == 4);
    for (auto* p : out) CHECK(p == nullptr);

    // 3. library errors: 0, every entry NULL, the code reported; the next call works again
    for (int rc : {ORB_ERR_ARG, ORB_ERR_DEVICE, ORB_ERR_INTERNAL}) {
        g_rc = rc;
        g_match = {4, 3, 0, 0};
        g_count = 4;
        out.assign(7, &stale);
        n = matcher.SearchByBoW(&kf, F, out);
        CHECK(n == 0 && out.size() == 4);
        for (auto* p : out) CHECK(p == nullptr);
        CHECK(orbgpu::LastShimError() == rc);
        CHECK(orbgpu::LastShimMessage().find("orb_search_by_bow") != std::string::npos);
    }
    g_rc = 0;
    orbgpu::ClearShimError();
    n = matcher.SearchByBoW(&kf, F, out);
    CHECK(n == 4 && out[0] == &mp[1] && out[1] == &mp[3] && out[2] == &mp[0] && out[3] == &mp[0]);
    CHECK(orbgpu::LastShimError() == ORB_OK);

    // 4. an empty frame: no entries, the library still sees both views
    MockFrame empty;
    g_count = 0;
    n = matcher.SearchByBoW(&kf, empty, out);
    CHECK(n == 0 && out.empty() && g_seen.frame.n == 0 && g_seen.frame.n_nodes == 0);

    // 5. two-camera rigs are not covered
    MockKF fisheye = kf;
    fisheye.cam2 = true;
    MockFrame two = F;
    two.nleft = 2;
    CHECK(!Matcher::Supports(&fisheye, F) && !Matcher::Supports(&kf, two));

    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK bow_shim_check\n");
    return 0;
}
