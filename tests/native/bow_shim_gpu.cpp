// ORBmatcher::SearchByBoW of include/orbgpu_matcher.hpp against the real liborbgpu.so on the GPU
// (tests/test_bow_shim_gpu.py; links only liborbgpu).  Input: a scene file written by the test -- a keyframe
// and a frame (keypoints, descriptors, FeatureVectors), the keyframe's usable flags, and the matches the
// Python restatement of src/ORBmatcher.cc:260-494 (tests/bow_search_ref.py) expects with and without the
// orientation check.  The program builds mock KeyFrame / Frame / MapPoint objects from it, runs the
// drop-in matcher as Tracking::TrackReferenceKeyFrame does, and checks vpMapPointMatches entry by entry.
//
// File: int32 header {magic 0x426f5753, nK, nF, nodesK, nodesF, idxK, idxF}; keyframe: keypoints (28 B each),
// descriptors (32 B each), usable flags (1 B each), node ids (u32), CSR offsets (nodes + 1), indices;
// frame: keypoints, descriptors, node ids, offsets, indices; expected: match[nF] and count without the
// check, then match[nF] and count with it.
#include <cstdio>
#include <cstring>
#include <map>
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

struct MockMP {
    bool bad = false;
};
using FeatureVector = std::map<unsigned int, std::vector<unsigned int>>;
struct MockKF {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    std::vector<MockMP*> mps;
    FeatureVector fv;
    std::vector<float> scale, sigma2;
};
struct MockFrame {
    std::vector<orb_keypoint_t> kps;
    std::vector<uint8_t> desc;
    FeatureVector fv;
    std::vector<float> scale;
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
    static void Pinhole(KeyFrame*, float K[4]) { K[0] = 458.654f; K[1] = 457.296f; K[2] = 367.215f; K[3] = 248.375f; }
    static int Levels(KeyFrame* k) { return (int)k->scale.size(); }
    static const float* ScaleFactors(KeyFrame* k) { return k->scale.data(); }
    static const float* LevelSigma2(KeyFrame* k) { return k->sigma2.data(); }
    static bool SingleCamera(KeyFrame*) { return true; }
    static orb_frame_view_t View(const Frame& f) {
        orb_frame_view_t v{};
        v.n = (int)f.kps.size();
        v.kps_un = f.kps.data();
        v.desc = f.desc.data();
        v.nlevels = (int)f.scale.size();
        v.scale_factors = f.scale.data();
        return v;
    }
    static bool SingleCamera(const Frame&) { return true; }
    static bool IsBad(MapPoint* p) { return p->bad; }
};
using Matcher = orbgpu::ORBmatcher<Access>;

template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static FeatureVector feature_vector(const std::vector<uint32_t>& node, const std::vector<int32_t>& off,
                                    const std::vector<int32_t>& idx) {
    FeatureVector fv;
    for (size_t i = 0; i < node.size(); ++i) fv[node[i]].assign(idx.begin() + off[i], idx.begin() + off[i + 1]);
    return fv;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: bow_shim_gpu <scene file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[7];
    if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] != 0x426f5753) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    const int nK = hdr[1], nF = hdr[2], nnK = hdr[3], nnF = hdr[4], niK = hdr[5], niF = hdr[6];
    MockKF kf;
    MockFrame F;
    std::vector<uint8_t> usable;
    std::vector<uint32_t> nodeK, nodeF;
    std::vector<int32_t> offK, idxK, offF, idxF, exp[2];
    int32_t exp_n[2] = {0, 0};
    bool ok = read_vec(f, kf.kps, nK) && read_vec(f, kf.desc, (size_t)nK * 32) && read_vec(f, usable, nK) &&
              read_vec(f, nodeK, nnK) && read_vec(f, offK, nnK + 1) && read_vec(f, idxK, niK) && read_vec(f, F.kps, nF) &&
              read_vec(f, F.desc, (size_t)nF * 32) && read_vec(f, nodeF, nnF) && read_vec(f, offF, nnF + 1) &&
              read_vec(f, idxF, niF);
    for (int c = 0; ok && c < 2; ++c) ok = read_vec(f, exp[c], nF) && std::fread(&exp_n[c], 4, 1, f) == 1;
    std::fclose(f);
    if (!ok) {
        std::printf("short scene file\n");
        return 2;
    }
    kf.fv = feature_vector(nodeK, offK, idxK);
    F.fv = feature_vector(nodeF, offF, idxF);
    kf.scale = F.scale = {1.f, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 2.985984f, 3.5831808f};
    for (float s : kf.scale) kf.sigma2.push_back(s * s);
    // the keyframe's map points: usable ones good; the others NULL or bad in turn (both are skipped, :307-313)
    std::vector<std::unique_ptr<MockMP>> store;
    kf.mps.assign(nK, nullptr);
    for (int i = 0; i < nK; ++i) {
        if (!usable[i] && (i & 1)) continue;
        store.emplace_back(new MockMP());
        store.back()->bad = !usable[i];
        kf.mps[i] = store.back().get();
    }

    for (int c = 0; c < 2; ++c) {  // ORBmatcher(0.7, false), then TrackReferenceKeyFrame's ORBmatcher(0.7, true)
        Matcher matcher(0.7f, c == 1);
        MockMP stale;
        std::vector<MockMP*> out(3, &stale);
        orbgpu::ClearShimError();
        const int n = matcher.SearchByBoW(&kf, F, out);
        CHECK(orbgpu::LastShimError() == ORB_OK);
        CHECK(n == exp_n[c]);
        CHECK((int)out.size() == nF);
        int wrong = 0, found = 0;
        for (int i = 0; i < nF && i < (int)out.size(); ++i) {
            MockMP* want = exp[c][i] >= 0 ? kf.mps[exp[c][i]] : nullptr;
            wrong += out[i] != want;
            found += out[i] != nullptr;
        }
        CHECK(wrong == 0);
        CHECK(found == exp_n[c] && found > 0);
        std::printf("check_ori %d: %d matches (expected %d), %d wrong entries\n", c, n, exp_n[c], wrong);
    }
    // an invalid view (the frame lists a feature twice): ORB_ERR_ARG from the library -> 0 and all NULL
    {
        MockFrame bad = F;
        auto& first = bad.fv.begin()->second;
        first.push_back(first.front());
        Matcher matcher(0.7f, true);
        MockMP stale;
        std::vector<MockMP*> out(3, &stale);
        const int n = matcher.SearchByBoW(&kf, bad, out);
        CHECK(n == 0 && (int)out.size() == nF && orbgpu::LastShimError() == ORB_ERR_ARG);
        for (auto* p : out) CHECK(p == nullptr);
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK bow_shim_gpu\n");
    return 0;
}
