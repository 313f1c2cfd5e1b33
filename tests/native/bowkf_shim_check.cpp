// CPU check of the loop-closing BoW shims: ORBmatcher<A>::SearchByBoW(KeyFrame*, KeyFrame*, ...) and its batched
// form (include/orbgpu_matcher.hpp; reference src/ORBmatcher.cc:893-1044, src/LoopClosing.cc:840-851) and
// orbgpu::LoopBowProblems (include/orbgpu_sim3.hpp; :855-881 + src/Sim3Solver.cc:71-118) on a mock KeyFrame /
// MapPoint graph.  orb_search_by_bow_kf and orb_loop_bow_problems are plain sequential test doubles, so this runs
// without a GPU; the kernels are compared with the restatement in tests/test_bow_kf_gpu.py.  Checked:
//   * the views and the ok masks as the double receives them (NULL and bad map points masked on both sides);
//   * vpMatches12 sized by pKF1's map points and written from matches12, the return value;
//   * the batched form: NULL and bad window keyframes skipped, one library call;
//   * LoopBowProblems: one pool id per MapPoint across keyframes, pair_ok, group, the poses, obs_ok from
//     GetIndexInKeyFrame, vpMatchedPoints / vpKeyFrameMatchedMP / numBoWMatches and the solver's correspondences;
//   * an ORB_ERR_* injected into each new entry: nothing matched, no solver, the code in LastShimError().
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "orbgpu_matcher.hpp"
#include "orbgpu_sim3.hpp"
#include "bowkf_mock.h"

int g_random_calls = 0;
static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);          \
            ++g_fail;                                                         \
        }                                                                     \
    } while (0)

using Matcher = orbgpu::ORBmatcher<Access>;
using Solver = orbgpu::Sim3Solver<Access>;

// ---- the C ABI's test doubles ------------------------------------------------------------------------------
static int g_rc_search = 0, g_rc_loop = 0, g_rc_ransac = 0, g_search_calls = 0, g_loop_calls = 0, g_last_pairs = 0;
static std::string g_err = "injected";
static std::vector<uint8_t> g_ok1;
static std::vector<std::vector<uint8_t>> g_ok2;
static orb_loop_bow_in_t g_in;
static std::vector<orb_loop_bow_kf_t> g_kf2s;
static std::vector<std::vector<int32_t>> g_mp_id2;
static std::vector<int32_t> g_mp_id1, g_group;
static std::vector<uint8_t> g_pair_ok, g_obs1, g_bad;
static std::vector<float> g_xyz;

static int dist(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount(a[i] ^ b[i]);
    return d;
}

extern "C" {
const char* orb_last_error(void) { return g_err.c_str(); }
int orb_matcher_create(float nnratio, int, orb_matcher_t* out) {
    *out = reinterpret_cast<orb_matcher_t>(new float(nnratio));
    return ORB_OK;
}
int orb_matcher_destroy(orb_matcher_t m) {
    delete reinterpret_cast<float*>(m);
    return ORB_OK;
}
// the reference's walk, sequential, without the orientation check
int orb_search_by_bow_kf(orb_matcher_t m, const orb_kf_view_t* kf1, const uint8_t* ok1, const orb_kf_view_t* kf2s,
                         const uint8_t* const* ok2s, int n_pairs, int32_t* matches12, int32_t* n_matches) {
    ++g_search_calls;
    g_last_pairs = n_pairs;
    if (g_rc_search != 0) return g_rc_search;
    const float nnratio = *reinterpret_cast<float*>(m);
    g_ok1.assign(ok1, ok1 + kf1->n);
    g_ok2.clear();
    for (int p = 0; p < n_pairs; ++p) {
        const orb_kf_view_t& k2 = kf2s[p];
        g_ok2.emplace_back(ok2s[p], ok2s[p] + k2.n);
        std::vector<char> claimed(k2.n, 0);
        int32_t* row = matches12 + (size_t)p * kf1->n;
        for (int i = 0; i < kf1->n; ++i) row[i] = -1;
        n_matches[p] = 0;
        for (int a = 0; a < kf1->n_nodes; ++a)
            for (int b = 0; b < k2.n_nodes; ++b) {
                if (kf1->fv_node[a] != k2.fv_node[b]) continue;
                for (int x = kf1->fv_offset[a]; x < kf1->fv_offset[a + 1]; ++x) {
                    const int i1 = kf1->fv_index[x];
                    if (!ok1[i1]) continue;
                    int best1 = 256, best2 = 256, bi = -1;
                    for (int y = k2.fv_offset[b]; y < k2.fv_offset[b + 1]; ++y) {
                        const int i2 = k2.fv_index[y];
                        if (claimed[i2] || !ok2s[p][i2]) continue;
                        const int d = dist(kf1->desc + 32 * i1, k2.desc + 32 * i2);
                        if (d < best1) { best2 = best1; best1 = d; bi = i2; }
                        else if (d < best2) best2 = d;
                    }
                    if (best1 < 50 && (float)best1 < nnratio * (float)best2) {
                        row[i1] = bi;
                        claimed[bi] = 1;
                        ++n_matches[p];
                    }
                }
            }
    }
    return ORB_OK;
}
// the merge and the gather, sequential
int orb_loop_bow_problems(orb_matcher_t, const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out) {
    ++g_loop_calls;
    if (g_rc_loop != 0) return g_rc_loop;
    g_in = *in;
    g_kf2s.assign(in->kf2s, in->kf2s + in->n_pairs);
    g_group.assign(in->group, in->group + in->n_cand + 1);
    g_pair_ok.assign(in->pair_ok, in->pair_ok + in->n_pairs);
    g_mp_id1.assign(in->kf1.mp_id, in->kf1.mp_id + in->kf1.n);
    g_obs1.assign(in->kf1.obs_ok, in->kf1.obs_ok + in->kf1.n);
    g_xyz.assign(in->xyz, in->xyz + 3 * (size_t)in->n_points);
    g_bad.assign(in->bad, in->bad + in->n_points);
    g_mp_id2.clear();
    for (int p = 0; p < in->n_pairs; ++p)
        g_mp_id2.emplace_back(in->kf2s[p].mp_id, in->kf2s[p].mp_id + (in->kf2s[p].mp_id ? in->kf2s[p].n : 0));
    const int C = in->stride;
    for (int c = 0; c < in->n_cand; ++c) {
        std::set<int> seen;
        int32_t *mpt = out->matched_point + (size_t)c * C, *mpr = out->matched_pair + (size_t)c * C;
        for (int k = 0; k < C; ++k) mpt[k] = mpr[k] = -1;
        out->num_bow[c] = 0;
        for (int p = in->group[c]; p < in->group[c + 1]; ++p) {
            if (!in->pair_ok[p]) continue;
            for (int k = 0; k < in->kf1.n; ++k) {
                const int i2 = in->matches12[(size_t)p * C + k];
                if (i2 < 0) continue;
                const int id = in->kf2s[p].mp_id[i2];
                if (id < 0 || in->bad[id] || seen.count(id)) continue;
                seen.insert(id);
                ++out->num_bow[c];
                mpt[k] = id;
                mpr[k] = p - in->group[c];
            }
        }
        int n = 0;
        for (int k = 0; k < in->kf1.n; ++k) {
            if (mpt[k] < 0 || !in->ok1[k] || !in->kf1.obs_ok[k]) continue;
            const int p = in->group[c] + mpr[k], i2 = in->matches12[(size_t)p * C + k];
            const orb_loop_bow_kf_t& F = in->kf2s[p];
            if (!F.obs_ok[i2]) continue;
            const size_t at = (size_t)c * C + n;
            out->idx1[at] = k;
            out->max_err1[at] = (float)(9.210 * in->kf1.level_sigma2[in->kf1.kps[k].octave]);
            out->max_err2[at] = (float)(9.210 * F.level_sigma2[F.kps[i2].octave]);
            const float *X1 = in->xyz + 3 * in->kf1.mp_id[k], *X2 = in->xyz + 3 * mpt[k], *T2 = in->Tcw2 + 12 * c;
            for (int r = 0; r < 3; ++r) {
                out->x3dc1[3 * at + r] = in->Tcw1[4 * r] * X1[0] + in->Tcw1[4 * r + 1] * X1[1] + in->Tcw1[4 * r + 2] * X1[2] + in->Tcw1[4 * r + 3];
                out->x3dc2[3 * at + r] = T2[4 * r] * X2[0] + T2[4 * r + 1] * X2[1] + T2[4 * r + 2] * X2[2] + T2[4 * r + 3];
            }
            ++n;
        }
        out->n[c] = n;
    }
    return ORB_OK;
}
int orb_sim3_ransac(const orb_sim3_problem_t*, int, const orb_sim3_out_t*) { return g_rc_ransac; }
}  // extern "C"

// descriptor codes at least 128 bits apart from each other
static const uint8_t kCode[10] = {0x00, 0xFF, 0x0F, 0xF0, 0x33, 0xCC, 0x55, 0xAA, 0x3C, 0xC3};

int main() {
    // the map: ten points; point 6 is bad
    std::vector<MockMP> mp(10);
    for (int i = 0; i < 10; ++i) {
        mp[i].pos[0] = 0.1f * i;
        mp[i].pos[1] = -0.2f * i;
        mp[i].pos[2] = 3.f + i;
    }
    mp[6].bad = true;
    // the current keyframe: features 0..5 with codes 0..5; feature 3 without a map point, feature 4's point is bad
    MockKF cur;
    cur.add(1, kCode[0], &mp[0], 0);
    cur.add(1, kCode[1], &mp[1], 1);
    cur.add(2, kCode[2], &mp[2], 2);
    cur.add(2, kCode[3], nullptr);
    cur.add(2, kCode[4], &mp[6]);
    cur.add(3, kCode[5], &mp[3], 3, 0.f, false);  // the point does not list the keyframe
    cur.t[0] = 0.5f;
    // window keyframes: w0 sees codes 0, 1, 2 (points 7, 8, 9), w1 sees 1, 2 (points 8 again, 5 new at the same k = 2)
    // and code 5 (point 4); w2 is bad; a NULL entry; w3 has a feature without a map point under code 0
    MockKF w0, w1, w2, w3;
    w0.add(1, kCode[1], &mp[8], 2);
    w0.add(1, kCode[0], &mp[7], 1);
    w0.add(2, kCode[2], &mp[9], 0);
    w0.add(2, kCode[4], &mp[5]);  // KF1's feature 4 is masked: never matched
    w1.add(1, kCode[1], &mp[8], 1);
    w1.add(2, kCode[2], &mp[5], 4);
    w1.add(3, kCode[5], &mp[4], 2);
    w2.add(1, kCode[0], &mp[7]);
    w2.bad = true;
    w3.add(1, kCode[0], nullptr);
    w3.add(1, kCode[1], &mp[6]);  // a bad point: masked
    MockKF cand0, cand1;
    cand0.t[2] = 1.f;
    cand1.t[1] = -2.f;
    cand1.K[0] = 400.f;

    Matcher matcher(0.7f, false);
    // ---- the single form
    std::vector<MockMP*> v12(3, &mp[0]);
    int n = matcher.SearchByBoW(&cur, &w0, v12);
    CHECK(n == 3 && g_search_calls == 1 && orbgpu::LastShimError() == ORB_OK);
    CHECK(v12.size() == 6 && v12[0] == &mp[7] && v12[1] == &mp[8] && v12[2] == &mp[9] && !v12[3] && !v12[4] && !v12[5]);
    CHECK((g_ok1 == std::vector<uint8_t>{1, 1, 1, 0, 0, 1}));
    CHECK(g_ok2.size() == 1 && (g_ok2[0] == std::vector<uint8_t>{1, 1, 1, 1}));
    n = matcher.SearchByBoW(&cur, &w3, v12);
    CHECK(n == 0 && (g_ok2[0] == std::vector<uint8_t>{0, 0}) && v12.size() == 6 && !v12[0] && !v12[1]);
    // ---- the batched form: one call, NULL and bad keyframes skipped
    std::vector<MockKF*> window{&w0, nullptr, &w1, &w2, &w3};
    std::vector<std::vector<MockMP*>> vv;
    std::vector<int> cnt;
    g_search_calls = 0;
    CHECK(matcher.SearchByBoW(&cur, window, vv, cnt));
    CHECK(g_search_calls == 1 && g_last_pairs == 3 && vv.size() == 5 && (cnt == std::vector<int>{3, 0, 3, 0, 0}));
    CHECK(vv[1].empty() && vv[3].empty() && vv[0].size() == 6 && vv[0][1] == &mp[8]);
    CHECK(vv[2][1] == &mp[8] && vv[2][2] == &mp[5] && vv[2][5] == &mp[4] && !vv[2][0]);
    // ---- the merge and the gather: candidate 0 has the window above, candidate 1 only w1
    std::vector<orbgpu::LoopBowCandidate<Access>> out;
    g_search_calls = 0;
    CHECK((orbgpu::LoopBowProblems<Access>(matcher, &cur, {&cand0, &cand1}, {window, {&w1}}, true, out)));
    CHECK(g_search_calls == 1 && g_loop_calls == 1 && g_last_pairs == 4 && out.size() == 2);
    CHECK((g_group == std::vector<int32_t>{0, 5, 6}) && (g_pair_ok == std::vector<uint8_t>{1, 0, 1, 0, 1, 1}));
    CHECK(g_in.n_pairs == 6 && g_in.n_cand == 2 && g_in.stride == 6 && g_in.kf1.n == 6);
    CHECK(g_in.Tcw1[3] == 0.5f && g_in.Tcw2[11] == 1.f && g_in.Tcw2[12 + 7] == -2.f && g_in.Tcw1[0] == 1.f);
    // one id per MapPoint, whichever keyframe lists it: point 8 in w0 and w1 (twice: both candidates), point 5
    CHECK(g_mp_id2[0][0] == g_mp_id2[2][0] && g_mp_id2[2][0] == g_mp_id2[5][0] && g_mp_id2[0][3] == g_mp_id2[2][1]);
    CHECK(g_mp_id1[3] == -1 && g_mp_id1[0] >= 0 && g_mp_id1[0] != g_mp_id1[1] && g_mp_id2[4][0] == -1);
    CHECK(g_mp_id2[1].empty() && g_mp_id2[3].empty());
    CHECK((g_obs1 == std::vector<uint8_t>{1, 1, 1, 0, 1, 0}));
    CHECK(g_in.n_points == 10 && g_xyz[3 * g_mp_id1[1] + 2] == 4.f && g_bad[g_mp_id1[4]] == 1);
    CHECK(g_kf2s[0].nlevels == 3 && g_kf2s[2].nlevels == 5 && g_kf2s[2].level_sigma2[4] == w1.sigma2[4]);
    const orbgpu::LoopBowCandidate<Access>& c0 = out[0];
    // points 7, 8, 9 through w0; 8 again, then 5 (overwrites k = 2) and 4 through w1
    CHECK(c0.numBoWMatches == 5 && (c0.vnMatches == std::vector<int>{3, 0, 3, 0, 0}));
    CHECK(c0.vpMatchedPoints.size() == 6 && c0.vpMatchedPoints[0] == &mp[7] && c0.vpMatchedPoints[1] == &mp[8] &&
          c0.vpMatchedPoints[2] == &mp[5] && c0.vpMatchedPoints[5] == &mp[4] && !c0.vpMatchedPoints[3]);
    CHECK(c0.vpKeyFrameMatchedMP[0] == &w0 && c0.vpKeyFrameMatchedMP[2] == &w1 && c0.vpKeyFrameMatchedMP[5] == &w1 &&
          !c0.vpKeyFrameMatchedMP[4]);
    // the solver: k = 5 is dropped (the point does not list the current keyframe)
    CHECK(c0.solver && c0.solver->Correspondences() == 3 && (c0.solver->Indices1() == std::vector<int>{0, 1, 2}));
    CHECK(c0.solver->MaxError1()[1] == (float)(9.210 * cur.sigma2[1]) && c0.solver->MaxError2()[2] == (float)(9.210 * w1.sigma2[4]));
    CHECK(c0.solver->X3Dc1()[0] == mp[0].pos[0] + 0.5f && c0.solver->X3Dc2()[2] == mp[7].pos[2] + 1.f);
    CHECK(out[1].numBoWMatches == 3 && out[1].solver && out[1].solver->Correspondences() == 2 &&
          out[1].vpMatchedPoints[1] == &mp[8] && out[1].vpKeyFrameMatchedMP[1] == &w1);
    // the solver is usable: too few correspondences for the default minimum -> bNoMore, no library call needed
    bool no_more = false;
    std::vector<bool> inl;
    int n_inl = 0;
    c0.solver->iterate(5, no_more, inl, n_inl);
    CHECK(no_more && n_inl == 0 && inl.size() == 6);
    // ---- injected failures
    for (int code : {ORB_ERR_ARG, ORB_ERR_DEVICE, ORB_ERR_CAPACITY}) {
        orbgpu::ClearShimError();
        g_rc_search = code;
        v12.assign(2, &mp[0]);
        CHECK(matcher.SearchByBoW(&cur, &w0, v12) == 0 && orbgpu::LastShimError() == code);
        CHECK(v12.size() == 6 && !v12[0] && !v12[1] && !v12[2]);
        orbgpu::ClearShimError();
        CHECK(!matcher.SearchByBoW(&cur, window, vv, cnt) && orbgpu::LastShimError() == code);
        CHECK((cnt == std::vector<int>{0, 0, 0, 0, 0}) && vv[0].size() == 6 && !vv[0][0] && vv[1].empty());
        orbgpu::ClearShimError();
        CHECK(!(orbgpu::LoopBowProblems<Access>(matcher, &cur, {&cand0}, {window}, true, out)) && orbgpu::LastShimError() == code);
        CHECK(out.size() == 1 && out[0].numBoWMatches == 0 && !out[0].solver && out[0].vpMatchedPoints.size() == 6 &&
              !out[0].vpMatchedPoints[0]);
        g_rc_search = 0;
        g_rc_loop = code;
        orbgpu::ClearShimError();
        CHECK(!(orbgpu::LoopBowProblems<Access>(matcher, &cur, {&cand0}, {window}, true, out)) && orbgpu::LastShimError() == code);
        CHECK(out[0].numBoWMatches == 0 && !out[0].solver && !out[0].vpMatchedPoints[1] && !out[0].vpKeyFrameMatchedMP[1]);
        g_rc_loop = 0;
    }
    orbgpu::ClearShimError();
    CHECK((orbgpu::LoopBowProblems<Access>(matcher, &cur, {}, {}, true, out)) && out.empty());
    if (g_fail) return 1;
    std::printf("OK bowkf_shim_check\n");
    return 0;
}
