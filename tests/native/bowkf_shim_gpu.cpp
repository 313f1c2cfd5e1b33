// The loop-closing BoW shims (ORBmatcher<A>::SearchByBoW(KeyFrame*, KeyFrame*, ...), its batched form and
// orbgpu::LoopBowProblems) against the real liborbgpu.so on the GPU.  The mock graph is built from a scene file
// written by tests/test_bowkf_shim_gpu.py, whose expected values come from the restatement tests/bow_kf_ref.py:
//   int32 magic, n_kf (1 + P), n_cand, n_points, n1;  int32 group[n_cand + 1];  float Tcw[(1 + n_cand) x 12] (the
//   current keyframe's, then the candidates');  float xyz[n_points x 3];  uint8 bad[n_points];
//   per keyframe (the current one first): int32 n, n_nodes;  keypoints n x 28;  descriptors n x 32;
//     int32 mp_id[n];  uint8 observed[n];  per node: int32 id, count, indices[count];
//   expected: int32 rows[P x n1], counts[P];  per candidate: int32 num_bow, n, matched_point[n1], matched_pair[n1],
//     idx1[n];  float max_err1[n], max_err2[n], x3dc1[3n], x3dc2[3n];  double bound1[3n], bound2[3n]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
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

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::printf("FAIL short scene file\n");
        std::exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int32_t>(f, 5);
    if (hd[0] != 0x426b6631) return 2;
    const int n_kf = hd[1], n_cand = hd[2], n_points = hd[3], n1 = hd[4], P = n_kf - 1;
    const auto group = rd<int32_t>(f, n_cand + 1);
    const auto Tcw = rd<float>(f, (size_t)(1 + n_cand) * 12);
    const auto xyz = rd<float>(f, (size_t)n_points * 3);
    const auto bad = rd<uint8_t>(f, n_points);
    std::vector<MockMP> pool(n_points);
    for (int i = 0; i < n_points; ++i) {
        std::memcpy(pool[i].pos, &xyz[3 * i], 12);
        pool[i].bad = bad[i] != 0;
    }
    auto set_pose = [&](MockKF& k, int at) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) k.R[3 * r + c] = Tcw[12 * at + 4 * r + c];
            k.t[r] = Tcw[12 * at + 4 * r + 3];
        }
    };
    std::vector<std::unique_ptr<MockKF>> kfs;
    for (int k = 0; k < n_kf; ++k) {
        kfs.emplace_back(new MockKF);
        MockKF& K = *kfs.back();
        const auto nn = rd<int32_t>(f, 2);
        K.kps = rd<orb_keypoint_t>(f, nn[0]);
        K.desc = rd<uint8_t>(f, (size_t)nn[0] * 32);
        const auto mp_id = rd<int32_t>(f, nn[0]);
        const auto observed = rd<uint8_t>(f, nn[0]);
        for (int i = 0; i < nn[0]; ++i) {
            K.mps.push_back(mp_id[i] >= 0 ? &pool[mp_id[i]] : nullptr);
            if (mp_id[i] >= 0 && observed[i]) pool[mp_id[i]].obs[&K] = i;
        }
        for (int j = 0; j < nn[1]; ++j) {
            const auto nc = rd<int32_t>(f, 2);
            for (int32_t i : rd<int32_t>(f, nc[1])) K.fv[(unsigned)nc[0]].push_back((unsigned)i);
        }
    }
    set_pose(*kfs[0], 0);
    std::vector<std::unique_ptr<MockKF>> cands;
    for (int c = 0; c < n_cand; ++c) {
        cands.emplace_back(new MockKF);
        set_pose(*cands.back(), 1 + c);
    }
    const auto rows = rd<int32_t>(f, (size_t)P * n1);
    const auto counts = rd<int32_t>(f, P);

    MockKF* cur = kfs[0].get();
    CHECK((int)cur->kps.size() == n1);
    orbgpu::ORBmatcher<Access> matcher(0.7f, true);
    // ---- the single form and the batched form against the restatement's rows
    std::vector<MockKF*> window;
    for (int p = 0; p < P; ++p) window.push_back(kfs[1 + p].get());
    std::vector<std::vector<MockMP*>> vv;
    std::vector<int> cnt;
    CHECK(matcher.SearchByBoW(cur, window, vv, cnt) && orbgpu::LastShimError() == ORB_OK);
    int total = 0;
    for (int p = 0; p < P; ++p) {
        std::vector<MockMP*> v12;
        const int n = matcher.SearchByBoW(cur, window[p], v12);
        CHECK(n == counts[p] && cnt[p] == counts[p] && (int)v12.size() == n1 && v12 == vv[p]);
        int wrong = 0;
        for (int i = 0; i < n1; ++i) {
            const int32_t j = rows[(size_t)p * n1 + i];
            wrong += v12[i] != (j >= 0 ? window[p]->mps[j] : nullptr);
        }
        CHECK(wrong == 0);
        total += n;
    }
    CHECK(total > 40);
    // ---- a bad window keyframe and a NULL entry are skipped; the rest is unchanged
    {
        std::vector<MockKF*> w2 = window;
        w2.insert(w2.begin() + 1, nullptr);
        w2[2]->bad = true;
        std::vector<std::vector<MockMP*>> v2;
        std::vector<int> c2;
        CHECK(matcher.SearchByBoW(cur, w2, v2, c2));
        CHECK(v2[1].empty() && v2[2].empty() && c2[1] == 0 && c2[2] == 0 && v2[0] == vv[0] && v2[3] == vv[2]);
        w2[2]->bad = false;
    }
    // ---- the merge, the gather and the solver
    std::vector<MockKF*> vc;
    std::vector<std::vector<MockKF*>> cov(n_cand);
    for (int c = 0; c < n_cand; ++c) {
        vc.push_back(cands[c].get());
        for (int p = group[c]; p < group[c + 1]; ++p) cov[c].push_back(window[p]);
    }
    std::vector<orbgpu::LoopBowCandidate<Access>> out;
    CHECK((orbgpu::LoopBowProblems<Access>(matcher, cur, vc, cov, false, out)) && orbgpu::LastShimError() == ORB_OK);
    CHECK((int)out.size() == n_cand);
    std::vector<orbgpu::Sim3Solver<Access>*> solvers;
    for (int c = 0; c < n_cand && c < (int)out.size(); ++c) {
        const auto hn = rd<int32_t>(f, 2);
        const auto mpt = rd<int32_t>(f, n1), mpr = rd<int32_t>(f, n1), idx1 = rd<int32_t>(f, hn[1]);
        const auto e1 = rd<float>(f, hn[1]), e2 = rd<float>(f, hn[1]), x1 = rd<float>(f, 3 * (size_t)hn[1]),
                   x2 = rd<float>(f, 3 * (size_t)hn[1]);
        const auto b1 = rd<double>(f, 3 * (size_t)hn[1]), b2 = rd<double>(f, 3 * (size_t)hn[1]);
        const orbgpu::LoopBowCandidate<Access>& o = out[c];
        CHECK(o.numBoWMatches == hn[0] && o.solver && (int)o.vpMatchedPoints.size() == n1);
        if (!o.solver) continue;
        int wrong = 0;
        for (int k = 0; k < n1; ++k) {
            wrong += o.vpMatchedPoints[k] != (mpt[k] >= 0 ? &pool[mpt[k]] : nullptr);
            wrong += o.vpKeyFrameMatchedMP[k] != (mpr[k] >= 0 ? cov[c][mpr[k]] : nullptr);
        }
        CHECK(wrong == 0);
        const orbgpu::Sim3Solver<Access>& s = *o.solver;
        CHECK(s.Correspondences() == hn[1] && hn[1] >= 6);
        if (s.Correspondences() != hn[1]) continue;
        for (int i = 0; i < hn[1]; ++i) {
            wrong += s.Indices1()[i] != idx1[i];
            wrong += std::memcmp(&s.MaxError1()[i], &e1[i], 4) != 0 || std::memcmp(&s.MaxError2()[i], &e2[i], 4) != 0;
            for (int r = 0; r < 3; ++r) {
                wrong += !(std::fabs((double)s.X3Dc1()[3 * i + r] - x1[3 * i + r]) <= b1[3 * i + r]);
                wrong += !(std::fabs((double)s.X3Dc2()[3 * i + r] - x2[3 * i + r]) <= b2[3 * i + r]);
            }
        }
        CHECK(wrong == 0);
        solvers.push_back(o.solver.get());
    }
    // the solvers run: one library call for all candidates, then the reference's loop
    for (auto* s : solvers) s->SetRansacParameters(0.99, 6, 40);
    orbgpu::Sim3Solver<Access>::Batch(solvers);
    CHECK(orbgpu::LastShimError() == ORB_OK && g_random_calls > 0);
    for (auto* s : solvers) {
        bool no_more = false, converged = false;
        std::vector<bool> inl;
        int n_inl = 0;
        while (!converged && !no_more) s->iterate(20, no_more, inl, n_inl, converged);
        int set = 0;
        for (bool b : inl) set += b;
        CHECK(converged && n_inl > 6 && set == n_inl && (int)inl.size() == n1);  // the scene is one similarity
    }
    // ---- an argument the library rejects (a feature listed twice): nothing matched, the code reported
    {
        MockKF& w = *window[0];
        const unsigned node = w.fv.begin()->first;
        w.fv[node].push_back(w.fv[node][0]);
        std::vector<MockMP*> v12(3, &pool[0]);
        orbgpu::ClearShimError();
        CHECK(matcher.SearchByBoW(cur, &w, v12) == 0 && orbgpu::LastShimError() == ORB_ERR_ARG);
        int set = 0;
        for (MockMP* p : v12) set += p != nullptr;
        CHECK((int)v12.size() == n1 && set == 0);
        orbgpu::ClearShimError();
        CHECK(!(orbgpu::LoopBowProblems<Access>(matcher, cur, vc, cov, false, out)) && orbgpu::LastShimError() == ORB_ERR_ARG);
        CHECK(!out[0].solver && out[0].numBoWMatches == 0);
        w.fv[node].pop_back();
    }
    std::fclose(f);
    if (g_fail) return 1;
    std::printf("OK bowkf_shim_gpu\n");
    return 0;
}
