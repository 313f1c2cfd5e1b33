// Optimizer::OptimizeSim3 on MI355X (reference src/Optimizer.cc:4195-4494, called per loop / merge candidate
// at src/LoopClosing.cc:689 and :991), batched over candidates, FP64.
//
// One 256-thread workgroup per problem runs the whole two-stage schedule in one launch, as orb_pose.hip does
// for PoseOptimization: optimize(5) with Huber kernels, the first cull on the stored errors, the < 10 exit,
// optimize(10 or 5) without kernels, the second cull.  The pairs live in LDS for the whole run (88 B each:
// P3D1c, P3D2c, obs1, obs2, two informations), with each pair's last chi2 of both edges and its culled flag
// beside them; room for kRoom = ORB_OPTSIM3_MAX_PAIRS = 1024 pairs (105 KB of the CU's 160 KB).  A larger
// problem is rejected at the entry (ORB_ERR_ARG): the reference's callers pass the matches of one keyframe.
//
// Per LM iteration (arithmetic in orb_optsim3_math.h, shared with the host build of the tests):
//   perturb    lanes 0..13 build the 14 estimates Sim3(+-1e-9 e_d) * S of g2o's central differences and their
//              inverses, lane 14 the estimate's own inverse: once per linearisation, in LDS, reused by every edge
//   linearise  thread t takes pairs t, t + 256, ...: the errors at S (kept: chi2 of both edges), 2 x 14 error
//              evaluations, the Huber weights, and the pair's share of the 28 + 7 entries of J^T W J, -J^T W e
//              and of the robust chi2; 36 sums reduced in a fixed order (xor butterfly in each wave, then the
//              four waves in order), so two runs give the same bits
//   trial      thread 0 factors H + lambda I (LDL^T), applies exp(dx) * S and publishes the trial estimate;
//              all threads evaluate the errors there (kept, even when the trial is rejected: g2o classifies on
//              the last evaluated state); thread 0 runs the accept / reject rule
// No MFMA: one 7x7 system per problem; the work is the per-edge evaluations and the reductions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_optsim3_math.h"
#include "orbgpu.h"
#include "orbgpu_internal.h"

namespace {

using orbgpu::kOptSim3Acc;
using orbgpu::OptSim3Pair;
using orbgpu::Sim3d;

constexpr int kOsThreads = 256;
constexpr int kOsWaves = kOsThreads / 64;
constexpr int kOsRoom = ORB_OPTSIM3_MAX_PAIRS;
constexpr int kOsPerLaunch = 16;

struct OsProb {
    int n, fix_scale;
    float cam1[4], cam2[4];
    float th2;
    double s12[8];
    const double *p1c, *p2c, *obs1, *obs2;
    const float *is1, *is2;
    double* s12_out;
    int32_t *n_in, *n_bad;
    uint8_t* inlier;
    double *chi2_12, *chi2_21;
};
struct OsLaunch {
    OsProb p[kOsPerLaunch];
};
static_assert(sizeof(OsLaunch) <= 4096, "the problem records travel as kernel arguments");

__device__ __forceinline__ double os_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kOsThreads) void k_optsim3(const OsLaunch L) {
    // the pairs, field by field: 88 B per pair
    __shared__ double lp1[3][kOsRoom], lp2[3][kOsRoom], lo1[2][kOsRoom], lo2[2][kOsRoom];
    __shared__ float li1[kOsRoom], li2[kOsRoom];
    // each pair's stored chi2 of e12 / e21 (the last evaluated state's) and its culled flag
    __shared__ double lc12[kOsRoom], lc21[kOsRoom];
    __shared__ uint8_t lbad[kOsRoom];
    __shared__ Sim3d sP[15], sPi[15];  // 0..13 the perturbed estimates, 14 the state under evaluation; inverses
    __shared__ Sim3d sCur;             // the vertex's estimate
    __shared__ double part[kOsWaves][kOptSim3Acc], tot[kOptSim3Acc], sys[kOptSim3Acc];
    __shared__ int s_cmd;

    const OsProb& P = L.p[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n;
    const bool fix = P.fix_scale != 0;
    const int nd = fix ? 6 : 7;
    const orbgpu::OptSim3Huber hub = orbgpu::optsim3_huber(P.th2);
    const double th2 = (double)P.th2;

    if (tid < 8) P.s12_out[tid] = P.s12[tid];
    if (n == 0) {  // no edge: both optimize() calls return at once, nCorrespondences - nBad = 0 < 10
        if (tid == 0) {
            *P.n_in = 0;
            *P.n_bad = 0;
        }
        return;
    }
    for (int i = tid; i < n; i += kOsThreads) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lp1[k][i] = P.p1c[3 * (size_t)i + k];
            lp2[k][i] = P.p2c[3 * (size_t)i + k];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            lo1[k][i] = P.obs1[2 * (size_t)i + k];
            lo2[k][i] = P.obs2[2 * (size_t)i + k];
        }
        li1[i] = P.is1[i];
        li2[i] = P.is2[i];
        lc12[i] = lc21[i] = 0.0;
        lbad[i] = 0;
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sCur.q[k] = P.s12[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) sCur.t[k] = P.s12[4 + k];
        sCur.s = P.s12[7];
    }
    __syncthreads();

    auto pair_at = [&](int i) {
        OptSim3Pair p;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.p1[k] = lp1[k][i];
            p.p2[k] = lp2[k][i];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            p.o1[k] = lo1[k][i];
            p.o2[k] = lo2[k][i];
        }
        p.is1 = li1[i];
        p.is2 = li2[i];
        return p;
    };
    // v summed over the workgroup into tot[0], in a fixed order
    auto reduce1 = [&](double v) {
        const double s = os_wave_sum(v);
        if (lane == 0) part[wave][0] = s;
        __syncthreads();
        if (tid == 0) tot[0] = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
        __syncthreads();
    };
    // computeActiveErrors + buildSystem at sCur
    auto linearise = [&](bool robust) {
        if (tid < 14) {
            const Sim3d S = orbgpu::optsim3_perturbed(sCur, tid, fix);
            sP[tid] = S;
            sPi[tid] = orbgpu::sim3_inverse(S);
        } else if (tid == 14) {
            const Sim3d S = sCur;
            sP[14] = S;
            sPi[14] = orbgpu::sim3_inverse(S);
        }
        __syncthreads();
        double acc[kOptSim3Acc];
#pragma unroll
        for (int k = 0; k < kOptSim3Acc; ++k) acc[k] = 0.0;
        for (int i = tid; i < n; i += kOsThreads) {
            if (lbad[i]) continue;
            const OptSim3Pair p = pair_at(i);
            double c12, c21;
            orbgpu::optsim3_linearize_pair(sP, sPi, p, P.cam1, P.cam2, hub, robust, nd, acc, c12, c21);
            lc12[i] = c12;
            lc21[i] = c21;
        }
#pragma unroll
        for (int k = 0; k < kOptSim3Acc; ++k) {
            const double s = os_wave_sum(acc[k]);
            if (lane == 0) part[wave][k] = s;
        }
        __syncthreads();
        if (tid < kOptSim3Acc) tot[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        __syncthreads();
    };
    // computeActiveErrors at sP[14] (inverse sPi[14]); tot[0]: the robust chi2
    auto errors = [&](bool robust) {
        double sum = 0.0;
        for (int i = tid; i < n; i += kOsThreads) {
            if (lbad[i]) continue;
            const OptSim3Pair p = pair_at(i);
            double c12, c21;
            sum += orbgpu::optsim3_error_pair(sP[14], sPi[14], p, P.cam1, P.cam2, hub, robust, c12, c21);
            lc12[i] = c12;
            lc21[i] = c21;
        }
        reduce1(sum);
    };
    // SparseOptimizer::optimize(iters) over the pairs not culled (at least one)
    orbgpu::OptSim3Lm lm;   // thread 0's
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    bool ok = false;
    auto optimize = [&](int iters, bool robust) {
        if (tid == 0) orbgpu::optsim3_lm_begin(lm, iters);
        for (;;) {
            linearise(robust);
            if (tid == 0) {
                for (int k = 0; k < kOptSim3Acc; ++k) sys[k] = tot[k];
                orbgpu::optsim3_lm_iteration(lm, sys);
            }
            int cmd;
            for (;;) {
                if (tid == 0) {
                    ok = orbgpu::optsim3_solve7(sys, lm.lambda, x);
                    const Sim3d T = orbgpu::optsim3_oplus(sCur, x, fix);
                    sP[14] = T;
                    sPi[14] = orbgpu::sim3_inverse(T);
                }
                __syncthreads();
                errors(robust);
                if (tid == 0) {
                    bool accept;
                    const int c = orbgpu::optsim3_lm_decide(lm, tot[0], ok, x, sys + 28, accept);
                    if (accept) sCur = sP[14];
                    s_cmd = c;
                }
                __syncthreads();
                cmd = s_cmd;
                if (cmd != orbgpu::kOptSim3Trial) break;
            }
            if (cmd == orbgpu::kOptSim3Done) break;
        }
        __syncthreads();
    };
    auto count = [&](int mine) {
        reduce1((double)mine);
        const int total = (int)tot[0];
        __syncthreads();  // tot[0] is rewritten by the next reduction
        return total;
    };

    int nBad = 0;
    for (int stage = 0; stage < 2; ++stage) {
        // ---- optimize(5) with the kernels, then optimize(nMoreIterations) without
        optimize(stage == 0 ? 5 : (nBad > 0 ? 10 : 5), stage == 0);
        if (stage == 1) break;
        // ---- the first cull, on the stored errors (:4418-4447)
        int mine = 0;
        for (int i = tid; i < n; i += kOsThreads) {
            const bool bad = lc12[i] > th2 || lc21[i] > th2;
            lbad[i] = bad;
            mine += bad;
        }
        nBad = count(mine);
        if (n - nBad < 10) {  // return 0, g2oS12 unchanged (s12_out already holds the input)
            for (int i = tid; i < n; i += kOsThreads) {
                P.inlier[i] = !lbad[i];
                if (P.chi2_12) P.chi2_12[i] = lc12[i];
                if (P.chi2_21) P.chi2_21[i] = lc21[i];
            }
            if (tid == 0) {
                *P.n_in = 0;
                *P.n_bad = nBad;
            }
            return;
        }
    }
    // ---- the second cull: computeError() at the final estimate (:4467-4486)
    if (tid == 0) {
        const Sim3d S = sCur;
        sP[14] = S;
        sPi[14] = orbgpu::sim3_inverse(S);
    }
    __syncthreads();
    errors(false);
    int mine = 0;
    for (int i = tid; i < n; i += kOsThreads) {
        const bool in = !lbad[i] && !(lc12[i] > th2 || lc21[i] > th2);
        P.inlier[i] = in;
        mine += in;
        if (P.chi2_12) P.chi2_12[i] = lc12[i];
        if (P.chi2_21) P.chi2_21[i] = lc21[i];
    }
    const int nIn = count(mine);
    if (tid < 4) P.s12_out[tid] = sCur.q[tid];
    else if (tid < 7) P.s12_out[tid] = sCur.t[tid - 4];
    else if (tid == 7) P.s12_out[7] = sCur.s;
    if (tid == 0) {
        *P.n_in = nIn;
        *P.n_bad = nBad;
    }
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

bool optsim3_args_ok(const orb_optsim3_problem_t& p, const orb_optsim3_out_t& o) {
    if (p.n < 0 || p.n > kOsRoom || !(p.th2 > 0.f) || !std::isfinite(p.th2)) return false;
    if (p.n > 0 && (!p.p1c || !p.p2c || !p.obs1 || !p.obs2 || !p.inv_sigma2_1 || !p.inv_sigma2_2 || !o.inlier)) return false;
    return o.s12_out && o.n_in && o.n_bad;
}

int optsim3_check(const orb_optsim3_problem_t* problems, int n_problems, const orb_optsim3_out_t* outs) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !outs)))
        return orbgpu_fail(ORB_ERR_ARG, "bad OptimizeSim3 arguments");
    for (int k = 0; k < n_problems; ++k)
        if (!optsim3_args_ok(problems[k], outs[k]))
            return orbgpu_fail(ORB_ERR_ARG, "OptimizeSim3: invalid problem (0 <= n <= 1024, th2 > 0, no NULL array)");
    return ORB_OK;
}

// The launches of one call; every pointer device memory.
int optsim3_launch(const orb_optsim3_problem_t* probs, int n_problems, const orb_optsim3_out_t* outs, hipStream_t s) {
    for (int base = 0; base < n_problems; base += kOsPerLaunch) {
        const int cnt = std::min(kOsPerLaunch, n_problems - base);
        OsLaunch L;
        memset(&L, 0, sizeof(L));
        for (int k = 0; k < cnt; ++k) {
            const orb_optsim3_problem_t& p = probs[base + k];
            const orb_optsim3_out_t& o = outs[base + k];
            OsProb& q = L.p[k];
            q.n = p.n; q.fix_scale = p.fix_scale; q.th2 = p.th2;
            memcpy(q.cam1, p.cam1, sizeof(q.cam1));
            memcpy(q.cam2, p.cam2, sizeof(q.cam2));
            memcpy(q.s12, p.s12, sizeof(q.s12));
            q.p1c = p.p1c; q.p2c = p.p2c; q.obs1 = p.obs1; q.obs2 = p.obs2;
            q.is1 = p.inv_sigma2_1; q.is2 = p.inv_sigma2_2;
            q.s12_out = o.s12_out; q.n_in = o.n_in; q.n_bad = o.n_bad; q.inlier = o.inlier;
            q.chi2_12 = o.chi2_12; q.chi2_21 = o.chi2_21;
        }
        hipLaunchKernelGGL(k_optsim3, dim3(cnt), dim3(kOsThreads), 0, s, L);
    }
    return hipGetLastError() == hipSuccess ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "OptimizeSim3 kernel launch failed");
}

}  // namespace

extern "C" {

int orb_optimize_sim3_device(const orb_optsim3_problem_t* problems, int n_problems, const orb_optsim3_out_t* outs,
                             void* stream) {
    const int rc = optsim3_check(problems, n_problems, outs);
    if (rc != ORB_OK || n_problems == 0) return rc;
    return optsim3_launch(problems, n_problems, outs, (hipStream_t)stream);
}

int orb_optimize_sim3(const orb_optsim3_problem_t* problems, int n_problems, const orb_optsim3_out_t* outs) {
    const int rc0 = optsim3_check(problems, n_problems, outs);
    if (rc0 != ORB_OK || n_problems == 0) return rc0;
    if (orb_device_count() <= 0) return orbgpu_fail(ORB_ERR_DEVICE, "no HIP device visible");
    // packed layout: per problem p1c | p2c | obs1 | obs2 | is1 | is2 (one upload), then s12_out | n_in, n_bad |
    // inlier | chi2_12 | chi2_21 (one download)
    struct Off { size_t p1, p2, o1, o2, i1, i2, s, nn, in, c12, c21; };
    std::vector<Off> offs(n_problems);
    size_t off = 0;
    for (int k = 0; k < n_problems; ++k) {
        const size_t n = (size_t)std::max(problems[k].n, 1);
        Off& o = offs[k];
        o.p1 = off; off = align256(off + 24 * n);
        o.p2 = off; off = align256(off + 24 * n);
        o.o1 = off; off = align256(off + 16 * n);
        o.o2 = off; off = align256(off + 16 * n);
        o.i1 = off; off = align256(off + 4 * n);
        o.i2 = off; off = align256(off + 4 * n);
    }
    const size_t in_bytes = off;
    for (int k = 0; k < n_problems; ++k) {
        const size_t n = (size_t)std::max(problems[k].n, 1);
        Off& o = offs[k];
        o.s = off; off = align256(off + 64);
        o.nn = off; off = align256(off + 8);
        o.in = off; off = align256(off + n);
        o.c12 = off; off = align256(off + 8 * n);
        o.c21 = off; off = align256(off + 8 * n);
    }
    std::vector<char> h(off);
    std::vector<orb_optsim3_problem_t> dp(problems, problems + n_problems);
    std::vector<orb_optsim3_out_t> dout(n_problems);
    hipStream_t s = hipStreamPerThread;
    char* d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d), off, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    for (int k = 0; k < n_problems; ++k) {
        const orb_optsim3_problem_t& p = problems[k];
        const Off& o = offs[k];
        const size_t n = (size_t)p.n;
        if (n) {
            memcpy(&h[o.p1], p.p1c, 24 * n);
            memcpy(&h[o.p2], p.p2c, 24 * n);
            memcpy(&h[o.o1], p.obs1, 16 * n);
            memcpy(&h[o.o2], p.obs2, 16 * n);
            memcpy(&h[o.i1], p.inv_sigma2_1, 4 * n);
            memcpy(&h[o.i2], p.inv_sigma2_2, 4 * n);
        }
        dp[k].p1c = reinterpret_cast<const double*>(d + o.p1);
        dp[k].p2c = reinterpret_cast<const double*>(d + o.p2);
        dp[k].obs1 = reinterpret_cast<const double*>(d + o.o1);
        dp[k].obs2 = reinterpret_cast<const double*>(d + o.o2);
        dp[k].inv_sigma2_1 = reinterpret_cast<const float*>(d + o.i1);
        dp[k].inv_sigma2_2 = reinterpret_cast<const float*>(d + o.i2);
        dout[k] = orb_optsim3_out_t{reinterpret_cast<double*>(d + o.s), reinterpret_cast<int32_t*>(d + o.nn),
                                    reinterpret_cast<int32_t*>(d + o.nn + 4), reinterpret_cast<uint8_t*>(d + o.in),
                                    reinterpret_cast<double*>(d + o.c12), reinterpret_cast<double*>(d + o.c21)};
    }
    int rc = ORB_OK;
    if (hipMemcpyAsync(d, h.data(), in_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = orbgpu_fail(ORB_ERR_DEVICE, "OptimizeSim3 upload failed");
    if (rc == ORB_OK) rc = optsim3_launch(dp.data(), n_problems, dout.data(), s);
    if (rc == ORB_OK && (hipMemcpyAsync(&h[in_bytes], d + in_bytes, off - in_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                         hipStreamSynchronize(s) != hipSuccess))
        rc = orbgpu_fail(ORB_ERR_DEVICE, "OptimizeSim3 device error");
    if (hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    if (rc != ORB_OK) return rc;
    for (int k = 0; k < n_problems; ++k) {
        const orb_optsim3_problem_t& p = problems[k];
        const orb_optsim3_out_t& o = outs[k];
        const Off& f = offs[k];
        const size_t n = (size_t)p.n;
        memcpy(o.s12_out, &h[f.s], 64);
        memcpy(o.n_in, &h[f.nn], 4);
        memcpy(o.n_bad, &h[f.nn + 4], 4);
        if (n) {
            memcpy(o.inlier, &h[f.in], n);
            if (o.chi2_12) memcpy(o.chi2_12, &h[f.c12], 8 * n);
            if (o.chi2_21) memcpy(o.chi2_21, &h[f.c21], 8 * n);
        }
    }
    return ORB_OK;
}

}  // extern "C"
