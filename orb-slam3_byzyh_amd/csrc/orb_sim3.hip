// Sim3Solver's RANSAC on MI355X (reference src/Sim3Solver.cc:149-439, called at src/LoopClosing.cc:899-913),
// batched over loop-closing candidates and over hypotheses.  Pinhole cameras only, like the rest of the library.
//
// The reference draws a triple, solves Horn's closed form, reprojects all N correspondences both ways and stops
// at the first hypothesis with more than mRansacMinInliers inliers.  The hypotheses do not depend on each other,
// so every one of them is evaluated and the serial control flow becomes a selection over the counts:
//   winner = the first hypothesis with count > min_inliers        (where iterate() returns)
//   best   = the last hypothesis attaining the maximum count      (mnBestInliers is updated on >=)
// The random draws stay with the caller: the sample triples are an input.
//
//   k_sim3_hypotheses  grid (ceil(n_hyp / 64), problem), 256 threads.  A block owns 64 hypotheses.  Wave 0 solves
//                      their closed forms, one lane each (orb_sim3_math.h: FP64, rounded to float once), and
//                      leaves T12 / T21 in LDS.  Then the four waves share the 64-point words of the problem:
//                      a lane holds one correspondence in registers and walks the block's hypotheses (the
//                      transform is an LDS broadcast); one ballot per (hypothesis, word) is the mask word, which
//                      lane j keeps for hypothesis j and stores after the walk; the counts are popcounts of the
//                      words, summed over the waves through LDS.  The points come through L2 (<= 48 B each).
//   k_sim3_resolve     one wave per problem: winner and best by a wave reduction over the counts, then the chosen
//                      row of the mask table unpacked into inlier_mask.
//
// The problem records travel as kernel arguments, 16 problems to a launch: no staging buffer, no upload, nothing
// to wait for, so the device form only enqueues.  A triple with an index out of range or a repeated index is not
// read: its hypothesis gets count -1, a NaN transform and an empty mask row, and is never selected.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_sim3_math.h"
#include "orbgpu.h"
#include "orbgpu_internal.h"

namespace {

constexpr int kSim3Threads = 256;
constexpr int kSim3Waves = kSim3Threads / 64;
constexpr int kSim3HypPerBlock = 64;
constexpr int kSim3PerLaunch = 16;
constexpr int kSim3MaxHyp = 1024;
constexpr int kSim3MaxN = 1 << 20;

struct Sim3Prob {
    int n, n_hyp, min_inliers, fix_scale;
    float cam1[4], cam2[4];
    const float *x1, *x2, *e1, *e2;
    const int32_t* samples;
    int32_t* hyp_inliers;
    float* hyp_t12;
    float* hyp_scale;
    int32_t *winner, *best;
    uint8_t* inlier_mask;
    uint64_t* mask;  // n_hyp x ceil(n / 64): the caller's hyp_mask or the call's scratch
};
struct Sim3Launch {
    Sim3Prob p[kSim3PerLaunch];
};

__host__ __device__ inline int sim3_words(int n) { return (n + 63) >> 6; }

__global__ __launch_bounds__(kSim3Threads) void k_sim3_hypotheses(const Sim3Launch L) {
    __shared__ float s_T12[kSim3HypPerBlock][12];
    __shared__ float s_T21[kSim3HypPerBlock][12];
    __shared__ int s_cnt[kSim3Waves][kSim3HypPerBlock];
    const Sim3Prob& P = L.p[blockIdx.y];
    const int h0 = blockIdx.x * kSim3HypPerBlock;
    const int n = P.n;
    if (h0 >= P.n_hyp || n < P.min_inliers) return;  // block-uniform (n < min_inliers: bNoMore, nothing evaluated)
    const int nh = min(kSim3HypPerBlock, P.n_hyp - h0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = sim3_words(n);

    bool valid = false;
    if (wave == 0 && lane < nh) {
        const int h = h0 + lane;
        const int i0 = P.samples[3 * h], i1 = P.samples[3 * h + 1], i2 = P.samples[3 * h + 2];
        valid = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n && i0 != i1 && i0 != i2 && i1 != i2;
        float T12[12], T21[12], s;
        if (valid) {
            float p1[3][3], p2[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p1[0][k] = P.x1[3 * i0 + k]; p1[1][k] = P.x1[3 * i1 + k]; p1[2][k] = P.x1[3 * i2 + k];
                p2[0][k] = P.x2[3 * i0 + k]; p2[1][k] = P.x2[3 * i1 + k]; p2[2][k] = P.x2[3 * i2 + k];
            }
            orbgpu::sim3_closed_form(p1, p2, P.fix_scale != 0, T12, T21, &s);
        } else {
            s = __builtin_nanf("");
#pragma unroll
            for (int k = 0; k < 12; ++k) T12[k] = T21[k] = s;
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            s_T12[lane][k] = T12[k];
            s_T21[lane][k] = T21[k];
            P.hyp_t12[12 * (size_t)h + k] = T12[k];
        }
        P.hyp_scale[h] = s;
    }
    __syncthreads();

    int cnt = 0;  // lane j: hypothesis h0 + j's inliers among this wave's words
    for (int w = wave; w < W; w += kSim3Waves) {
        const int i = w * 64 + lane;
        const bool in = i < n;
        float X1[3] = {0.f, 0.f, 1.f}, X2[3] = {0.f, 0.f, 1.f}, thr1 = 0.f, thr2 = 0.f;
        if (in) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                X1[k] = P.x1[3 * (size_t)i + k];
                X2[k] = P.x2[3 * (size_t)i + k];
            }
            thr1 = P.e1[i];
            thr2 = P.e2[i];
        }
        // mvP1im1, mvP2im2 (FromCameraToImage, :477-487)
        const float im1[2] = {P.cam1[0] * X1[0] / X1[2] + P.cam1[2], P.cam1[1] * X1[1] / X1[2] + P.cam1[3]};
        const float im2[2] = {P.cam2[0] * X2[0] / X2[2] + P.cam2[2], P.cam2[1] * X2[1] / X2[2] + P.cam2[3]};
        unsigned long long word = 0;
        for (int j = 0; j < nh; ++j) {  // wave-uniform: every lane votes
            const bool ok = in && orbgpu::sim3_inlier(s_T12[j], s_T21[j], X1, X2, im1, im2, P.cam1, P.cam2, thr1, thr2);
            const unsigned long long b = __ballot(ok);
            if (lane == j) word = b;
        }
        if (lane < nh) {
            P.mask[(size_t)(h0 + lane) * W + w] = word;
            cnt += __popcll(word);
        }
    }
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && lane < nh) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < kSim3Waves; ++k) total += s_cnt[k][lane];
        P.hyp_inliers[h0 + lane] = valid ? total : -1;
    }
}

__global__ __launch_bounds__(64) void k_sim3_resolve(const Sim3Launch L) {
    const Sim3Prob& P = L.p[blockIdx.x];
    const int lane = threadIdx.x, n = P.n;
    int first = INT32_MAX;      // the first hypothesis past min_inliers
    long long key = -1;         // (count << 11 | h): the maximum is the last hypothesis of the largest count
    if (n >= P.min_inliers) {
        for (int h = lane; h < P.n_hyp; h += 64) {
            const int c = P.hyp_inliers[h];
            if (c < 0) continue;
            if (c > P.min_inliers) first = min(first, h);
            const long long k = ((long long)c << 11) | h;
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        first = min(first, __shfl_xor(first, d, 64));
        const long long other = __shfl_xor(key, d, 64);
        key = other > key ? other : key;
    }
    const int winner = first == INT32_MAX ? -1 : first;
    const int best = key < 0 ? -1 : (int)(key & 2047);
    if (lane == 0) {
        *P.winner = winner;
        *P.best = best;
    }
    const int row = winner >= 0 ? winner : best;
    const int W = sim3_words(n);
    for (int i = lane; i < n; i += 64)
        P.inlier_mask[i] = row < 0 ? 0 : (uint8_t)((P.mask[(size_t)row * W + (i >> 6)] >> (i & 63)) & 1ull);
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

bool sim3_args_ok(const orb_sim3_problem_t& p, const orb_sim3_out_t& o) {
    if (p.n < 0 || p.n > kSim3MaxN || p.n_hyp < 1 || p.n_hyp > kSim3MaxHyp || !p.samples) return false;
    if (p.n > 0 && (!p.x3dc1 || !p.x3dc2 || !p.max_err1 || !p.max_err2 || !o.inlier_mask)) return false;
    return o.hyp_inliers && o.hyp_t12 && o.hyp_scale && o.winner && o.best;
}

size_t sim3_mask_bytes(const orb_sim3_problem_t& p) { return align256(8 * (size_t)p.n_hyp * std::max(sim3_words(p.n), 1)); }

// The launches of one call; every pointer device memory; scratch: the mask tables of the problems whose
// hyp_mask is NULL, sim3_mask_bytes each, in order.
int sim3_launch(const orb_sim3_problem_t* probs, int n_problems, const orb_sim3_out_t* outs, char* scratch, hipStream_t s) {
    size_t off = 0;
    for (int base = 0; base < n_problems; base += kSim3PerLaunch) {
        const int cnt = std::min(kSim3PerLaunch, n_problems - base);
        Sim3Launch L;
        memset(&L, 0, sizeof(L));
        int max_hyp = 0;
        for (int k = 0; k < cnt; ++k) {
            const orb_sim3_problem_t& p = probs[base + k];
            const orb_sim3_out_t& o = outs[base + k];
            Sim3Prob& q = L.p[k];
            q.n = p.n; q.n_hyp = p.n_hyp; q.min_inliers = p.min_inliers; q.fix_scale = p.fix_scale;
            memcpy(q.cam1, p.cam1, sizeof(q.cam1));
            memcpy(q.cam2, p.cam2, sizeof(q.cam2));
            q.x1 = p.x3dc1; q.x2 = p.x3dc2; q.e1 = p.max_err1; q.e2 = p.max_err2;
            q.samples = p.samples;
            q.hyp_inliers = o.hyp_inliers; q.hyp_t12 = o.hyp_t12; q.hyp_scale = o.hyp_scale;
            q.winner = o.winner; q.best = o.best; q.inlier_mask = o.inlier_mask;
            q.mask = o.hyp_mask;
            if (!q.mask) {
                q.mask = reinterpret_cast<uint64_t*>(scratch + off);
                off += sim3_mask_bytes(p);
            }
            if (p.n >= p.min_inliers) max_hyp = std::max(max_hyp, p.n_hyp);
        }
        if (max_hyp > 0)
            hipLaunchKernelGGL(k_sim3_hypotheses, dim3((max_hyp + kSim3HypPerBlock - 1) / kSim3HypPerBlock, cnt),
                               dim3(kSim3Threads), 0, s, L);
        hipLaunchKernelGGL(k_sim3_resolve, dim3(cnt), dim3(64), 0, s, L);
    }
    return hipGetLastError() == hipSuccess ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "Sim3 RANSAC kernel launch failed");
}

}  // namespace

extern "C" {

int orb_sim3_ransac_device(const orb_sim3_problem_t* problems, int n_problems, const orb_sim3_out_t* outs, void* stream) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !outs)))
        return orbgpu_fail(ORB_ERR_ARG, "bad Sim3 RANSAC arguments");
    size_t scratch = 0;
    for (int k = 0; k < n_problems; ++k) {
        if (!sim3_args_ok(problems[k], outs[k]))
            return orbgpu_fail(ORB_ERR_ARG, "Sim3 RANSAC: invalid problem (n <= 2^20, 1 <= n_hyp <= 1024, no NULL array)");
        if (!outs[k].hyp_mask) scratch += sim3_mask_bytes(problems[k]);
    }
    if (n_problems == 0) return ORB_OK;
    hipStream_t s = (hipStream_t)stream;
    char* d = nullptr;  // stream-ordered (calls on different streams do not share it)
    if (scratch && hipMallocAsync(reinterpret_cast<void**>(&d), scratch, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    int rc = sim3_launch(problems, n_problems, outs, d, s);
    if (d && hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    return rc;
}

int orb_sim3_ransac(const orb_sim3_problem_t* problems, int n_problems, const orb_sim3_out_t* outs) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !outs)))
        return orbgpu_fail(ORB_ERR_ARG, "bad Sim3 RANSAC arguments");
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = problems[k];
        if (!sim3_args_ok(p, outs[k]))
            return orbgpu_fail(ORB_ERR_ARG, "Sim3 RANSAC: invalid problem (n <= 2^20, 1 <= n_hyp <= 1024, no NULL array)");
        if (p.n < p.min_inliers) continue;  // not evaluated: its samples are not read
        for (int h = 0; h < p.n_hyp; ++h) {
            const int32_t* t = &p.samples[3 * h];
            if (t[0] < 0 || t[0] >= p.n || t[1] < 0 || t[1] >= p.n || t[2] < 0 || t[2] >= p.n || t[0] == t[1] ||
                t[0] == t[2] || t[1] == t[2])
                return orbgpu_fail(ORB_ERR_ARG, "Sim3 RANSAC: a sample triple repeats an index or leaves 0..n-1");
        }
    }
    if (n_problems == 0) return ORB_OK;
    // packed layout: per problem x1 | x2 | e1 | e2 | samples (one upload), then hyp_inliers | hyp_t12 | hyp_scale |
    // winner, best | inlier_mask | the mask table (one download: the table only where the caller asked for it)
    struct Off { size_t x1, x2, e1, e2, smp, cnt, t12, scl, wb, im, mask; };
    std::vector<Off> offs(n_problems);
    size_t off = 0;
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = problems[k];
        const size_t n = (size_t)std::max(p.n, 1);
        Off& o = offs[k];
        o.x1 = off; off = align256(off + 12 * n);
        o.x2 = off; off = align256(off + 12 * n);
        o.e1 = off; off = align256(off + 4 * n);
        o.e2 = off; off = align256(off + 4 * n);
        o.smp = off; off = align256(off + 12 * (size_t)p.n_hyp);
    }
    const size_t in_bytes = off;
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = problems[k];
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 4 * (size_t)p.n_hyp);
        o.t12 = off; off = align256(off + 48 * (size_t)p.n_hyp);
        o.scl = off; off = align256(off + 4 * (size_t)p.n_hyp);
        o.wb = off; off = align256(off + 8);
        o.im = off; off = align256(off + (size_t)std::max(p.n, 1));
        o.mask = off; off += sim3_mask_bytes(p);
    }
    std::vector<char> h(off);
    std::vector<orb_sim3_problem_t> dp(problems, problems + n_problems);
    std::vector<orb_sim3_out_t> dout(n_problems);
    hipStream_t s = hipStreamPerThread;
    char* d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d), off, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = problems[k];
        const Off& o = offs[k];
        const size_t n = (size_t)p.n;
        if (n) {
            memcpy(&h[o.x1], p.x3dc1, 12 * n);
            memcpy(&h[o.x2], p.x3dc2, 12 * n);
            memcpy(&h[o.e1], p.max_err1, 4 * n);
            memcpy(&h[o.e2], p.max_err2, 4 * n);
        }
        memcpy(&h[o.smp], p.samples, 12 * (size_t)p.n_hyp);
        dp[k].x3dc1 = reinterpret_cast<const float*>(d + o.x1);
        dp[k].x3dc2 = reinterpret_cast<const float*>(d + o.x2);
        dp[k].max_err1 = reinterpret_cast<const float*>(d + o.e1);
        dp[k].max_err2 = reinterpret_cast<const float*>(d + o.e2);
        dp[k].samples = reinterpret_cast<const int32_t*>(d + o.smp);
        dout[k] = orb_sim3_out_t{reinterpret_cast<int32_t*>(d + o.cnt), reinterpret_cast<float*>(d + o.t12),
                                 reinterpret_cast<float*>(d + o.scl), reinterpret_cast<int32_t*>(d + o.wb),
                                 reinterpret_cast<int32_t*>(d + o.wb + 4), reinterpret_cast<uint8_t*>(d + o.im),
                                 reinterpret_cast<uint64_t*>(d + o.mask)};
    }
    int rc = ORB_OK;
    if (hipMemcpyAsync(d, h.data(), in_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = orbgpu_fail(ORB_ERR_DEVICE, "Sim3 RANSAC upload failed");
    if (rc == ORB_OK) rc = sim3_launch(dp.data(), n_problems, dout.data(), nullptr, s);
    if (rc == ORB_OK && (hipMemcpyAsync(&h[in_bytes], d + in_bytes, off - in_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                         hipStreamSynchronize(s) != hipSuccess))
        rc = orbgpu_fail(ORB_ERR_DEVICE, "Sim3 RANSAC device error");
    if (hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    if (rc != ORB_OK) return rc;
    for (int k = 0; k < n_problems; ++k) {
        const orb_sim3_problem_t& p = problems[k];
        const orb_sim3_out_t& o = outs[k];
        const Off& f = offs[k];
        memcpy(o.winner, &h[f.wb], 4);
        memcpy(o.best, &h[f.wb + 4], 4);
        if (p.n) memcpy(o.inlier_mask, &h[f.im], (size_t)p.n);
        if (p.n < p.min_inliers) continue;  // nothing was evaluated: the per-hypothesis arrays stay as they were
        memcpy(o.hyp_inliers, &h[f.cnt], 4 * (size_t)p.n_hyp);
        memcpy(o.hyp_t12, &h[f.t12], 48 * (size_t)p.n_hyp);
        memcpy(o.hyp_scale, &h[f.scl], 4 * (size_t)p.n_hyp);
        if (o.hyp_mask) memcpy(o.hyp_mask, &h[f.mask], 8 * (size_t)p.n_hyp * sim3_words(p.n));
    }
    return ORB_OK;
}

}  // extern "C"
