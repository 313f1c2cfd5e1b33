// The Sim3 searches of loop closing on MI355X, batched: ORBmatcher::SearchByProjection(KF, Scw, vpPoints,
// vpMatched, th, ratioHamming) (reference src/ORBmatcher.cc:496-619), its overload that also fills vpMatchedKF
// (:621-733) and the search half of ORBmatcher::Fuse(KF, Scw, vpPoints, th, vpReplacePoint) (:1547-1651), as
// LoopClosing.cc calls them (:976, :1005, :1265, :2712, :2765).  KeyFrame::GetFeaturesInArea / IsInImage
// src/KeyFrame.cc:843-897; MapPoint::PredictScale src/MapPoint.cc:688-706.
//
// A job is one call of a reference function: a keyframe, a pose (Tcw, Ow: the SE3 of the candidate's Sim3), a
// range of a shared point pool, th, ratioHamming and a mode.  Jobs of one call may share a keyframe.
//   k_s3p_grid     one workgroup per distinct keyframe: KeyFrame::mGrid and the packed (x, y, angle, octave)
//                  rows (k_frame_prep_body of orb_frame_grid.h)
//   k_s3p_search   blockIdx.y = job, one thread per point, 256 points per block.  The block stages the
//                  keyframe's 3,073 cell offsets and, when the keyframe has at most kS3pLdsRows keypoints, its
//                  keypoint records and cell index list in LDS (a larger keyframe leaves them in global memory:
//                  the same walk, the same results); the point's descriptor sits in registers; a keyframe
//                  descriptor is read only for a keypoint inside the window whose octave passed.  FUSE mode
//                  keeps the first Hamming minimum.  The claim modes keep, per point, the candidates whose
//                  distance passes the threshold, the kS3pKeep best by (distance, scan position), and their
//                  count.
//   k_s3p_resolve  one workgroup per claim job: the reference's one sequential rule -- a keypoint an earlier
//                  point matched (vpMatched[idx] != NULL, :589 / :704) is skipped by every later point --
//                  resolved by fixed-point rounds.  Every round posts claim[j] = the smallest point whose
//                  current answer is keypoint j (pre-filled vpMatched entries, taken0, claim from the start),
//                  then every point takes the first of its kept candidates that no earlier point claims.  The
//                  fixed point is the sequential loop's result by induction on the point index (point i's
//                  answer depends only on the answers of points below i), and after round r the first r points
//                  are final, so the rounds end.  A point can only ever claim a keypoint whose distance passes
//                  the threshold -- when its best unclaimed candidate fails it claims nothing -- so the
//                  candidates that fail never change an outcome and are not kept.  A point whose kept
//                  candidates are all claimed while its window held more passing ones walks its window again,
//                  skipping the claimed keypoints: nothing is truncated.
//
// Float arithmetic as the reference build (g++ -O3 -march=native) contracts it (oracle/orb_frustum_oracle.cpp,
// oracle/orb_projection_oracle.cpp: `a*b + c*d` -> fma(a, b, c*d), `a*b + c` -> fma(a, b, c)).  This file is
// compiled with -ffp-contract=off and every fma is explicit:
//   Pc[r]  = fma(R[r][2], P[2], fma(R[r][0], P[0], R[r][1] * P[1])) + t[r]
//   dot3   = fma(a[2], b[2], fma(a[0], b[0], a[1] * b[1]))      (|PO|^2 and PO . normal)
//   PROJECT, FUSE (Pinhole::project):   u = fx * Pc[0] / Pc[2] + cx
//   INVZ (:660-665):   invz = 1 / Pc[2];  x = Pc[0] * invz;  u = fma(fx, x, cx)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_frame_grid.h"
#include "orb_predict_scale.h"
#include "orbgpu.h"
#include "orbgpu_internal.h"

// Defined in orb_triangulation.hip: the matcher handle's staging buffers.
int orbgpu_matcher_reserve(orb_matcher_t m, size_t bytes, char** d_buf, char** h_buf, hipStream_t* stream,
                           int* check_ori);
int orbgpu_matcher_upload_slot(orb_matcher_t m, size_t bytes, char** h);
int orbgpu_matcher_upload_mark(orb_matcher_t m, hipStream_t s);

namespace {

constexpr int kThLow = 50;              // src/ORBmatcher.cc:37
constexpr int kS3pMaxLevels = 12;
constexpr int kS3pThreads = 256;
constexpr int kS3pLdsRows = 2048;       // keypoint records staged in LDS: 20 B each + the cell offsets = 53,252 B
constexpr int kS3pMaxCap = 16384;       // k_frame_prep_body's limit
constexpr int kS3pMaxPool = 1 << 20;
constexpr int kS3pMaxJobPoints = 1 << 24;  // the sum of the jobs' point counts (the per-point scratch)
constexpr int kS3pMaxJobs = 65535, kS3pMaxKfs = 1024;
constexpr int kS3pKeep = 8;             // passing candidates kept per point for the rounds
constexpr int kResolveThreads = 1024;
constexpr int kClaimLds = 8192;         // claims in LDS up to this many keypoints, else in the job's matched row
constexpr uint32_t kNoCand = 0xffffffffu;

// one keyframe as the kernels read it
struct S3pKf {
    const orb_keypoint_t* kps;   // mvKeysUn (cap)
    const int32_t* n_raw;        // KeyFrame::N as its producer left it
    const uint4* desc;           // mDescriptors
    float4* kp4;                 // scratch: x, y, angle, octave bits
    int32_t* cell_off;           // scratch: kCells + 1
    int32_t* cell_idx;           // scratch: cap
    int32_t* cell_of;            // scratch: cap
    int32_t* misc;               // scratch: [0] the clamped count, [4..7] k_frame_prep_body's zero words
    int cap, nlevels;
    float min_x, max_x, min_y, max_y, inv_w, inv_h, fx, fy, cx, cy;
    float scale[kS3pMaxLevels];
    float steps[kS3pMaxLevels];  // MapPoint::PredictScale level thresholds (orb_predict_scale.h)
};

// one job
struct S3pJob {
    int kf, first, count, mode;
    int out_off;                 // its points' place in skip / best_idx / best_dist / the per-point scratch
    float th, thr;               // thr = TH_LOW * ratioHamming, the float product (:610 / :723)
    float Tcw[12], Ow[3];
};

// what the search leaves for the rounds, per point of a claim job
struct S3pPoint {
    float u, v, radius;
    int level;
    int npass;                   // candidates that passed the threshold (0: gated, skipped or none)
    uint32_t keep[kS3pKeep];     // the best of them by (distance, scan position): keypoint | distance << 16
};

__global__ __launch_bounds__(kPrepThreads) void k_s3p_grid(const S3pKf* __restrict__ kfs) {
    const S3pKf& K = kfs[blockIdx.y];
    k_frame_prep_body(K.kps, K.n_raw, K.cap, K.min_x, K.min_y, K.inv_w, K.inv_h, K.kp4, K.cell_off, K.cell_idx, K.cell_of,
                      K.misc, nullptr, ScratchInit{nullptr, 0, nullptr, 0, K.misc + 4, nullptr, -1});
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return fmaf(a[2], b[2], fmaf(a[0], b[0], a[1] * b[1]));
}

__device__ __forceinline__ int kf_count(const S3pKf& K) {
    const int raw = *K.n_raw;
    return raw < 0 || raw > K.cap ? 0 : raw;  // a flagged count: no keypoints, no matches
}

// The window walk in GetFeaturesInArea's order with the octave test (:592-596 / :707-710 / :1637-1640):
// fn(j) for every keypoint j that is a candidate.  KP / CO / CI: the keyframe's records, global pointers or
// LDS readers.
template <class KP, class CO, class CI, class Fn>
__device__ __forceinline__ void s3p_window(const S3pKf& K, KP kp4, CO cell_off, CI cell_idx, float u, float v, float radius,
                                           int level, Fn fn) {
    const int x0 = max(0, (int)floorf((u - K.min_x - radius) * K.inv_w));
    if (x0 >= kGridCols) return;
    const int x1 = min(kGridCols - 1, (int)ceilf((u - K.min_x + radius) * K.inv_w));
    if (x1 < 0) return;
    const int y0 = max(0, (int)floorf((v - K.min_y - radius) * K.inv_h));
    if (y0 >= kGridRows) return;
    const int y1 = min(kGridRows - 1, (int)ceilf((v - K.min_y + radius) * K.inv_h));
    if (y1 < 0) return;
    for (int ix = x0; ix <= x1; ++ix) {
        // cells (ix, y0 .. y1) are consecutive: one span of the index list, in the reference's order
        const int b = cell_off[ix * kGridRows + y0], e = cell_off[ix * kGridRows + y1 + 1];
        for (int k = b; k < e; ++k) {
            const int j = cell_idx[k];
            const float4 kp = kp4[j];
            if (!(fabsf(kp.x - u) < radius && fabsf(kp.y - v) < radius)) continue;  // GetFeaturesInArea (KeyFrame.cc:884)
            const int oct = __float_as_int(kp.w);
            if (oct < level - 1 || oct > level) continue;
            fn(j);
        }
    }
}

// the gates before the window (:526-572); false: the point is not searched
__device__ __forceinline__ bool s3p_gates(const S3pKf& K, const S3pJob& J, const float P[3], const float Pn[3], float mind,
                                          float maxd, float& u, float& v, float& radius, int& level) {
    float Pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        Pc[r] = fmaf(J.Tcw[4 * r + 2], P[2], fmaf(J.Tcw[4 * r], P[0], J.Tcw[4 * r + 1] * P[1])) + J.Tcw[4 * r + 3];
    if (Pc[2] < 0.0f) return false;                                 // :538
    if (J.mode == ORB_S3P_CLAIM_INVZ) {                             // :660-665
        const float invz = 1.0f / Pc[2];
        u = fmaf(K.fx, Pc[0] * invz, K.cx);
        v = fmaf(K.fy, Pc[1] * invz, K.cy);
    } else {                                                        // Pinhole::project(Eigen::Vector3f)
        u = K.fx * Pc[0] / Pc[2] + K.cx;
        v = K.fy * Pc[1] / Pc[2] + K.cy;
    }
    if (!(u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y)) return false;  // KeyFrame::IsInImage
    const float PO[3] = {P[0] - J.Ow[0], P[1] - J.Ow[1], P[2] - J.Ow[2]};
    const float dist = sqrtf(dot3(PO, PO));
    if (dist < 0.8f * mind || dist > 1.2f * maxd) return false;     // :557 (Get{Min,Max}DistanceInvariance)
    if (dot3(PO, Pn) < 0.5f * dist) return false;                   // :564 (0.5 * dist is exact in double too)
    level = orbgpu::predict_scale_level(maxd / dist, K.steps, K.nlevels);
    radius = J.th * K.scale[level];
    return true;
}

// the search's per-candidate state: FUSE keeps the first minimum, the claim modes the sorted kept list
struct S3pFound {
    int bestDist = 256, bestIdx = -1;
    int npass = 0;
    uint32_t key[kS3pKeep];  // distance << 20 | scan position among the passing candidates
    int kp[kS3pKeep];
};

template <class KP, class CO, class CI>
__device__ __forceinline__ void s3p_search_point(const S3pKf& K, const S3pJob& J, KP kp4, CO cell_off, CI cell_idx, float u,
                                                 float v, float radius, int level, const uint4 d0, const uint4 d1,
                                                 S3pFound& f) {
    if (J.mode == ORB_S3P_FUSE) {
        s3p_window(K, kp4, cell_off, cell_idx, u, v, radius, level, [&](int j) {
            const int dist = hamming(d0, d1, K.desc[2 * (size_t)j], K.desc[2 * (size_t)j + 1]);
            if (dist < f.bestDist) {                                // :1646-1650
                f.bestDist = dist;
                f.bestIdx = j;
            }
        });
        return;
    }
    s3p_window(K, kp4, cell_off, cell_idx, u, v, radius, level, [&](int j) {
        const int dist = hamming(d0, d1, K.desc[2 * (size_t)j], K.desc[2 * (size_t)j + 1]);
        if (!((float)dist <= J.thr)) return;                        // :610 / :723
        uint32_t key = (uint32_t)dist << 20 | (uint32_t)f.npass;
        ++f.npass;
        int jj = j;
#pragma unroll
        for (int q = 0; q < kS3pKeep; ++q) {  // insertion into the sorted list (selects only)
            const bool lt = key < f.key[q];
            const uint32_t tk = f.key[q];
            const int tj = f.kp[q];
            f.key[q] = lt ? key : tk;
            f.kp[q] = lt ? jj : tj;
            key = lt ? tk : key;
            jj = lt ? tj : jj;
        }
    });
}

__global__ __launch_bounds__(kS3pThreads) void k_s3p_search(const S3pKf* __restrict__ kfs, const S3pJob* __restrict__ jobs,
                                                            const float* __restrict__ pos, const float* __restrict__ normal,
                                                            const float* __restrict__ min_dist,
                                                            const float* __restrict__ max_dist,
                                                            const uint4* __restrict__ mp_desc,
                                                            const uint8_t* __restrict__ skip, S3pPoint* __restrict__ pts,
                                                            int32_t* __restrict__ best_idx, int32_t* __restrict__ best_dist,
                                                            int32_t* __restrict__ nmatches) {
    __shared__ int32_t s_off[kCells + 1];
    __shared__ __attribute__((aligned(16))) float s_kp[4 * kS3pLdsRows];
    __shared__ int32_t s_idx[kS3pLdsRows];
    const S3pJob& J = jobs[blockIdx.y];
    if ((int)(blockIdx.x * kS3pThreads) >= J.count) return;  // block-uniform (the grid covers the longest job)
    const S3pKf& K = kfs[J.kf];
    const int p = blockIdx.x * kS3pThreads + threadIdx.x;
    const int nk = kf_count(K);
    const bool lds = nk <= kS3pLdsRows;  // block-uniform
    if (nk > 0) {
        for (int c = threadIdx.x; c <= kCells; c += kS3pThreads) s_off[c] = K.cell_off[c];
        if (lds)
            for (int j = threadIdx.x; j < nk; j += kS3pThreads) {
                const float4 kp = K.kp4[j];
                s_kp[4 * j] = kp.x;
                s_kp[4 * j + 1] = kp.y;
                s_kp[4 * j + 2] = kp.z;
                s_kp[4 * j + 3] = kp.w;
                s_idx[j] = K.cell_idx[j];  // (the list may be shorter than nk: keypoints outside the grid)
            }
        __syncthreads();
    }
    const bool active = p < J.count;
    const size_t o = (size_t)J.out_off + (active ? p : 0);
    S3pFound f;
#pragma unroll
    for (int q = 0; q < kS3pKeep; ++q) { f.key[q] = kNoCand; f.kp[q] = -1; }
    float u = 0.0f, v = 0.0f, radius = 0.0f;
    int level = 0;
    if (active && nk > 0 && !(skip && skip[o])) {                   // :526 (the caller's flags)
        const size_t i = (size_t)J.first + p;
        const float P[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const float Pn[3] = {normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
        if (s3p_gates(K, J, P, Pn, min_dist[i], max_dist[i], u, v, radius, level)) {
            const uint4 d0 = mp_desc[2 * i], d1 = mp_desc[2 * i + 1];
            if (lds)
                s3p_search_point(K, J, LdsF4{(const ORB_LDS float*)s_kp}, LdsArr<int32_t>{(const ORB_LDS int32_t*)s_off},
                                 LdsArr<int32_t>{(const ORB_LDS int32_t*)s_idx}, u, v, radius, level, d0, d1, f);
            else
                s3p_search_point(K, J, (const float4*)K.kp4, LdsArr<int32_t>{(const ORB_LDS int32_t*)s_off},
                                 (const int32_t*)K.cell_idx, u, v, radius, level, d0, d1, f);
        }
    }
    if (J.mode == ORB_S3P_FUSE) {
        const bool fused = active && f.bestDist <= kThLow;          // :1655
        if (active) {
            best_idx[o] = fused ? f.bestIdx : -1;
            if (best_dist) best_dist[o] = f.bestDist;
        }
        const int n = __popcll(__ballot(fused));
        if (n > 0 && (threadIdx.x & 63) == 0) atomicAdd(&nmatches[blockIdx.y], n);
        return;
    }
    if (!active) return;
    S3pPoint& Q = pts[o];
    Q.u = u;
    Q.v = v;
    Q.radius = radius;
    Q.level = level;
    Q.npass = f.npass;
#pragma unroll
    for (int q = 0; q < kS3pKeep; ++q)
        Q.keep[q] = f.kp[q] < 0 ? kNoCand : (uint32_t)f.kp[q] | (f.key[q] >> 20) << 16;
}

// Point i's answer given the claims of this round (keypoint | distance << 16, or -1): the first kept
// candidate no earlier point claims; when all of them are claimed and the window held more passing
// candidates, the window again (global records), claimed keypoints skipped.
__device__ __forceinline__ int s3p_answer(const S3pKf& K, const S3pJob& J, const S3pPoint& Q, const int32_t* claim, int i,
                                          const uint4* __restrict__ mp_desc) {
#pragma unroll
    for (int q = 0; q < kS3pKeep; ++q) {
        const uint32_t e = Q.keep[q];
        if (e == kNoCand) return -1;
        if (claim[e & 0xffffu] >= i) return (int)e;
    }
    if (Q.npass <= kS3pKeep) return -1;
    const size_t g = (size_t)J.first + i;
    const uint4 d0 = mp_desc[2 * g], d1 = mp_desc[2 * g + 1];
    int bestDist = 256, bestIdx = -1;
    s3p_window(K, (const float4*)K.kp4, (const int32_t*)K.cell_off, (const int32_t*)K.cell_idx, Q.u, Q.v, Q.radius, Q.level,
               [&](int j) {
                   if (claim[j] < i) return;                        // :589 / :704
                   const int dist = hamming(d0, d1, K.desc[2 * (size_t)j], K.desc[2 * (size_t)j + 1]);
                   if ((float)dist <= J.thr && dist < bestDist) {
                       bestDist = dist;
                       bestIdx = j;
                   }
               });
    return bestIdx < 0 ? -1 : bestIdx | bestDist << 16;
}

__global__ __launch_bounds__(kResolveThreads) void k_s3p_resolve(const S3pKf* __restrict__ kfs,
                                                                 const S3pJob* __restrict__ jobs,
                                                                 const uint4* __restrict__ mp_desc,
                                                                 const uint8_t* __restrict__ taken0, int stride,
                                                                 const S3pPoint* __restrict__ pts, int32_t* matched,
                                                                 int32_t* __restrict__ nmatches, int32_t* best_idx,
                                                                 int32_t* __restrict__ best_dist) {
    __shared__ int32_t s_claim[kClaimLds];
    __shared__ int s_count;
    const S3pJob& J = jobs[blockIdx.x];
    if (J.mode == ORB_S3P_FUSE) return;
    const S3pKf& K = kfs[J.kf];
    const int nk = kf_count(K), n = J.count, tid = threadIdx.x;
    int32_t* const row = matched + (size_t)blockIdx.x * stride;
    int32_t* const claim = nk <= kClaimLds ? s_claim : row;         // (stride >= cap >= nk)
    const uint8_t* const tk = taken0 ? taken0 + (size_t)blockIdx.x * stride : nullptr;
    const S3pPoint* const Q = pts + J.out_off;
    int32_t* const st = best_idx + J.out_off;                       // the current answers, packed
    for (int i = tid; i < n; i += kResolveThreads) st[i] = -1;
    if (tid == 0) s_count = 0;
    for (;;) {
        for (int j = tid; j < nk; j += kResolveThreads) claim[j] = tk && tk[j] ? -1 : INT_MAX;
        __syncthreads();
        for (int i = tid; i < n; i += kResolveThreads) {
            const int s = st[i];
            if (s >= 0) atomicMin(&claim[s & 0xffff], i);
        }
        __syncthreads();
        int changed = 0;
        for (int i = tid; i < n; i += kResolveThreads) {
            if (Q[i].npass == 0) continue;
            const int s = s3p_answer(K, J, Q[i], claim, i, mp_desc);
            if (s != st[i]) {
                st[i] = s;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // the claims of the last round are those of the final answers
    for (int j = tid; j < stride; j += kResolveThreads) {
        const int c = j < nk ? claim[j] : -1;
        row[j] = c == INT_MAX ? -1 : c;
    }
    int mine = 0;
    for (int i = tid; i < n; i += kResolveThreads) {
        const int s = st[i];
        st[i] = s < 0 ? -1 : s & 0xffff;
        if (best_dist) best_dist[J.out_off + i] = s < 0 ? 256 : s >> 16;
        mine += s >= 0;
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0) nmatches[blockIdx.x] = s_count;
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// per-keyframe scratch: kp4 | cell_off | cell_idx | cell_of | misc
struct KfScratch {
    size_t kp4, off, idx, of, misc, end;
};
KfScratch kf_scratch(size_t base, int cap) {
    KfScratch s;
    s.kp4 = base;
    s.off = align256(s.kp4 + 16 * (size_t)cap);
    s.idx = align256(s.off + 4 * (size_t)(kCells + 1));
    s.of = align256(s.idx + 4 * (size_t)cap);
    s.misc = align256(s.of + 4 * (size_t)cap);
    s.end = align256(s.misc + 32);
    return s;
}

// One call, checked: the keyframe and job records (scratch pointers unset), the totals.
struct S3pPlan {
    std::vector<S3pKf> kfs;
    std::vector<S3pJob> jobs;
    size_t total = 0;      // the sum of the jobs' point counts
    int max_count = 0;
    bool any_claim = false;
    size_t o_jobs = 0, args_bytes = 0, o_pts = 0, scratch_bytes = 0;
};

int s3p_fail(const char* what) { return orbgpu_fail(ORB_ERR_ARG, what); }

// Argument checks shared by both entries; kfs as device views (the host entry passes views over its staging
// area, whose pointers are not read here).
int s3p_plan(const orb_sim3_projection_kf_device_t* kfs, int n_kfs, const orb_sim3_projection_job_t* jobs, int n_jobs,
             int pool_n, int stride, S3pPlan& pl) {
    pl.kfs.resize(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_device_t& f = kfs[k].frame;
        S3pKf& o = pl.kfs[k];
        memset(&o, 0, sizeof(o));
        if (f.cap <= 0 || f.cap > kS3pMaxCap || f.cap > stride)
            return orbgpu_fail(ORB_ERR_CAPACITY, "Sim3 projection: keyframe capacity outside 1 .. min(16384, stride)");
        if (!f.scale_factors || f.nlevels < 1 || f.nlevels > kS3pMaxLevels ||
            !orbgpu::predict_scale_thresholds(kfs[k].log_scale_factor, f.nlevels, o.steps))
            return s3p_fail("Sim3 projection: invalid keyframe view (nlevels <= 12, log scale factor > 0)");
        o.kps = f.kps_un;
        o.n_raw = f.n;
        o.desc = reinterpret_cast<const uint4*>(f.desc);
        o.cap = f.cap;
        o.nlevels = f.nlevels;
        o.min_x = f.min_x; o.max_x = f.max_x; o.min_y = f.min_y; o.max_y = f.max_y;
        o.inv_w = f.grid_inv_w; o.inv_h = f.grid_inv_h;
        o.fx = f.fx; o.fy = f.fy; o.cx = f.cx; o.cy = f.cy;
        for (int l = 0; l < f.nlevels; ++l) o.scale[l] = f.scale_factors[l];
    }
    pl.jobs.resize(n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const orb_sim3_projection_job_t& a = jobs[j];
        S3pJob& o = pl.jobs[j];
        memset(&o, 0, sizeof(o));
        if (a.kf < 0 || a.kf >= n_kfs) return s3p_fail("Sim3 projection: job keyframe index out of range");
        if (a.first < 0 || a.count < 0 || a.first > pool_n || a.count > pool_n - a.first)
            return s3p_fail("Sim3 projection: job point range outside the pool");
        if (a.mode != ORB_S3P_CLAIM_PROJECT && a.mode != ORB_S3P_CLAIM_INVZ && a.mode != ORB_S3P_FUSE)
            return s3p_fail("Sim3 projection: unknown job mode");
        if (!(a.th > 0.0f) || !std::isfinite(a.th)) return s3p_fail("Sim3 projection: th must be positive and finite");
        o.thr = (float)kThLow * a.ratio_hamming;
        // (a threshold of 256 or more would let the reference write vpMatched[-1])
        if (a.mode != ORB_S3P_FUSE && !(a.ratio_hamming > 0.0f && o.thr < 256.0f))
            return s3p_fail("Sim3 projection: ratioHamming must be positive with 50 * ratioHamming < 256");
        if (pl.total + (size_t)a.count > (size_t)kS3pMaxJobPoints)
            return orbgpu_fail(ORB_ERR_CAPACITY, "Sim3 projection: more than 2^24 points over all jobs");
        o.kf = a.kf; o.first = a.first; o.count = a.count; o.mode = a.mode;
        o.out_off = (int)pl.total;
        o.th = a.th;
        memcpy(o.Tcw, a.Tcw, sizeof(o.Tcw));
        memcpy(o.Ow, a.Ow, sizeof(o.Ow));
        pl.total += (size_t)a.count;
        pl.max_count = std::max(pl.max_count, a.count);
        pl.any_claim |= a.mode != ORB_S3P_FUSE;
    }
    // device-only area: keyframe records | job records || per-point scratch | keyframe scratch
    pl.o_jobs = align256(sizeof(S3pKf) * (size_t)n_kfs);
    pl.args_bytes = align256(pl.o_jobs + sizeof(S3pJob) * (size_t)n_jobs);
    pl.o_pts = 0;
    size_t off = align256(sizeof(S3pPoint) * (pl.any_claim ? pl.total : 0));
    for (const S3pKf& k : pl.kfs) off = kf_scratch(off, k.cap).end;
    pl.scratch_bytes = off;
    return ORB_OK;
}

// The launches of one call (their number does not depend on the job count).  d_args / d_scratch: device
// areas of pl.args_bytes / pl.scratch_bytes; h_args: staging of the former.
int s3p_launch(S3pPlan& pl, char* h_args, char* d_args, char* d_scratch, const orb_fuse_points_device_t& pool,
               const uint8_t* d_skip, const uint8_t* d_taken0, int stride, int32_t* d_matched, int32_t* d_nmatches,
               int32_t* d_best_idx, int32_t* d_best_dist, hipStream_t s) {
    const int K = (int)pl.kfs.size(), B = (int)pl.jobs.size();
    size_t off = align256(sizeof(S3pPoint) * (pl.any_claim ? pl.total : 0));
    for (S3pKf& k : pl.kfs) {
        const KfScratch sc = kf_scratch(off, k.cap);
        k.kp4 = reinterpret_cast<float4*>(d_scratch + sc.kp4);
        k.cell_off = reinterpret_cast<int32_t*>(d_scratch + sc.off);
        k.cell_idx = reinterpret_cast<int32_t*>(d_scratch + sc.idx);
        k.cell_of = reinterpret_cast<int32_t*>(d_scratch + sc.of);
        k.misc = reinterpret_cast<int32_t*>(d_scratch + sc.misc);
        off = sc.end;
    }
    memcpy(h_args, pl.kfs.data(), sizeof(S3pKf) * (size_t)K);
    memcpy(h_args + pl.o_jobs, pl.jobs.data(), sizeof(S3pJob) * (size_t)B);
    if (hipMemcpyAsync(d_args, h_args, pl.args_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_matched, 0xFF, 4 * (size_t)B * stride, s) != hipSuccess ||
        hipMemsetAsync(d_nmatches, 0, 4 * (size_t)B, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Sim3 projection: argument upload failed");
    const S3pKf* dk = reinterpret_cast<const S3pKf*>(d_args);
    const S3pJob* dj = reinterpret_cast<const S3pJob*>(d_args + pl.o_jobs);
    S3pPoint* dp = reinterpret_cast<S3pPoint*>(d_scratch + pl.o_pts);
    const uint4* desc = reinterpret_cast<const uint4*>(pool.desc);
    if (pl.max_count > 0) {
        hipLaunchKernelGGL(k_s3p_grid, dim3(1, K), dim3(kPrepThreads), 0, s, dk);
        hipLaunchKernelGGL(k_s3p_search, dim3((pl.max_count + kS3pThreads - 1) / kS3pThreads, B), dim3(kS3pThreads), 0, s, dk,
                           dj, pool.pos, pool.normal, pool.min_dist, pool.max_dist, desc, d_skip, dp, d_best_idx, d_best_dist,
                           d_nmatches);
        if (pl.any_claim)
            hipLaunchKernelGGL(k_s3p_resolve, dim3(B), dim3(kResolveThreads), 0, s, dk, dj, desc, d_taken0, stride, dp,
                               d_matched, d_nmatches, d_best_idx, d_best_dist);
    }
    return hipGetLastError() == hipSuccess ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "Sim3 projection: kernel launch failed");
}

bool pool_ok(int n, const void* pos, const void* normal, const void* mn, const void* mx, const void* desc) {
    return n >= 0 && n <= kS3pMaxPool && (n == 0 || (pos && normal && mn && mx && desc));
}

int counts_ok(int n_kfs, const void* kfs, int n_jobs, const void* jobs) {
    if (n_kfs < 0 || n_jobs < 0 || (n_kfs > 0 && !kfs) || (n_jobs > 0 && !jobs)) return s3p_fail("bad Sim3 projection arguments");
    if (n_kfs > kS3pMaxKfs || n_jobs > kS3pMaxJobs)
        return orbgpu_fail(ORB_ERR_CAPACITY, "Sim3 projection: more than 65535 jobs or 1024 keyframes");
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_sim3_projection_device(orb_matcher_t m, const orb_sim3_projection_kf_device_t* kfs, int n_kfs,
                               const orb_sim3_projection_job_t* jobs, int n_jobs, const orb_fuse_points_device_t* pool,
                               const uint8_t* d_skip, const uint8_t* d_taken0, int stride, int32_t* d_matched,
                               int32_t* d_nmatches, int32_t* d_best_idx, int32_t* d_best_dist, void* stream) {
    if (!m || !pool || !pool_ok(pool->n, pool->pos, pool->normal, pool->min_dist, pool->max_dist, pool->desc))
        return s3p_fail("bad Sim3 projection arguments");
    if (int rc = counts_ok(n_kfs, kfs, n_jobs, jobs)) return rc;
    if (n_jobs == 0) return ORB_OK;
    if (stride <= 0 || !d_matched || !d_nmatches || !d_best_idx) return s3p_fail("Sim3 projection: null output or stride <= 0");
    for (int k = 0; k < n_kfs; ++k)
        if (!kfs[k].frame.kps_un || !kfs[k].frame.desc || !kfs[k].frame.n ||
            (reinterpret_cast<uintptr_t>(kfs[k].frame.desc) & 15) != 0)
            return s3p_fail("Sim3 projection: null or unaligned keyframe arrays");
    if (pool->n > 0 && (reinterpret_cast<uintptr_t>(pool->desc) & 15) != 0)
        return s3p_fail("Sim3 projection: unaligned point descriptors");
    S3pPlan pl;
    if (int rc = s3p_plan(kfs, n_kfs, jobs, n_jobs, pool->n, stride, pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* h = nullptr;
    if (int rc = orbgpu_matcher_upload_slot(m, pl.args_bytes, &h)) return rc;
    char* d = nullptr;  // stream-ordered (calls on different streams do not share it)
    if (hipMallocAsync(reinterpret_cast<void**>(&d), pl.args_bytes + pl.scratch_bytes, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    int rc = s3p_launch(pl, h, d, d + pl.args_bytes, *pool, d_skip, d_taken0, stride, d_matched, d_nmatches, d_best_idx,
                        d_best_dist, s);
    if (orbgpu_matcher_upload_mark(m, s) != ORB_OK && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "event record failed");
    if (hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    return rc;
}

int orb_sim3_projection(orb_matcher_t m, const orb_sim3_projection_kf_t* kfs, int n_kfs,
                        const orb_sim3_projection_job_t* jobs, int n_jobs, const orb_fuse_points_t* pool,
                        const uint8_t* skip, const uint8_t* taken0, int stride, int32_t* matched, int32_t* nmatches,
                        int32_t* best_idx, int32_t* best_dist) {
    if (!m || !pool || !pool_ok(pool->n, pool->pos, pool->normal, pool->min_dist, pool->max_dist, pool->desc))
        return s3p_fail("bad Sim3 projection arguments");
    if (int rc = counts_ok(n_kfs, kfs, n_jobs, jobs)) return rc;
    if (n_jobs == 0) return ORB_OK;
    if (stride <= 0 || !matched || !nmatches || !best_idx) return s3p_fail("Sim3 projection: null output or stride <= 0");
    // every argument is checked before the handle's staging is touched
    std::vector<orb_sim3_projection_kf_device_t> dk(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_view_t& f = kfs[k].frame;
        if (f.n < 0 || f.n > kS3pMaxCap || f.n > stride)
            return orbgpu_fail(ORB_ERR_CAPACITY, "Sim3 projection: keyframe count outside 0 .. min(16384, stride)");
        if (f.n > 0 && (!f.kps_un || !f.desc)) return s3p_fail("Sim3 projection: null keyframe arrays");
        orb_frame_device_t& g = dk[k].frame;
        memset(&dk[k], 0, sizeof(dk[k]));
        g.cap = std::max(f.n, 1);
        g.min_x = f.min_x; g.max_x = f.max_x; g.min_y = f.min_y; g.max_y = f.max_y;
        g.grid_inv_w = f.grid_inv_w; g.grid_inv_h = f.grid_inv_h;
        g.fx = f.fx; g.fy = f.fy; g.cx = f.cx; g.cy = f.cy;
        g.nlevels = f.nlevels;
        g.scale_factors = f.scale_factors;
        dk[k].log_scale_factor = kfs[k].log_scale_factor;
    }
    S3pPlan pl;
    if (int rc = s3p_plan(dk.data(), n_kfs, jobs, n_jobs, pool->n, stride, pl)) return rc;
    // packed layout, one upload: per keyframe count | kps | desc; the pool; the skip and taken0 flags; then
    // the device-only argument records, the outputs and the scratch
    struct Off { size_t cnt, kps, desc; };
    std::vector<Off> offs(n_kfs);
    size_t off = 0;
    for (int k = 0; k < n_kfs; ++k) {
        const size_t cap = (size_t)dk[k].frame.cap;
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 4);
        o.kps = off; off = align256(off + cap * sizeof(orb_keypoint_t));
        o.desc = off; off = align256(off + cap * 32);
    }
    const size_t N = (size_t)pool->n, T = pl.total, BS = (size_t)n_jobs * (size_t)stride;
    const size_t o_pos = off; off = align256(off + 12 * N);
    const size_t o_nrm = off; off = align256(off + 12 * N);
    const size_t o_min = off; off = align256(off + 4 * N);
    const size_t o_max = off; off = align256(off + 4 * N);
    const size_t o_dsc = off; off = align256(off + 32 * N);
    const size_t o_skip = off; off = align256(off + (skip ? T : 0));
    const size_t o_tk = off; off = align256(off + (taken0 ? BS : 0));
    const size_t in_bytes = off;
    const size_t o_args = off; off += pl.args_bytes;
    const size_t o_mat = off; off = align256(off + 4 * BS);
    const size_t o_cnt = off; off = align256(off + 4 * (size_t)n_jobs);
    const size_t o_idx = off; off = align256(off + 4 * T);
    const size_t o_dist = off; off = align256(off + 4 * T);
    const size_t o_scratch = off;
    const size_t total = off + pl.scratch_bytes;

    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int rc = orbgpu_matcher_reserve(m, total, &d, &h, &s, &check_ori)) return rc;
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_view_t& f = kfs[k].frame;
        const Off& o = offs[k];
        S3pKf& r = pl.kfs[k];
        r.kps = reinterpret_cast<const orb_keypoint_t*>(d + o.kps);
        r.desc = reinterpret_cast<const uint4*>(d + o.desc);
        r.n_raw = reinterpret_cast<const int32_t*>(d + o.cnt);
        *reinterpret_cast<int32_t*>(h + o.cnt) = f.n;
        if (f.n) {
            memcpy(h + o.kps, f.kps_un, (size_t)f.n * sizeof(orb_keypoint_t));
            memcpy(h + o.desc, f.desc, (size_t)f.n * 32);
        }
    }
    if (N) {
        memcpy(h + o_pos, pool->pos, 12 * N);
        memcpy(h + o_nrm, pool->normal, 12 * N);
        memcpy(h + o_min, pool->min_dist, 4 * N);
        memcpy(h + o_max, pool->max_dist, 4 * N);
        memcpy(h + o_dsc, pool->desc, 32 * N);
    }
    if (skip && T) memcpy(h + o_skip, skip, T);
    if (taken0) memcpy(h + o_tk, taken0, BS);
    if (hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Sim3 projection: upload failed");
    const orb_fuse_points_device_t dp{pool->n, reinterpret_cast<const float*>(d + o_pos),
                                      reinterpret_cast<const float*>(d + o_nrm), reinterpret_cast<const float*>(d + o_min),
                                      reinterpret_cast<const float*>(d + o_max), reinterpret_cast<const uint8_t*>(d + o_dsc)};
    // (a job without points is never written by a kernel: its points' outputs do not exist)
    if (int rc = s3p_launch(pl, h + o_args, d + o_args, d + o_scratch, dp,
                            skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr,
                            taken0 ? reinterpret_cast<const uint8_t*>(d + o_tk) : nullptr, stride,
                            reinterpret_cast<int32_t*>(d + o_mat), reinterpret_cast<int32_t*>(d + o_cnt),
                            reinterpret_cast<int32_t*>(d + o_idx), reinterpret_cast<int32_t*>(d + o_dist), s))
        return rc;
    if (hipMemcpyAsync(h + o_mat, d + o_mat, o_scratch - o_mat, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Sim3 projection: device error");
    memcpy(matched, h + o_mat, 4 * BS);
    memcpy(nmatches, h + o_cnt, 4 * (size_t)n_jobs);
    if (T) {
        memcpy(best_idx, h + o_idx, 4 * T);
        if (best_dist) memcpy(best_dist, h + o_dist, 4 * T);
    }
    return ORB_OK;
}

}  // extern "C"
