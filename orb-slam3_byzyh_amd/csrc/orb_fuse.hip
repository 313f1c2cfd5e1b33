// ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) on MI355X: the search half (steps 1-6,
// reference src/ORBmatcher.cc:1356-1506; KeyFrame::GetFeaturesInArea / IsInImage src/KeyFrame.cc:843-897;
// MapPoint::PredictScale src/MapPoint.cc:688-706), batched over the target keyframes of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:917-1066).  Step 7 (the map mutation) stays with
// the caller (include/orbgpu_matcher.hpp).
//
// Inside one Fuse call the search of a point depends on nothing an earlier point did to the map, so a
// job (keyframe k, point i) is independent of every other:
//   k_fuse_grid    one workgroup per keyframe: KeyFrame::mGrid and the packed (x, y, angle, octave) rows,
//                  built on the device (k_frame_prep_body of orb_frame_grid.h)
//   k_fuse_search  blockIdx.y = keyframe, one thread per point, 256 points per block.  The block stages
//                  the keyframe's 3,073 cell offsets and, when the keyframe has at most kFuseLdsRows
//                  keypoints, its keypoint records (x, y, octave | u_R | cell index list: 24 B each) in
//                  LDS; the point's descriptor sits in registers; a keyframe descriptor is read (from
//                  global memory) only for a keypoint that passed the level and chi-square gates.  A
//                  larger keyframe leaves the records in global memory (the same walk, the same results).
//
// Float arithmetic as the reference build (g++ -O3 -march=native) contracts it -- the rule is written
// down in oracle/orb_frustum_oracle.cpp and oracle/orb_projection_oracle.cpp: `a*b + c*d` becomes
// fma(a, b, c*d), `a - b*c` becomes fma(-b, c, a).  This file is compiled with -ffp-contract=off and every
// fma is explicit:
//   Pc[r]  = fma(R[r][2], P[2], fma(R[r][0], P[0], R[r][1] * P[1])) + t[r]
//   invz   = 1 / Pc[2];   u = fx * Pc[0] / Pc[2] + cx;   v = fy * Pc[1] / Pc[2] + cy
//   ur     = fma(-bf, invz, u)
//   dot3   = fma(a[2], b[2], fma(a[0], b[0], a[1] * b[1]))      (|PO|^2 and PO . normal)
//   e2     = fma(ex, ex, ey * ey)                               (mvuRight[idx] < 0:  `ex*ex+ey*ey`)
//   e2     = fma(er, er, fma(ex, ex, ey * ey))                  (mvuRight[idx] >= 0: `ex*ex+ey*ey+er*er`)
//   the gate: (double)(e2 * mvInvLevelSigma2[octave]) > 5.99 / 7.8 -- the float product widened and
//   compared with the double literal, as upstream's `e2*...>7.8` does.
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr int kThLow = 50;             // src/ORBmatcher.cc:37
constexpr int kFuseMaxLevels = 12;
constexpr int kFuseThreads = 256;
constexpr int kFuseLdsRows = 2048;     // keypoint records staged in LDS: 24 B each + the cell offsets = 61,444 B
constexpr int kFuseMaxCap = 16384;     // k_frame_prep_body's limit
constexpr int kFuseMaxPoints = 1 << 20;

// one keyframe as the kernels read it (an array of these in device memory, one per keyframe)
struct FuseKf {
    const orb_keypoint_t* kps;   // mvKeysUn (cap)
    const int32_t* n_raw;        // KeyFrame::N as its producer left it
    const uint4* desc;           // mDescriptors
    const float* ur;             // mvuRight or null
    float4* kp4;                 // scratch: x, y, angle, octave bits
    int32_t* cell_off;           // scratch: kCells + 1
    int32_t* cell_idx;           // scratch: cap
    int32_t* cell_of;            // scratch: cap
    int32_t* misc;               // scratch: [0] the clamped count, [4..7] k_frame_prep_body's zero words
    int cap, nlevels;
    float Tcw[12], Ow[3];
    float min_x, max_x, min_y, max_y, inv_w, inv_h, fx, fy, cx, cy, bf;
    float scale[kFuseMaxLevels], inv_sigma2[kFuseMaxLevels];
    float steps[kFuseMaxLevels];  // MapPoint::PredictScale level thresholds (orb_predict_scale.h)
};

__global__ __launch_bounds__(kPrepThreads) void k_fuse_grid(const FuseKf* __restrict__ kfs) {
    const FuseKf& K = kfs[blockIdx.y];
    k_frame_prep_body(K.kps, K.n_raw, K.cap, K.min_x, K.min_y, K.inv_w, K.inv_h, K.kp4, K.cell_off, K.cell_idx, K.cell_of,
                      K.misc, nullptr, ScratchInit{nullptr, 0, nullptr, 0, K.misc + 4, nullptr, -1});
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return fmaf(a[2], b[2], fmaf(a[0], b[0], a[1] * b[1]));
}

// steps 5-6 for one point (src:1432-1501): the window walk in GetFeaturesInArea's order, the gates, the
// first Hamming minimum.  KP / UR / CO / CI: the keyframe's records, global pointers or LDS readers.
template <class KP, class UR, class CO, class CI>
__device__ __forceinline__ void fuse_window(const FuseKf& K, KP kp4, UR ur_arr, bool has_ur, CO cell_off, CI cell_idx,
                                            float u, float v, float ur, float radius, int level, const uint4 d0,
                                            const uint4 d1, int& bestDist, int& bestIdx) {
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
            const float ex = u - kp.x, ey = v - kp.y;
            if (!(fabsf(ex) < radius && fabsf(ey) < radius)) continue;  // GetFeaturesInArea (KeyFrame.cc:884)
            const int oct = __float_as_int(kp.w);
            if (oct < level - 1 || oct > level || oct < 0) continue;    // src:1455
            const float kpr = has_ur ? ur_arr[j] : -1.0f;
            float e2 = fmaf(ex, ex, ey * ey);
            double limit = 5.99;                                        // src:1486
            if (kpr >= 0) {                                             // src:1459-1474
                const float er = ur - kpr;
                e2 = fmaf(er, er, e2);
                limit = 7.8;
            }
            if ((double)(e2 * K.inv_sigma2[oct]) > limit) continue;
            const int dist = hamming(d0, d1, K.desc[2 * (size_t)j], K.desc[2 * (size_t)j + 1]);
            if (dist < bestDist) {                                      // src:1496-1500
                bestDist = dist;
                bestIdx = j;
            }
        }
    }
}

__global__ __launch_bounds__(kFuseThreads) void k_fuse_search(const FuseKf* __restrict__ kfs, int n,
                                                              const float* __restrict__ pos,
                                                              const float* __restrict__ normal,
                                                              const float* __restrict__ min_dist,
                                                              const float* __restrict__ max_dist,
                                                              const uint4* __restrict__ mp_desc,
                                                              const uint8_t* __restrict__ skip, float th,
                                                              int32_t* __restrict__ best_idx,
                                                              int32_t* __restrict__ best_dist) {
    __shared__ int32_t s_off[kCells + 1];
    __shared__ __attribute__((aligned(16))) float s_kp[4 * kFuseLdsRows];
    __shared__ float s_ur[kFuseLdsRows];
    __shared__ int32_t s_idx[kFuseLdsRows];
    const FuseKf& K = kfs[blockIdx.y];
    const int i = blockIdx.x * kFuseThreads + threadIdx.x;
    const size_t job = (size_t)blockIdx.y * n + i;
    const int raw = *K.n_raw;
    const bool flagged = raw < 0 || raw > K.cap;  // no matches for this keyframe
    const int nk = flagged ? 0 : raw;
    const bool lds = nk <= kFuseLdsRows;          // block-uniform
    const bool has_ur = K.ur != nullptr;
    if (nk > 0) {
        for (int c = threadIdx.x; c <= kCells; c += kFuseThreads) s_off[c] = K.cell_off[c];
        if (lds)
            for (int j = threadIdx.x; j < nk; j += kFuseThreads) {
                const float4 kp = K.kp4[j];
                s_kp[4 * j] = kp.x;
                s_kp[4 * j + 1] = kp.y;
                s_kp[4 * j + 2] = kp.z;
                s_kp[4 * j + 3] = kp.w;
                s_idx[j] = K.cell_idx[j];  // (the list may be shorter than nk: keypoints outside the grid)
                if (has_ur) s_ur[j] = K.ur[j];
            }
        __syncthreads();
    }
    if (i >= n) return;
    int bestDist = 256, bestIdx = -1;
    do {
        if (nk == 0 || (skip && skip[job])) break;                  // src:1359-1376 (the caller's flags)
        const float P[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
        float Pc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            Pc[r] = fmaf(K.Tcw[4 * r + 2], P[2], fmaf(K.Tcw[4 * r], P[0], K.Tcw[4 * r + 1] * P[1])) + K.Tcw[4 * r + 3];
        if (Pc[2] < 0.0f) break;                                    // src:1384
        const float invz = 1.0f / Pc[2];
        const float u = K.fx * Pc[0] / Pc[2] + K.cx;                // Pinhole::project(Eigen::Vector3f)
        const float v = K.fy * Pc[1] / Pc[2] + K.cy;
        if (!(u >= K.min_x && u < K.max_x && v >= K.min_y && v < K.max_y)) break;  // KeyFrame::IsInImage
        const float ur = fmaf(-K.bf, invz, u);
        const float PO[3] = {P[0] - K.Ow[0], P[1] - K.Ow[1], P[2] - K.Ow[2]};
        const float dist3D = sqrtf(dot3(PO, PO));
        const float maxd = max_dist[i];
        if (dist3D < 0.8f * min_dist[i] || dist3D > 1.2f * maxd) break;         // src:1411
        const float Pn[3] = {normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2]};
        if (dot3(PO, Pn) < 0.5f * dist3D) break;                    // src:1420 (0.5 * dist3D is exact in double too)
        const int level = orbgpu::predict_scale_level(maxd / dist3D, K.steps, K.nlevels);
        const float radius = th * K.scale[level];
        const uint4 d0 = mp_desc[2 * (size_t)i], d1 = mp_desc[2 * (size_t)i + 1];
        if (lds)
            fuse_window(K, LdsF4{(const ORB_LDS float*)s_kp}, LdsArr<float>{(const ORB_LDS float*)s_ur}, has_ur,
                        LdsArr<int32_t>{(const ORB_LDS int32_t*)s_off}, LdsArr<int32_t>{(const ORB_LDS int32_t*)s_idx}, u, v,
                        ur, radius, level, d0, d1, bestDist, bestIdx);
        else
            fuse_window(K, (const float4*)K.kp4, K.ur, has_ur, LdsArr<int32_t>{(const ORB_LDS int32_t*)s_off},
                        (const int32_t*)K.cell_idx, u, v, ur, radius, level, d0, d1, bestDist, bestIdx);
    } while (false);
    best_idx[job] = bestDist <= kThLow ? bestIdx : -1;              // src:1506
    if (best_dist) best_dist[job] = bestDist;
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

bool th_ok(float th) { return th > 0.0f && std::isfinite(th); }

// the host-side fields of a keyframe view (both entries); steps receives PredictScale's thresholds
bool levels_ok(int nlevels, const float* scale_factors, const float* inv_sigma2, float lsf, float* steps) {
    if (!scale_factors || !inv_sigma2 || nlevels < 1 || nlevels > kFuseMaxLevels) return false;
    return orbgpu::predict_scale_thresholds(lsf, nlevels, steps);
}

bool frame_ok(const orb_frame_device_t& f, const float* inv_sigma2, float lsf, float* steps) {
    if (f.cap <= 0 || f.cap > kFuseMaxCap || !f.kps_un || !f.desc || !f.n) return false;
    if ((reinterpret_cast<uintptr_t>(f.desc) & 15) != 0) return false;
    return levels_ok(f.nlevels, f.scale_factors, inv_sigma2, lsf, steps);
}

// The launches of one call: `kfs` on the host with the scratch pointers unset; d_args / d_scratch device
// areas of args_bytes(n_kfs) / scratch_bytes(kfs) bytes; h_args pinned (or pageable) staging of the former.
size_t fuse_args_bytes(int n_kfs) { return align256(sizeof(FuseKf) * (size_t)n_kfs); }

int fuse_launch(std::vector<FuseKf>& kfs, char* h_args, char* d_args, char* d_scratch, const orb_fuse_points_device_t& pts,
                const uint8_t* d_skip, float th, int32_t* d_best_idx, int32_t* d_best_dist, hipStream_t s) {
    const int K = (int)kfs.size();
    size_t off = 0;
    for (FuseKf& k : kfs) {
        const KfScratch sc = kf_scratch(off, k.cap);
        k.kp4 = reinterpret_cast<float4*>(d_scratch + sc.kp4);
        k.cell_off = reinterpret_cast<int32_t*>(d_scratch + sc.off);
        k.cell_idx = reinterpret_cast<int32_t*>(d_scratch + sc.idx);
        k.cell_of = reinterpret_cast<int32_t*>(d_scratch + sc.of);
        k.misc = reinterpret_cast<int32_t*>(d_scratch + sc.misc);
        off = sc.end;
    }
    memcpy(h_args, kfs.data(), sizeof(FuseKf) * (size_t)K);
    if (hipMemcpyAsync(d_args, h_args, sizeof(FuseKf) * (size_t)K, hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Fuse argument upload failed");
    hipLaunchKernelGGL(k_fuse_grid, dim3(1, K), dim3(kPrepThreads), 0, s, reinterpret_cast<const FuseKf*>(d_args));
    hipLaunchKernelGGL(k_fuse_search, dim3((pts.n + kFuseThreads - 1) / kFuseThreads, K), dim3(kFuseThreads), 0, s,
                       reinterpret_cast<const FuseKf*>(d_args), pts.n, pts.pos, pts.normal, pts.min_dist, pts.max_dist,
                       reinterpret_cast<const uint4*>(pts.desc), d_skip, th, d_best_idx, d_best_dist);
    return hipGetLastError() == hipSuccess ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "Fuse kernel launch failed");
}

size_t fuse_scratch_bytes(const std::vector<FuseKf>& kfs) {
    size_t off = 0;
    for (const FuseKf& k : kfs) off = kf_scratch(off, k.cap).end;
    return off;
}

// argument checks shared by both entries and the FuseKf records (scratch pointers unset)
int fuse_prepare(const orb_fuse_kf_device_t* kfs, int n_kfs, float th, std::vector<FuseKf>& out) {
    if (!th_ok(th)) return orbgpu_fail(ORB_ERR_ARG, "Fuse: th must be positive and finite");
    out.resize(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_device_t& f = kfs[k].frame;
        FuseKf& o = out[k];
        memset(&o, 0, sizeof(o));
        if (!frame_ok(f, kfs[k].inv_level_sigma2, kfs[k].log_scale_factor, o.steps))
            return orbgpu_fail(ORB_ERR_ARG, "Fuse: invalid keyframe view (cap <= 16384, nlevels <= 12, log scale factor > 0)");
        o.kps = f.kps_un;
        o.n_raw = f.n;
        o.desc = reinterpret_cast<const uint4*>(f.desc);
        o.ur = f.u_right;
        o.cap = f.cap;
        o.nlevels = f.nlevels;
        memcpy(o.Tcw, f.Tcw, sizeof(o.Tcw));
        memcpy(o.Ow, kfs[k].Ow, sizeof(o.Ow));
        o.min_x = f.min_x; o.max_x = f.max_x; o.min_y = f.min_y; o.max_y = f.max_y;
        o.inv_w = f.grid_inv_w; o.inv_h = f.grid_inv_h;
        o.fx = f.fx; o.fy = f.fy; o.cx = f.cx; o.cy = f.cy; o.bf = f.bf;
        for (int l = 0; l < f.nlevels; ++l) {
            o.scale[l] = f.scale_factors[l];
            o.inv_sigma2[l] = kfs[k].inv_level_sigma2[l];
        }
    }
    return ORB_OK;
}

bool points_ok(int n, const void* pos, const void* normal, const void* mn, const void* mx, const void* desc) {
    return n >= 0 && n <= kFuseMaxPoints && (n == 0 || (pos && normal && mn && mx && desc));
}

}  // namespace

extern "C" {

int orb_fuse_device(orb_matcher_t m, const orb_fuse_kf_device_t* kfs, int n_kfs, const orb_fuse_points_device_t* points,
                    const uint8_t* d_skip, float th, int32_t* d_best_idx, int32_t* d_best_dist, void* stream) {
    if (!m || !points || n_kfs < 0 || n_kfs > 65535 || (n_kfs > 0 && !kfs) ||
        !points_ok(points->n, points->pos, points->normal, points->min_dist, points->max_dist, points->desc))
        return orbgpu_fail(ORB_ERR_ARG, "bad Fuse arguments");
    if (points->n == 0 || n_kfs == 0) return ORB_OK;
    if (!d_best_idx || (reinterpret_cast<uintptr_t>(points->desc) & 15) != 0)
        return orbgpu_fail(ORB_ERR_ARG, "Fuse: null output or unaligned point descriptors");
    std::vector<FuseKf> recs;
    if (int rc = fuse_prepare(kfs, n_kfs, th, recs)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t abytes = fuse_args_bytes(n_kfs), sbytes = fuse_scratch_bytes(recs);
    char* h = nullptr;
    if (int rc = orbgpu_matcher_upload_slot(m, abytes, &h)) return rc;
    char* d = nullptr;  // stream-ordered (calls on different streams do not share it)
    if (hipMallocAsync(reinterpret_cast<void**>(&d), abytes + sbytes, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    int rc = fuse_launch(recs, h, d, d + abytes, *points, d_skip, th, d_best_idx, d_best_dist, s);
    if (orbgpu_matcher_upload_mark(m, s) != ORB_OK && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "event record failed");
    if (hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    return rc;
}

int orb_fuse(orb_matcher_t m, const orb_fuse_kf_t* kfs, int n_kfs, const orb_fuse_points_t* points, const uint8_t* skip,
             float th, int32_t* best_idx, int32_t* best_dist) {
    if (!m || !points || n_kfs < 0 || n_kfs > 65535 || (n_kfs > 0 && !kfs) ||
        !points_ok(points->n, points->pos, points->normal, points->min_dist, points->max_dist, points->desc))
        return orbgpu_fail(ORB_ERR_ARG, "bad Fuse arguments");
    const int n = points->n;
    if (n == 0 || n_kfs == 0) return ORB_OK;
    if (!best_idx) return orbgpu_fail(ORB_ERR_ARG, "Fuse: null output");
    if (!th_ok(th)) return orbgpu_fail(ORB_ERR_ARG, "Fuse: th must be positive and finite");
    // every argument is checked before the handle's staging is touched
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_view_t& f = kfs[k].frame;
        float steps[kFuseMaxLevels];
        if (f.n < 0 || f.n > kFuseMaxCap || (f.n > 0 && (!f.kps_un || !f.desc)) ||
            !levels_ok(f.nlevels, f.scale_factors, kfs[k].inv_level_sigma2, kfs[k].log_scale_factor, steps))
            return orbgpu_fail(ORB_ERR_ARG, "Fuse: invalid keyframe view (N <= 16384, nlevels <= 12, log scale factor > 0)");
    }
    // packed layout, one upload: per keyframe count | kps | desc | u_right; the points; the skip flags;
    // then the device-only areas (arguments, grids) and the outputs
    struct Off { size_t cnt, kps, desc, ur; };
    std::vector<Off> offs(n_kfs);
    size_t off = 0;
    for (int k = 0; k < n_kfs; ++k) {
        const size_t cap = (size_t)std::max(kfs[k].frame.n, 1);
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 4);
        o.kps = off; off = align256(off + cap * sizeof(orb_keypoint_t));
        o.desc = off; off = align256(off + cap * 32);
        o.ur = off; off = align256(off + cap * 4);
    }
    const size_t N = (size_t)n, jobs = N * (size_t)n_kfs;
    const size_t o_pos = off; off = align256(off + 12 * N);
    const size_t o_nrm = off; off = align256(off + 12 * N);
    const size_t o_min = off; off = align256(off + 4 * N);
    const size_t o_max = off; off = align256(off + 4 * N);
    const size_t o_dsc = off; off = align256(off + 32 * N);
    const size_t o_skip = off; off = align256(off + jobs);
    const size_t o_args = off; off += fuse_args_bytes(n_kfs);
    const size_t in_bytes = o_args;  // (the argument records are uploaded by fuse_launch)
    const size_t o_idx = off; off = align256(off + 4 * jobs);
    const size_t o_dist = off; off = align256(off + 4 * jobs);
    const size_t o_scratch = off;
    for (int k = 0; k < n_kfs; ++k) off = kf_scratch(off, std::max(kfs[k].frame.n, 1)).end;
    const size_t total = off;

    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int rc = orbgpu_matcher_reserve(m, total, &d, &h, &s, &check_ori)) return rc;
    // the keyframes as device views over the staging area
    std::vector<orb_fuse_kf_device_t> dk(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_view_t& f = kfs[k].frame;
        const Off& o = offs[k];
        orb_frame_device_t& g = dk[k].frame;
        memset(&dk[k], 0, sizeof(dk[k]));
        g.kps_un = reinterpret_cast<const orb_keypoint_t*>(d + o.kps);
        g.desc = reinterpret_cast<const uint8_t*>(d + o.desc);
        g.n = reinterpret_cast<const int32_t*>(d + o.cnt);
        g.u_right = f.u_right ? reinterpret_cast<const float*>(d + o.ur) : nullptr;
        g.cap = std::max(f.n, 1);
        g.min_x = f.min_x; g.max_x = f.max_x; g.min_y = f.min_y; g.max_y = f.max_y;
        g.grid_inv_w = f.grid_inv_w; g.grid_inv_h = f.grid_inv_h;
        g.fx = f.fx; g.fy = f.fy; g.cx = f.cx; g.cy = f.cy; g.bf = f.bf; g.b = f.b;
        g.nlevels = f.nlevels;
        g.scale_factors = f.scale_factors;
        memcpy(g.Tcw, f.Tcw, sizeof(g.Tcw));
        memcpy(dk[k].Ow, kfs[k].Ow, sizeof(dk[k].Ow));
        dk[k].inv_level_sigma2 = kfs[k].inv_level_sigma2;
        dk[k].log_scale_factor = kfs[k].log_scale_factor;
    }
    std::vector<FuseKf> recs;
    if (int rc = fuse_prepare(dk.data(), n_kfs, th, recs)) return rc;
    for (int k = 0; k < n_kfs; ++k) {
        const orb_frame_view_t& f = kfs[k].frame;
        const Off& o = offs[k];
        *reinterpret_cast<int32_t*>(h + o.cnt) = f.n;
        if (f.n) {
            memcpy(h + o.kps, f.kps_un, (size_t)f.n * sizeof(orb_keypoint_t));
            memcpy(h + o.desc, f.desc, (size_t)f.n * 32);
            if (f.u_right) memcpy(h + o.ur, f.u_right, (size_t)f.n * 4);
        }
    }
    memcpy(h + o_pos, points->pos, 12 * N);
    memcpy(h + o_nrm, points->normal, 12 * N);
    memcpy(h + o_min, points->min_dist, 4 * N);
    memcpy(h + o_max, points->max_dist, 4 * N);
    memcpy(h + o_dsc, points->desc, 32 * N);
    if (skip) memcpy(h + o_skip, skip, jobs);
    if (hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Fuse upload failed");
    const orb_fuse_points_device_t dp{n, reinterpret_cast<const float*>(d + o_pos), reinterpret_cast<const float*>(d + o_nrm),
                                      reinterpret_cast<const float*>(d + o_min), reinterpret_cast<const float*>(d + o_max),
                                      reinterpret_cast<const uint8_t*>(d + o_dsc)};
    if (int rc = fuse_launch(recs, h + o_args, d + o_args, d + o_scratch, dp,
                             skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr, th,
                             reinterpret_cast<int32_t*>(d + o_idx), reinterpret_cast<int32_t*>(d + o_dist), s))
        return rc;
    if (hipMemcpyAsync(h + o_idx, d + o_idx, o_scratch - o_idx, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "Fuse device error");
    memcpy(best_idx, h + o_idx, 4 * jobs);
    if (best_dist) memcpy(best_dist, h + o_dist, 4 * jobs);
    return ORB_OK;
}

}  // extern "C"
