// ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) on MI355X
// (reference src/ORBmatcher.cc:1951-2185; Frame::GetFeaturesInArea src/Frame.cc:859-951).
//
// The reference loop is sequential in one respect only: once a current keypoint holds a map point
// with observations, later last-frame points skip it (src:2050-2052).  Everything else -- the
// projection, the grid window, the level range, the stereo check, the Hamming distances -- is
// independent per point, so:
//   k_proj_candidates  per last-frame point: project, walk the 64 x 48 grid window in the reference's
//                      cell order and keep (keypoint, distance) of every candidate that passes the
//                      static tests.  Three forms write the same lists: one wave per point (host and
//                      single device calls), and for the tracking chain's batches one thread per point
//                      with the frame's records staged in LDS (_l_b) or, when they do not fit, read
//                      from global memory (_t_b).
//   k_lmp_candidates   the same for SearchByProjection(Frame, local map points) (src:46-240).
//   k_resolve_rounds   one workgroup: the in-order assignment of both overloads (ratio test for the
//                      local map), decided in parallel rounds (below), then the rotation histogram /
//                      ComputeThreeMaxima filter (src:2158-2181).
// Float arithmetic follows the reference build's contractions (see oracle/orb_projection_oracle.cpp);
// this file is compiled with -ffp-contract=off and every fma is explicit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "orbgpu.h"
#include "orb_frame_grid.h"
#include "orb_rot_hist.h"
#include "orbgpu_internal.h"

// Defined in orb_triangulation.hip: the matcher handle's staging buffers and ratio.
int orbgpu_matcher_reserve(orb_matcher_t m, size_t bytes, char** d_buf, char** h_buf, hipStream_t* stream,
                           int* check_ori);
float orbgpu_matcher_nnratio(orb_matcher_t m);
int orbgpu_matcher_check_ori(orb_matcher_t m);

namespace {

constexpr int kThHigh = 100, kHisto = kOrbHistoLength;
constexpr int kMaxLevels = 12;

struct ProjParams {
    float Tcw[12];
    float min_x, max_x, min_y, max_y, inv_w, inv_h, fx, fy, cx, cy, bf, th;
    float scale[kMaxLevels];
    int n_cur, n_last, has_ur, bForward, bBackward, cap, check_ori;
};

// SearchByProjection(Frame&, vector<MapPoint*>, th, bFarPoints, thFarPoints), src:46-240
struct LocalParams {
    float min_x, min_y, inv_w, inv_h, th, th_far, nnratio;
    float scale[kMaxLevels];
    int n_cur, n_pts, has_ur, far, nlevels, cap;
};

struct Cand {
    int32_t i2;
    int32_t dist;
};

// The current frame's records as the window walkers and the candidate test read them: global
// pointers, or in the LDS-staged form orb_frame_grid.h's address-space-3 readers.
template <class KP = const float4*, class UR = const float*, class DS = const uint4*, class CO = const int32_t*,
          class CI = const int32_t*>
struct CurRecords {
    KP kp;  // x, y, angle, octave bits
    UR ur;
    DS desc;
    CO cell_off;
    CI cell_idx;
};

// The argument blocks of the candidate kernels (by value for a single call, one per frame on the
// device for a batch).
struct k_proj_candidates_args {
    ProjParams P;
    const int32_t* n_dev;  // device forms: the point count the prep kernel clamped (NULL: P.n_last)
    const uint8_t* valid;
    const float* xyz;
    const uint4* mp_desc;
    const int32_t* last_octave;
    CurRecords<> cur;
    Cand* cands;
    int32_t* ncand;
    int32_t* overflow;
    const uint8_t* observed;
    int32_t* lister;
};
struct k_lmp_candidates_args {
    LocalParams P;
    const uint8_t* in_view;
    const uint8_t* bad;
    const float* proj;
    const float* view_cos;
    const float* depth;
    const int32_t* level;
    const uint4* mp_desc;
    CurRecords<> cur;
    Cand* cands;
    int32_t* ncand;
    int32_t* overflow;
    const uint8_t* observed;
    const uint8_t* taken0;
    int32_t* lister;
};
__device__ __forceinline__ int n_points(const k_proj_candidates_args& A) { return A.n_dev ? *A.n_dev : A.P.n_last; }
__device__ __forceinline__ int n_points(const k_lmp_candidates_args& A) { return A.P.n_pts; }
__device__ __forceinline__ const uint8_t* taken0(const k_proj_candidates_args&) { return nullptr; }
__device__ __forceinline__ const uint8_t* taken0(const k_lmp_candidates_args& A) { return A.taken0; }

// A point's search: the grid cells x0..x1, y0..y1 around (u, v), the radius, the right-image
// coordinate, the octave range (maxLevel < 0: open) and the point's descriptor.
struct Window {
    int x0, x1, y0, y1;
    float u, v, radius, ur;
    int minLevel, maxLevel;
    uint4 d0, d1;
};

// The cells of (u, v) +- radius (Frame::GetFeaturesInArea, src/Frame.cc:865-885) and the point's
// descriptor; false when the window holds no cell.
template <class Params>
__device__ __forceinline__ bool open_window(const Params& P, const uint4* __restrict__ mp_desc, int i, Window& W) {
    W.x0 = max(0, (int)floorf((W.u - P.min_x - W.radius) * P.inv_w));
    W.x1 = min(kGridCols - 1, (int)ceilf((W.u - P.min_x + W.radius) * P.inv_w));
    W.y0 = max(0, (int)floorf((W.v - P.min_y - W.radius) * P.inv_h));
    W.y1 = min(kGridRows - 1, (int)ceilf((W.v - P.min_y + W.radius) * P.inv_h));
    if (!(W.x0 < kGridCols && W.x1 >= 0 && W.y0 < kGridRows && W.y1 >= 0)) return false;
    W.d0 = mp_desc[2 * (size_t)i];
    W.d1 = mp_desc[2 * (size_t)i + 1];
    return true;
}

// Last-frame point i (src:1978-2037): project with the current pose, the radius of its octave, the
// levels by forward / backward motion (src:2019-2024).  False: the point searches nothing.
__device__ __forceinline__ bool point_window(const k_proj_candidates_args& A, int i, Window& W) {
    const ProjParams& P = A.P;
    if (!A.valid[i]) return false;
    const float x = A.xyz[3 * i], y = A.xyz[3 * i + 1], z = A.xyz[3 * i + 2];
    float c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        c[r] = __fmaf_rn(P.Tcw[4 * r + 2], z, __fmaf_rn(P.Tcw[4 * r], x, P.Tcw[4 * r + 1] * y)) + P.Tcw[4 * r + 3];
    const float invzc = (float)(1.0 / (double)c[2]);
    W.u = P.fx * c[0] / c[2] + P.cx;
    W.v = P.fy * c[1] / c[2] + P.cy;
    if (invzc < 0 || W.u < P.min_x || W.u > P.max_x || W.v < P.min_y || W.v > P.max_y) return false;
    const int oct = A.last_octave[i];
    W.radius = P.th * P.scale[oct];
    if (P.bForward) { W.minLevel = oct; W.maxLevel = -1; }
    else if (P.bBackward) { W.minLevel = 0; W.maxLevel = oct; }
    else { W.minLevel = oct - 1; W.maxLevel = oct + 1; }
    W.ur = __fmaf_rn(-P.bf, invzc, W.u);
    return open_window(P, A.mp_desc, i, W);
}

// Local map point i (src:54-95): in view, not far, not bad; RadiusByViewingCos at the predicted
// level, levels level-1 .. level.
__device__ __forceinline__ bool point_window(const k_lmp_candidates_args& A, int i, Window& W) {
    const LocalParams& P = A.P;
    if (!(A.in_view[i] && !(P.far && A.depth[i] > P.th_far) && !A.bad[i])) return false;
    const int lvl = A.level[i];
    float r = ((double)A.view_cos[i] > 0.998) ? 2.5f : 4.0f;  // RadiusByViewingCos (src:243-250)
    if (P.th != 1.0f) r *= P.th;
    W.radius = r * P.scale[lvl];
    W.u = A.proj[3 * i];
    W.v = A.proj[3 * i + 1];
    W.ur = A.proj[3 * i + 2];
    W.minLevel = lvl - 1;
    W.maxLevel = lvl;
    return open_window(P, A.mp_desc, i, W);
}

// The static tests of keypoint j against a window (src:107-124, :2044-2055): the level range,
// |dx|, |dy| < radius, the stereo u_R gate.  The Hamming distance, or -1 when j is no candidate.
template <class Cur>
struct CandTest {
    const Window& W;
    const int has_ur;
    const Cur& cur;
    __device__ __forceinline__ int operator()(int j) const {
        const float4 kp = cur.kp[j];
        const int koct = __float_as_int(kp.w);
        if (W.minLevel > 0 || W.maxLevel >= 0) {  // bCheckLevels
            if (koct < W.minLevel) return -1;
            if (W.maxLevel >= 0 && koct > W.maxLevel) return -1;
        }
        const float distx = kp.x - W.u, disty = kp.y - W.v;
        if (!(fabsf(distx) < W.radius && fabsf(disty) < W.radius)) return -1;
        if (has_ur && cur.ur[j] > 0) {
            const float er = fabsf(W.ur - cur.ur[j]);
            if (er > W.radius) return -1;
        }
        return hamming(W.d0, W.d1, cur.desc[2 * (size_t)j], cur.desc[2 * (size_t)j + 1]);
    }
};

// After a point's candidates are written: its wave (lanes over the list: first = lane, stride 64) or
// its thread (first 0, stride 1) records, for every usable candidate keypoint (distance < 256, not
// already taken), the earliest observed point listing it (`lister`, initialised to 0x7f7f7f7f).
// k_resolve_init uses it to find the points whose answer no earlier point can change.
__device__ __forceinline__ void record_listers(int first, int stride, int i, int n, int cap, const Cand* __restrict__ c_i,
                                               const uint8_t* __restrict__ taken0, int32_t* __restrict__ lister) {
    if (n > cap) return;  // overflow: the call is redone with a larger capacity
    for (int k = first; k < n; k += stride) {
        const Cand c = c_i[k];
        if (c.dist < 256 && !(taken0 && taken0[c.i2])) atomicMin(&lister[c.i2], i);
    }
}

// One wave scans one point's grid window (Frame::GetFeaturesInArea, src/Frame.cc:859-951) in the
// reference's order -- cells ix outer, iy inner, keypoints of a cell in index order -- with the lanes
// spread over the window: 64 cells at a time, a wave prefix sum of the cells' keypoint counts, then
// 64 keypoints at a time (lane -> cell by binary search of the prefix), `test(j)` -> Hamming distance
// or -1, and an order-preserving ballot compaction into out[0 .. cap).  Returns the candidate count
// (wave-uniform; counted beyond cap).
template <class Test>
__device__ __forceinline__ int window_candidates(int lane, int* __restrict__ pre, int* __restrict__ beg,
                                                 const int32_t* __restrict__ cell_off, const int32_t* __restrict__ cell_idx,
                                                 int x0, int x1, int y0, int y1, Cand* __restrict__ out, int cap,
                                                 Test test) {
    const int ny = y1 - y0 + 1, ncells = (x1 - x0 + 1) * ny;
    int n = 0;
    for (int c0 = 0; c0 < ncells; c0 += 64) {
        const int t = c0 + lane;
        int b = 0, cnt = 0;
        if (t < ncells) {
            const int cell = (x0 + t / ny) * kGridRows + (y0 + t % ny);
            b = cell_off[cell];
            cnt = cell_off[cell + 1] - b;
        }
        int incl = cnt;  // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int total = __shfl(incl, 63, 64);
        pre[lane] = incl - cnt;
        beg[lane] = b;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int it = i0 + lane;
            int j = -1, dist = -1;
            if (it < total) {
                int lo = 0, hi = 63;  // the last cell lane whose prefix is <= it
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (pre[mid] <= it) lo = mid;
                    else hi = mid - 1;
                }
                j = cell_idx[beg[lo] + it - pre[lo]];
                dist = test(j);
            }
            const unsigned long long m = __ballot(dist >= 0);
            const int pos = n + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (dist >= 0 && pos < cap) out[pos] = Cand{j, dist};
            n += (int)__popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    return n;
}

// The same candidate lists with one THREAD per point (round 5): a window holds a handful of cells and
// keypoints, so a wave per point spent most of its time on the 64-lane prefix and compaction machinery;
// a thread walks its window's cells (ix outer, iy inner) and their keypoints in index order, which is
// window_candidates' order, and writes the same list.
template <class Test, class CO, class CI>
__device__ __forceinline__ int window_candidates_serial(CO cell_off, CI cell_idx, int x0, int x1, int y0,
                                                        int y1, Cand* __restrict__ out, int cap, Test test) {
    int n = 0;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const int cell = ix * kGridRows + iy;
            const int b = cell_off[cell], e = cell_off[cell + 1];
            for (int k = b; k < e; ++k) {
                const int j = cell_idx[k];
                const int dist = test(j);
                if (dist >= 0) {
                    if (n < cap) out[n] = Cand{j, dist};
                    ++n;
                }
            }
        }
    return n;
}

constexpr int kCandWaves = 4;
constexpr int kCandThreads = 256;

// One wave per point, both overloads (src:54-143 / :1978-2062 up to the minima).  pre / beg: the
// wave's 64-entry prefix arrays in LDS.
template <class Args>
__device__ __forceinline__ void candidates_wave(const Args& A, int* pre, int* beg) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCandWaves + (threadIdx.x >> 6);
    if (i >= n_points(A)) return;
    Cand* const out = A.cands + (size_t)i * A.P.cap;
    Window W;
    int n = 0;
    if (point_window(A, i, W))
        n = window_candidates(lane, pre, beg, A.cur.cell_off, A.cur.cell_idx, W.x0, W.x1, W.y0, W.y1, out, A.P.cap,
                              CandTest<CurRecords<>>{W, A.P.has_ur, A.cur});
    if (lane == 0) {
        A.ncand[i] = n;
        if (n > A.P.cap) atomicMax(A.overflow, n);
    }
    __threadfence_block();  // the wave's own candidate stores, read back across lanes
    if (A.observed[i]) record_listers(lane, 64, i, n, A.P.cap, out, taken0(A), A.lister);
}

// One thread per point (point i), the current frame's records through `cur`.
template <class Args, class Cur>
__device__ __forceinline__ void candidates_thread(const Args& A, int i, const Cur& cur) {
    if (i >= n_points(A)) return;
    Cand* const out = A.cands + (size_t)i * A.P.cap;
    Window W;
    int n = 0;
    if (point_window(A, i, W))
        n = window_candidates_serial(cur.cell_off, cur.cell_idx, W.x0, W.x1, W.y0, W.y1, out, A.P.cap,
                                     CandTest<Cur>{W, A.P.has_ur, cur});
    A.ncand[i] = n;
    if (n > A.P.cap) atomicMax(A.overflow, n);
    if (A.observed[i]) record_listers(0, 1, i, n, A.P.cap, out, taken0(A), A.lister);
}

__global__ __launch_bounds__(64 * kCandWaves) void k_proj_candidates(const k_proj_candidates_args A) {
    __shared__ int pre_s[kCandWaves][64], beg_s[kCandWaves][64];
    candidates_wave(A, pre_s[threadIdx.x >> 6], beg_s[threadIdx.x >> 6]);
}
__global__ __launch_bounds__(64 * kCandWaves) void k_lmp_candidates(const k_lmp_candidates_args A) {
    __shared__ int pre_s[kCandWaves][64], beg_s[kCandWaves][64];
    candidates_wave(A, pre_s[threadIdx.x >> 6], beg_s[threadIdx.x >> 6]);
}
// a thread per point on frame blockIdx.y of a batch (one argument block per frame)
__global__ __launch_bounds__(kCandThreads) void k_proj_candidates_t_b(const k_proj_candidates_args* __restrict__ a) {
    const k_proj_candidates_args& A = a[blockIdx.y];
    candidates_thread(A, blockIdx.x * kCandThreads + threadIdx.x, A.cur);
}
__global__ __launch_bounds__(kCandThreads) void k_lmp_candidates_t_b(const k_lmp_candidates_args* __restrict__ a) {
    const k_lmp_candidates_args& A = a[blockIdx.y];
    candidates_thread(A, blockIdx.x * kCandThreads + threadIdx.x, A.cur);
}

// LDS-staged batch forms (round 6).  The thread forms above walk a window as a chain of dependent
// global loads per candidate (cell offsets -> keypoint index -> keypoint record -> descriptor); with a
// batch those records are spread over hundreds of frames and miss the caches.  Here one 1024-thread
// workgroup per frame first copies the frame's grid (cell offsets, cell index list) and its keypoint
// records (x, y, angle, octave; u_R; descriptors: all `cap` rows, the frame's padding included) into
// LDS, then every thread walks its points' windows with the same code -- the same lists in the same
// order, the chain now on LDS.  LDS: 56 B per keypoint + the 3,073 cell offsets (cap <= kCandLdsCap).
constexpr int kCandLdsThreads = 1024;
constexpr int kCandLdsCap = (160 * 1024 - 4 * (kGridCols * kGridRows + 1)) / 56;
__host__ __device__ constexpr size_t cand_lds_bytes(int cap) {
    return (size_t)cap * (32 + 16 + 4 + 4) + 4 * (size_t)(kGridCols * kGridRows + 1);
}
// (the staged records are read through orb_frame_grid.h's address-space-3 readers)
using CandLds = CurRecords<LdsF4, LdsArr<float>, LdsU4, LdsArr<int32_t>, LdsArr<int32_t>>;
// descriptors | keypoint records | u_R | cell index list | cell offsets (16-B aligned sections); the
// first `rows` keypoint rows are staged (the cell offsets always)
__device__ __forceinline__ CandLds stage_frame_lds(uint8_t* smem, int cap, const CurRecords<>& g, int rows) {
    uint4* s_desc = reinterpret_cast<uint4*>(smem);
    float4* s_kp = reinterpret_cast<float4*>(smem + 32 * (size_t)cap);
    float* s_ur = reinterpret_cast<float*>(smem + 48 * (size_t)cap);
    int32_t* s_idx = reinterpret_cast<int32_t*>(smem + 52 * (size_t)cap);
    int32_t* s_off = reinterpret_cast<int32_t*>(smem + 56 * (size_t)cap);
    const int t = threadIdx.x;
    for (int k = t; k < 2 * rows; k += kCandLdsThreads) s_desc[k] = g.desc[k];
    for (int k = t; k < rows; k += kCandLdsThreads) {
        s_kp[k] = g.kp[k];
        s_idx[k] = g.cell_idx[k];
        if (g.ur) s_ur[k] = g.ur[k];
    }
    for (int k = t; k <= kGridCols * kGridRows; k += kCandLdsThreads) s_off[k] = g.cell_off[k];
    __syncthreads();
    // (u_R is read only when the frame has it, ProjParams / LocalParams has_ur)
    return CandLds{LdsF4{(const ORB_LDS float*)s_kp}, LdsArr<float>{(const ORB_LDS float*)s_ur},
                   LdsU4{(const ORB_LDS uint32_t*)s_desc}, LdsArr<int32_t>{(const ORB_LDS int32_t*)s_off},
                   LdsArr<int32_t>{(const ORB_LDS int32_t*)s_idx}};
}
// ---- the in-order assignment, resolved by parallel fixed-point rounds ----------------------------
// Both SearchByProjection loops visit the points in index order, and point i only sees the state the
// earlier points left: a current keypoint that holds a map point with observations is skipped
// (src:103-105, src:2040-2042).  That state changes once per keypoint -- the first successful
// assignment by an observed point -- so point i's answer is a function f_i of which of its candidates
// earlier observed points claimed:
//   A(i) = f_i({ j : some k < i, observed(k), A(k) = j }).
// One workgroup iterates this map on all points at once (Jacobi): every round computes claimMin[j] =
// the smallest observed point whose current answer is j, then every point re-derives its answer with
// the candidates claimed by an earlier point excluded.  A fixed point is the sequential answer (by
// induction on i), and after round r the first r points are final, so the iteration ends; in practice
// after a few rounds more than the longest chain of actual claim conflicts.  The results are then
// exactly those of the sequential loop:
//   mp[j]  = the last point assigned to keypoint j (a later unobserved-free assignment overwrites an
//            earlier one, src:156 / :2067), or -1;
//   count  = every successful assignment (the reference's nmatches++ per assignment), minus, for
//            SearchByProjection(Frame, Frame) with checkOri, every assignment in a rotation bin outside
//            ComputeThreeMaxima's top three, whose keypoint is then cleared (src:2160-2181).
// The candidate kernels store each point's candidates in the reference's scan order (the order key of
// a candidate is its list position) with their Hamming distances; the first / second minimum of the
// reference's update rules (src:126-142, :2057-2061) are the lexicographic (distance, order) minima.
constexpr int kResolveThreads = 1024, kResolveLdsKeypoints = 16384;
constexpr unsigned long long kNone = ~0ull;
constexpr int kTop = 8;  // best usable candidates kept per point for the rounds

struct ResolveArgs {
    int n_pts, n_cur, cap;
    int local;          // 1: best + second best with the ratio test (src:145-167); 0: best only (src:2064-2068)
    int check_ori;      // rotation histogram (SearchByProjection(Frame, Frame) only)
    float nnratio;
    const Cand* cands;
    const int32_t* ncand;
    const uint8_t* observed;   // per point: its map point has Observations() > 0
    const uint8_t* taken0;     // per keypoint: holds a map point with observations before the call (may be null)
    const float4* cur_kp;      // x, y, angle, octave bits
    const float* last_angle;   // per point (rotation bins)
    const int32_t* overflow;   // the candidate pass's overflow (> cap: results not written)
    int32_t* st;               // per point: the current answer, -1 no match, j >= 0 keypoint j
    int lds_keypoints;         // 1: claimMin in LDS (dynamic, 4 B per keypoint)
    int32_t* claimMin;         // per keypoint (when not in LDS)
    const int32_t* lister;     // per keypoint: the first observed point listing it (candidate kernels)
    int32_t* fixed;            // per keypoint: the smallest final (unaffected) observed claimant (0x7f.. none)
    int32_t* work;             // the points whose answer can change (the rounds' list), count in out_n[2]
    int4* top;                 // per point: its kTop best usable candidates as (dist, i2) pairs, by (dist, order)
    int32_t* nusable;          // per point: its usable candidate count
    int32_t* last;             // per keypoint
    int32_t* removed;          // per keypoint
    int32_t* mp;               // out: per keypoint
    int32_t* out_n;            // out: [0] count, [1] rounds
    int32_t* out_user;         // out (device forms, may be null): the count, for the caller
    const int32_t* dims;       // device forms: [0] n_pts, [1] n_cur read on the device (NULL: the fields above)
};

// a candidate resolve_point can take (the lister pass counts exactly these)
__device__ __forceinline__ bool usable(const ResolveArgs& a, const Cand& c) {
    return c.dist < 256 && !(a.taken0 && a.taken0[c.i2]);
}

// Visit point i's usable candidates in list order, fn(candidate, position).  The list is read 8
// entries at a time (and their taken0 bytes 8 at a time), so a thread keeps 8 loads in flight instead
// of one dependent round trip per candidate.
template <class Fn>
__device__ __forceinline__ void for_each_usable(const ResolveArgs& a, int i, Fn fn) {
    const Cand* C = a.cands + (size_t)i * a.cap;
    const int n = a.ncand[i];
    for (int k0 = 0; k0 < n; k0 += 8) {
        Cand cs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cs[u] = k0 + u < n ? C[k0 + u] : Cand{0, 256};
        bool tk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) tk[u] = a.taken0 && cs[u].dist < 256 && a.taken0[cs[u].i2];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (cs[u].dist < 256 && !tk[u]) fn(cs[u], k0 + u);  // dist >= 256: never below the initial 256
    }
}

// point i's answer given claimMin (candidates claimed by an earlier point excluded): the first and
// second minimum of (distance, list position), the reference's update order
__device__ __forceinline__ int resolve_point(const ResolveArgs& a, const int32_t* claimMin, int i) {
    unsigned long long m1 = kNone, m2 = kNone;
    int j1 = -1, j2 = -1;
    for_each_usable(a, i, [&](const Cand& c, int k) {  // (selects, no branches: the state stays in registers)
        const bool ok = claimMin[c.i2] >= i;
        const unsigned long long key = ((unsigned long long)c.dist << 32) | (unsigned)k;
        const bool lt1 = ok && key < m1, lt2 = ok && key < m2;
        m2 = lt1 ? m1 : (lt2 ? key : m2);
        j2 = lt1 ? j1 : (lt2 ? c.i2 : j2);
        m1 = lt1 ? key : m1;
        j1 = lt1 ? c.i2 : j1;
    });
    if (m1 == kNone) return -1;
    const int d1 = (int)(m1 >> 32);
    if (d1 > kThHigh) return -1;
    if (a.local) {  // src:148-155
        const int l1 = __float_as_int(a.cur_kp[j1].w);
        const int l2 = m2 != kNone ? __float_as_int(a.cur_kp[j2].w) : -1;
        const int d2 = m2 != kNone ? (int)(m2 >> 32) : 256;
        if (l1 == l2 && (float)d1 > a.nnratio * (float)d2) return -1;
    }
    return j1;
}

// The answer rules (src:145-167 / :2064-2068) given the first and second unclaimed candidates.
__device__ __forceinline__ int decide(const ResolveArgs& a, int d1, int j1, int d2, int j2) {
    if (j1 < 0 || d1 > kThHigh) return -1;
    if (a.local) {  // src:148-155
        const int l1 = __float_as_int(a.cur_kp[j1].w);
        const int l2 = j2 >= 0 ? __float_as_int(a.cur_kp[j2].w) : -1;
        if (l1 == l2 && (float)d1 > a.nnratio * (float)(j2 >= 0 ? d2 : 256)) return -1;
    }
    return j1;
}

// Points that cannot be affected are taken out of the rounds: point i can only lose a candidate j to
// an observed point k < i that has j among its usable candidates, so if every usable candidate of i
// has no such earlier lister, i's unconstrained answer is final, and its claim is fixed.
// k_resolve_init (one thread per point, over the whole chip): the unconstrained answer, the point's
// kTop best usable candidates in (distance, order), the classification, the work list and the fixed
// claims.  k_resolve_rounds (one workgroup) then iterates only the work list, each point re-deciding
// from its kTop best (a full scan only when too many of them are claimed).
__device__ __forceinline__ void resolve_init_point(const ResolveArgs& a, int i) {
    unsigned long long t[kTop];
    int ti[kTop];
#pragma unroll
    for (int q = 0; q < kTop; ++q) { t[q] = kNone; ti[q] = -1; }
    int nu = 0;
    bool affected = false;
    for_each_usable(a, i, [&](const Cand& c, int k) {
        ++nu;
        affected |= a.lister[c.i2] < i;
        unsigned long long key = ((unsigned long long)c.dist << 32) | (unsigned)k;
        int j = c.i2;
#pragma unroll
        for (int q = 0; q < kTop; ++q) {  // insertion into the sorted kTop (selects only)
            const bool lt = key < t[q];
            const unsigned long long tk = t[q];
            const int tj = ti[q];
            t[q] = lt ? key : tk;
            ti[q] = lt ? j : tj;
            key = lt ? tk : key;
            j = lt ? tj : j;
        }
    });
    const int st = decide(a, (int)(t[0] >> 32), ti[0], (int)(t[1] >> 32), ti[1]);
    a.st[i] = st;
#pragma unroll
    for (int q = 0; q < kTop; q += 2)
        a.top[(size_t)i * (kTop / 2) + q / 2] = make_int4((int)(t[q] >> 32), ti[q], (int)(t[q + 1] >> 32), ti[q + 1]);
    a.nusable[i] = nu;
    if (affected) a.work[atomicAdd(&a.out_n[2], 1)] = i;
    else if (st >= 0 && a.observed[i]) atomicMin(&a.fixed[st], i);
}
__device__ __forceinline__ void k_resolve_init_body(ResolveArgs a) {
    if (a.dims) {
        a.n_pts = a.dims[0];
        a.n_cur = a.dims[1];
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_pts || *a.overflow > a.cap) return;
    resolve_init_point(a, i);
}
__global__ __launch_bounds__(256) void k_resolve_init(ResolveArgs a) {
    k_resolve_init_body(a);
}
struct k_resolve_init_args {
    ResolveArgs a;
};
// the same on frame blockIdx.y of a batch (one argument block per frame)
__global__ __launch_bounds__(256) void k_resolve_init_b(const k_resolve_init_args* __restrict__ a) {
    const k_resolve_init_args& A = a[blockIdx.y];
    k_resolve_init_body(A.a);
}

// The LDS-staged candidate passes of a batch (one workgroup per frame).  (Running k_resolve_init's
// per-point pass in the same launch, after the frame's listers are final, was measured slower: 2.14 ->
// 2.62 ms per 512-frame call -- one CU per frame instead of the whole chip.)
__global__ __launch_bounds__(kCandLdsThreads) void k_proj_candidates_l_b(const k_proj_candidates_args* __restrict__ a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cand_smem[];
    const k_proj_candidates_args& A = a[blockIdx.x];
    const int np = n_points(A);
    if (np == 0) return;  // (a frame the motion gate turned off: nothing to stage)
    const CandLds S = stage_frame_lds(cand_smem, A.P.cap, A.cur, A.P.cap);
    for (int i = threadIdx.x; i < np; i += kCandLdsThreads) candidates_thread(A, i, S);
}
__global__ __launch_bounds__(kCandLdsThreads) void k_lmp_candidates_l_b(const k_lmp_candidates_args* __restrict__ a,
                                                                        const k_resolve_init_args* __restrict__ ri) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cand_smem[];
    const k_lmp_candidates_args& A = a[blockIdx.x];
    const ResolveArgs& R = ri[blockIdx.x].a;
    if (A.P.n_pts == 0) return;
    // a frame without keypoints (the motion gate's failed frames) stages only its (empty) grid
    const CandLds S = stage_frame_lds(cand_smem, A.P.cap, A.cur, R.dims && R.dims[1] == 0 ? 0 : A.P.cap);
    for (int i = threadIdx.x; i < A.P.n_pts; i += kCandLdsThreads) candidates_thread(A, i, S);
}

// point i's answer in a round, from its kTop best (claims by earlier points excluded)
__device__ __forceinline__ int resolve_top(const ResolveArgs& a, const int32_t* claimMin, int i) {
    int d1 = 0, j1 = -1, d2 = 0, j2 = -1, found = 0;
#pragma unroll
    for (int q = 0; q < kTop; q += 2) {
        const int4 e = a.top[(size_t)i * (kTop / 2) + q / 2];
        const int d[2] = {e.x, e.z}, j[2] = {e.y, e.w};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (j[u] < 0 || claimMin[j[u]] < i) continue;
            if (found == 0) { d1 = d[u]; j1 = j[u]; }
            else if (found == 1) { d2 = d[u]; j2 = j[u]; }
            ++found;
        }
    }
    const int need = a.local ? 2 : 1;
    if (found < need && a.nusable[i] > kTop) return resolve_point(a, claimMin, i);
    return decide(a, d1, j1, d2, j2);
}

// A work point's round state in registers: its kTop best (keypoint, distance, level), usable count,
// index, observed flag and current answer; the rounds then touch only LDS.
struct WorkPoint {
    int i, st, nu, obs;
    uint32_t e[kTop];  // keypoint (16 bits) | distance << 16 (8 bits) | (level + 1) << 24; 0xffffffff: none
};
constexpr int kWorkPerThread = 2;

__device__ __forceinline__ void load_work(const ResolveArgs& a, int i, WorkPoint& p) {
    p.i = i;
    p.st = a.st[i];
    p.nu = a.nusable[i];
    p.obs = a.observed[i];
    int d[kTop], j[kTop];
#pragma unroll
    for (int q = 0; q < kTop; q += 2) {
        const int4 t = a.top[(size_t)i * (kTop / 2) + q / 2];
        d[q] = t.x; j[q] = t.y; d[q + 1] = t.z; j[q + 1] = t.w;
    }
#pragma unroll
    for (int q = 0; q < kTop; ++q) {  // octaves are 0 .. 11, distances < 256, keypoints < 65536
        const int l1 = (a.local && j[q] >= 0) ? __float_as_int(a.cur_kp[j[q]].w) + 1 : 0;
        p.e[q] = j[q] < 0 ? 0xffffffffu : (uint32_t)j[q] | (uint32_t)d[q] << 16 | (uint32_t)l1 << 24;
    }
}

// resolve_top on a register-resident work point (same rules; the full scan when its kTop best run out)
__device__ __forceinline__ int resolve_reg(const ResolveArgs& a, const int32_t* claimMin, const WorkPoint& p) {
    uint32_t e1 = 0xffffffffu, e2 = 256u << 16;  // (e2 default: distance 256, level -1)
    int found = 0;
#pragma unroll
    for (int q = 0; q < kTop; ++q) {
        const bool ok = p.e[q] != 0xffffffffu && claimMin[p.e[q] & 0xffffu] >= p.i;
        if (ok && found == 0) e1 = p.e[q];
        else if (ok && found == 1) e2 = p.e[q];
        found += ok ? 1 : 0;
    }
    if (found < (a.local ? 2 : 1) && p.nu > kTop) return resolve_point(a, claimMin, p.i);
    if (found == 0) return -1;
    const int j1 = (int)(e1 & 0xffffu), d1 = (int)((e1 >> 16) & 0xffu), l1 = (int)(e1 >> 24) - 1;
    const int d2 = found > 1 ? (int)((e2 >> 16) & 0xffu) : 256, l2 = found > 1 ? (int)(e2 >> 24) - 1 : -1;
    if (d1 > kThHigh) return -1;
    if (a.local && l1 == l2 && (float)d1 > a.nnratio * (float)d2) return -1;  // src:148-155
    return j1;
}

__device__ __forceinline__ void k_resolve_rounds_body(ResolveArgs a) {
    if (a.dims) {
        a.n_pts = a.dims[0];
        a.n_cur = a.dims[1];
    }
    const int tid = threadIdx.x;
    __shared__ int hist[kHisto], keep[3], cnt[2];
    extern __shared__ int32_t kp_lds[];
    int32_t* const claimMin = a.lds_keypoints ? kp_lds : a.claimMin;
    if (*a.overflow > a.cap) {  // the host re-runs with a larger capacity
        if (tid == 0) *a.out_n = -1;
        return;
    }
    for (int j = tid; j < a.n_cur; j += kResolveThreads) {
        a.last[j] = -1;
        a.removed[j] = 0;
    }
    if (tid < kHisto) hist[tid] = 0;
    if (tid < 2) cnt[tid] = 0;
    const int nw = a.out_n[2];
    int rounds = 1;
    if (nw <= kWorkPerThread * kResolveThreads && a.n_cur <= 65536) {
        // the usual case: every work point in registers, the fixed claims in LDS next to claimMin
        int32_t* const fixedL = a.lds_keypoints ? kp_lds + a.n_cur : a.fixed;
        WorkPoint wp[kWorkPerThread];
#pragma unroll
        for (int q = 0; q < kWorkPerThread; ++q) {
            const int w = tid + q * kResolveThreads;
            wp[q].i = -1;
            if (w < nw) load_work(a, a.work[w], wp[q]);
        }
        if (a.lds_keypoints)
            for (int j = tid; j < a.n_cur; j += kResolveThreads) fixedL[j] = a.fixed[j];
        for (;; ++rounds) {
            __syncthreads();
            for (int j = tid; j < a.n_cur; j += kResolveThreads) claimMin[j] = fixedL[j];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kWorkPerThread; ++q)
                if (wp[q].i >= 0 && wp[q].st >= 0 && wp[q].obs) atomicMin(&claimMin[wp[q].st], wp[q].i);
            __syncthreads();
            int changed = 0;
#pragma unroll
            for (int q = 0; q < kWorkPerThread; ++q) {
                if (wp[q].i < 0) continue;
                const int r = resolve_reg(a, claimMin, wp[q]);
                changed += r != wp[q].st;
                wp[q].st = r;
            }
            if (__syncthreads_count(changed) == 0 || rounds > a.n_pts) break;
        }
#pragma unroll
        for (int q = 0; q < kWorkPerThread; ++q)
            if (wp[q].i >= 0) a.st[wp[q].i] = wp[q].st;
        __syncthreads();  // (global st: visible to the workgroup's results pass below)
    } else {
        for (;; ++rounds) {
            __syncthreads();
            for (int j = tid; j < a.n_cur; j += kResolveThreads) claimMin[j] = a.fixed[j];
            __syncthreads();
            for (int w = tid; w < nw; w += kResolveThreads) {
                const int i = a.work[w], j = a.st[i];
                if (j >= 0 && a.observed[i]) atomicMin(&claimMin[j], i);
            }
            __syncthreads();
            int changed = 0;
            for (int w = tid; w < nw; w += kResolveThreads) {
                const int i = a.work[w];
                const int r = resolve_top(a, claimMin, i);
                if (r != a.st[i]) {
                    a.st[i] = r;
                    ++changed;
                }
            }
            if (__syncthreads_count(changed) == 0 || rounds > a.n_pts) break;
        }
    }
    // results
    int nsucc = 0;
    for (int i = tid; i < a.n_pts; i += kResolveThreads) {
        const int j = a.st[i];
        if (j < 0) continue;
        ++nsucc;
        atomicMax(&a.last[j], i);
        if (a.check_ori) atomicAdd(&hist[orb_rot_bin(a.last_angle[i], a.cur_kp[j].z)], 1);
    }
    atomicAdd(&cnt[0], nsucc);
    __syncthreads();
    if (a.check_ori) {
        if (tid == 0) orb_three_maxima(hist, keep);  // ComputeThreeMaxima (src:2336-2378)
        __syncthreads();
        int nrem = 0;
        for (int i = tid; i < a.n_pts; i += kResolveThreads) {
            const int j = a.st[i];
            if (j < 0) continue;
            const int b = orb_rot_bin(a.last_angle[i], a.cur_kp[j].z);
            if (b != keep[0] && b != keep[1] && b != keep[2]) {
                a.removed[j] = 1;
                ++nrem;
            }
        }
        atomicAdd(&cnt[1], nrem);
        __syncthreads();
    }
    for (int j = tid; j < a.n_cur; j += kResolveThreads) a.mp[j] = a.removed[j] ? -1 : a.last[j];
    if (tid == 0) {
        a.out_n[0] = cnt[0] - cnt[1];
        a.out_n[1] = rounds;
        a.out_n[2] = nw;
        if (a.out_user) a.out_user[0] = cnt[0] - cnt[1];
    }
}
__global__ __launch_bounds__(kResolveThreads) void k_resolve_rounds(ResolveArgs a) {
    k_resolve_rounds_body(a);
}
struct k_resolve_rounds_args {
    ResolveArgs a;
};
// the same on frame blockIdx.y of a batch (one argument block per frame)
__global__ __launch_bounds__(kResolveThreads) void k_resolve_rounds_b(const k_resolve_rounds_args* __restrict__ a) {
    const k_resolve_rounds_args& A = a[blockIdx.y];
    k_resolve_rounds_body(A.a);
}

// ---- device-resident forms: the frame's grid and packed keypoints built on the device ------------
// Each prep kernel takes its argument block by value; the _b form runs frame blockIdx.y of a batch
// from one block per frame.

// The grid build itself (k_frame_prep_body, with the scratch initialisation it does in place of fill
// launches) is in orb_frame_grid.h, shared with Fuse.
struct k_frame_prep_args {
    const orb_keypoint_t* kps;
    const int32_t* n_ptr;
    int cap;
    float min_x;
    float min_y;
    float inv_w;
    float inv_h;
    float4* kp4;
    int32_t* cell_off;
    int32_t* cell_idx;
    int32_t* cell_of;
    int32_t* n_out0;
    int32_t* n_out1;
    ScratchInit z;
};
__device__ __forceinline__ void frame_prep(const k_frame_prep_args& A) {
    k_frame_prep_body(A.kps, A.n_ptr, A.cap, A.min_x, A.min_y, A.inv_w, A.inv_h, A.kp4, A.cell_off, A.cell_idx,
                      A.cell_of, A.n_out0, A.n_out1, A.z);
}
__global__ __launch_bounds__(kPrepThreads) void k_frame_prep(const k_frame_prep_args A) { frame_prep(A); }
__global__ __launch_bounds__(kPrepThreads) void k_frame_prep_b(const k_frame_prep_args* __restrict__ a) {
    frame_prep(a[blockIdx.y]);
}

// the last frame's per-point inputs of k_proj_candidates / the rotation bins: a point whose octave is
// outside the pyramid is not valid (the host form rejects the call instead)
struct k_last_prep_args {
    const orb_keypoint_t* kps;
    const uint8_t* valid;
    const int32_t* n_ptr;
    int cap;
    int nlevels;
    uint8_t* valid2;
    int32_t* octave;
    float* angle;
    int32_t* n_out0;
    int32_t* n_out1;
};
__device__ __forceinline__ void last_prep(const k_last_prep_args& A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(*A.n_ptr, 0), A.cap);
    if (i == 0) {
        *A.n_out0 = n;
        if (A.n_out1) *A.n_out1 = n;
    }
    if (i >= n) return;
    const orb_keypoint_t kp = A.kps[i];
    A.octave[i] = kp.octave;
    A.angle[i] = kp.angle;
    A.valid2[i] = A.valid[i] && kp.octave >= 0 && kp.octave < A.nlevels;
}
__global__ __launch_bounds__(256) void k_last_prep(const k_last_prep_args A) { last_prep(A); }
__global__ __launch_bounds__(256) void k_last_prep_b(const k_last_prep_args* __restrict__ a) { last_prep(a[blockIdx.y]); }

// local map points: a predicted level outside the pyramid leaves the point out
struct k_local_prep_args {
    const uint8_t* in_view;
    const int32_t* level;
    int n;
    int nlevels;
    uint8_t* in_view2;
};
__device__ __forceinline__ void local_prep(const k_local_prep_args& A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < A.n) A.in_view2[i] = A.in_view[i] && A.level[i] >= 0 && A.level[i] < A.nlevels;
}
__global__ __launch_bounds__(256) void k_local_prep(const k_local_prep_args A) { local_prep(A); }
__global__ __launch_bounds__(256) void k_local_prep_b(const k_local_prep_args* __restrict__ a) { local_prep(a[blockIdx.y]); }

// ---- host side ----------------------------------------------------------------------------------

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// k_resolve_rounds keeps claimMin and the fixed claims in dynamic LDS (8 B per keypoint, up to 128 KB)
bool resolve_lds_ready() {
    static const bool ok = hipFuncSetAttribute((const void*)k_resolve_rounds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               8 * kResolveLdsKeypoints) == hipSuccess;
    return ok;
}

// The candidate pass is one wave per point for a single call and one thread per point for a batch;
// both write the same lists.  A single frame's few thousand points leave the chip mostly idle, and a
// wave's parallel window scan has the shorter latency (0.51 vs 0.65 ms per tracked frame); a batch
// fills the chip, and threads carry far less per-point machinery (256 frames: 3.2 -> 1.5 ms per call).
// A batch takes the LDS-staged form (k_*_candidates_l_b) unless the frame's records do not fit one
// workgroup's LDS; then the threads read global memory (k_*_candidates_t_b).
bool cand_lds_mode(int cap) {
    if (cap > kCandLdsCap) return false;
    static const bool ready = [] {
        return hipFuncSetAttribute((const void*)k_proj_candidates_l_b, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)cand_lds_bytes(kCandLdsCap)) == hipSuccess &&
               hipFuncSetAttribute((const void*)k_lmp_candidates_l_b, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)cand_lds_bytes(kCandLdsCap)) == hipSuccess;
    }();
    return ready;
}

int sbp_fail(int code, const char* before, const char* name, const char* after) {
    return orbgpu_fail(code, (std::string(before) + name + after).c_str());
}

// A call's scratch, carved in 256-B aligned pieces.  A layout is run once with a null base for its
// size (z.off) and once with the real base for the pointers, so the two cannot disagree.
struct DevScratch {
    char* base = nullptr;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off = align256(off + std::max<size_t>(count, 1) * sizeof(T));
        return p;
    }
};

// Frame is orb_frame_view_t or orb_frame_device_t: the same scalar fields.
template <class Frame>
ProjParams make_proj_params(const Frame* cur, const float* last_Tcw, float th, int mono, int n_cur, int n_last, int cap,
                            int check_ori) {
    ProjParams P{};
    memcpy(P.Tcw, cur->Tcw, sizeof(P.Tcw));
    P.min_x = cur->min_x; P.max_x = cur->max_x; P.min_y = cur->min_y; P.max_y = cur->max_y;
    P.inv_w = cur->grid_inv_w; P.inv_h = cur->grid_inv_h;
    P.fx = cur->fx; P.fy = cur->fy; P.cx = cur->cx; P.cy = cur->cy; P.bf = cur->bf; P.th = th;
    for (int l = 0; l < cur->nlevels; ++l) P.scale[l] = cur->scale_factors[l];
    P.n_cur = n_cur; P.n_last = n_last; P.has_ur = cur->u_right != nullptr;
    {   // twc = -R^T t, tlc = Tlw * twc (src:1960-1968)
        const float* T = cur->Tcw;
        float twc[3], tlc[3];
        for (int i = 0; i < 3; ++i) twc[i] = -std::fma(T[8 + i], T[11], std::fma(T[i], T[3], T[4 + i] * T[7]));
        for (int i = 0; i < 3; ++i)
            tlc[i] = std::fma(last_Tcw[4 * i + 2], twc[2], std::fma(last_Tcw[4 * i], twc[0], last_Tcw[4 * i + 1] * twc[1])) +
                     last_Tcw[4 * i + 3];
        P.bForward = tlc[2] > cur->b && !mono;
        P.bBackward = -tlc[2] > cur->b && !mono;
    }
    P.cap = cap;
    P.check_ori = check_ori;
    return P;
}

template <class Frame>
LocalParams make_local_params(const Frame* F, float th, int far_points, float th_far_points, int n_cur, int n_pts,
                              int cap, float nnratio) {
    LocalParams P{};
    P.min_x = F->min_x; P.min_y = F->min_y; P.inv_w = F->grid_inv_w; P.inv_h = F->grid_inv_h;
    P.th = th; P.th_far = th_far_points; P.nnratio = nnratio;
    for (int l = 0; l < F->nlevels; ++l) P.scale[l] = F->scale_factors[l];
    P.n_cur = n_cur; P.n_pts = n_pts; P.has_ur = F->u_right != nullptr; P.far = far_points ? 1 : 0; P.nlevels = F->nlevels;
    P.cap = cap;
    return P;
}

// The candidate lists and the resolver's working set of one call, n_cur keypoints and np points:
// lister + fixed claims (to be initialised 0x7f..) | overflow word + 3 counters (0) | host forms: the
// match array, downloaded with the counters | candidates | ncand | st | claimMin, last, removed |
// work list | kTop best | usable counts
struct ResolveScratch {
    int32_t* lf;
    int32_t* ovf;
    int32_t* mp;
    Cand* cands;
    int32_t* ncand;
    int32_t* st;
    int32_t* kw;
    int32_t* work;
    int4* top;
    int32_t* nusable;
};
ResolveScratch carve_resolve(DevScratch& z, int n_cur, int np, int cap, bool host_match) {
    ResolveScratch r;
    r.lf = z.take<int32_t>(2 * (size_t)n_cur);
    r.ovf = z.take<int32_t>(4);
    r.mp = host_match ? z.take<int32_t>(n_cur) : nullptr;
    r.cands = z.take<Cand>((size_t)np * cap);
    r.ncand = z.take<int32_t>(np);
    r.st = z.take<int32_t>(np);
    r.kw = z.take<int32_t>(3 * (size_t)n_cur);
    r.work = z.take<int32_t>(np);
    r.top = z.take<int4>((kTop / 2) * (size_t)np);
    r.nusable = z.take<int32_t>(np);
    return r;
}

// The resolver's arguments over a ResolveScratch.  Host forms: n_pts / n_cur are the counts, the
// matches go to r.mp; device forms: they are the capacities, the counts come from `dims` on the device,
// and the matches and the count go to the caller's mp / out_user.
ResolveArgs make_resolve_args(const ResolveScratch& r, int n_pts, int n_cur, int cap, int local, int check_ori,
                              float nnratio, const uint8_t* observed, const uint8_t* taken0, const float4* cur_kp,
                              const float* last_angle, int32_t* mp, const int32_t* dims, int32_t* out_user) {
    const size_t nk = (size_t)std::max(n_cur, 1);  // (a piece of the scratch is never empty)
    ResolveArgs ra{};
    ra.n_pts = n_pts; ra.n_cur = n_cur; ra.cap = cap; ra.local = local; ra.check_ori = check_ori; ra.nnratio = nnratio;
    ra.cands = r.cands; ra.ncand = r.ncand; ra.observed = observed; ra.taken0 = taken0; ra.cur_kp = cur_kp;
    ra.last_angle = last_angle; ra.overflow = r.ovf; ra.st = r.st;
    ra.claimMin = r.kw; ra.last = r.kw + nk; ra.removed = r.kw + 2 * nk;
    ra.lister = r.lf; ra.fixed = r.lf + nk; ra.work = r.work; ra.top = r.top; ra.nusable = r.nusable;
    ra.lds_keypoints = n_cur <= kResolveLdsKeypoints && resolve_lds_ready() ? 1 : 0;
    ra.mp = mp; ra.out_n = r.ovf + 1; ra.dims = dims; ra.out_user = out_user;
    return ra;
}

// ---- host forms: one upload (inputs, initialised words), the kernels, one download ---------------

// Frame::AssignFeaturesToGrid: cell (round((x - mnMinX) * inv_w), round((y - mnMinY) * inv_h)),
// keypoints in index order inside each cell
void assign_features_to_grid(const orb_frame_view_t* F, std::vector<int32_t>& cell_off, std::vector<int32_t>& cell_idx) {
    const int n = F->n;
    cell_off.assign(kCells + 1, 0);
    std::vector<int32_t> cell_of(n, -1);
    for (int i = 0; i < n; ++i) {
        const orb_keypoint_t& kp = F->kps_un[i];
        const int px = (int)std::round((kp.x - F->min_x) * F->grid_inv_w);
        const int py = (int)std::round((kp.y - F->min_y) * F->grid_inv_h);
        if (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) continue;
        cell_of[i] = px * kGridRows + py;
        cell_off[cell_of[i] + 1]++;
    }
    for (int c = 0; c < kCells; ++c) cell_off[c + 1] += cell_off[c];
    cell_idx.resize(cell_off.back());
    std::vector<int32_t> fill(cell_off.begin(), cell_off.end() - 1);
    for (int i = 0; i < n; ++i)
        if (cell_of[i] >= 0) cell_idx[fill[cell_of[i]]++] = i;
}

// the (x, y, angle, octave bits) rows the kernels read
void pack_kp4(const orb_frame_view_t* F, float4* kp4) {
    for (int i = 0; i < F->n; ++i) {
        const orb_keypoint_t& kp = F->kps_un[i];
        kp4[i].x = kp.x;
        kp4[i].y = kp.y;
        kp4[i].z = kp.angle;
        memcpy(&kp4[i].w, &kp.octave, 4);
    }
}

// One attempt of a host call.  The pinned block h and the device block d share one layout: the
// current frame | the overload's points | ResolveScratch; everything before r.mp goes up in one copy,
// the overflow block and the matches come back in one.
struct HostCall {
    char* d = nullptr;
    char* h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0, cap = 0;
    float4* kp4;
    float* ur;
    uint4* desc;
    uint8_t* taken;  // NULL: the call has none
    int32_t* cell_off;
    int32_t* cell_idx;
    ResolveScratch r;
    // the host mirror of a device piece
    template <class T>
    T* host(T* p) const { return reinterpret_cast<T*>(h + (reinterpret_cast<char*>(p) - d)); }
    // ... filled from a caller's array of n elements
    template <class T, class S>
    void put(T* p, const S* src, size_t n) const { if (n) memcpy(host(p), src, n * sizeof(S)); }
    CurRecords<> cur() const { return CurRecords<>{kp4, ur, desc, cell_off, cell_idx}; }
};

// A host SearchByProjection: the grid, then up to three attempts (a point with more candidates than
// the capacity makes the resolve a no-op, and the call is redone with room for all).  layout(z) carves
// the overload's point arrays; stage(call, cand_args) fills their host mirrors, sets the candidate
// kernel's arguments and returns the resolver's.
template <class CandArgs, class Layout, class Stage>
int host_search(orb_matcher_t m, const orb_frame_view_t* F, const uint8_t* frame_taken, int np, int32_t* match,
                int32_t* n_matches, const char* name, void (*cand_kernel)(const CandArgs), Layout layout, Stage stage) {
    const int n = F->n;
    std::vector<int32_t> cell_off, cell_idx;
    assign_features_to_grid(F, cell_off, cell_idx);
    HostCall c;
    c.cap = 128;
    for (int attempt = 0; attempt < 3; ++attempt) {
        const auto carve = [&](char* base) {
            DevScratch z;
            z.base = base;
            c.kp4 = z.take<float4>(n);
            c.ur = z.take<float>(n);
            c.desc = z.take<uint4>(2 * (size_t)n);
            c.taken = frame_taken ? z.take<uint8_t>(n) : nullptr;
            c.cell_off = z.take<int32_t>(cell_off.size());
            c.cell_idx = z.take<int32_t>(cell_idx.size());
            layout(z);
            c.r = carve_resolve(z, n, np, c.cap, true);
            return z.off;
        };
        if (int rc = orbgpu_matcher_reserve(m, carve(nullptr), &c.d, &c.h, &c.s, &c.check_ori)) return rc;
        carve(c.d);
        pack_kp4(F, c.host(c.kp4));
        if (F->u_right) c.put(c.ur, F->u_right, n);
        c.put(c.desc, F->desc, (size_t)n * 32);
        if (frame_taken) c.put(c.taken, frame_taken, n);
        c.put(c.cell_off, cell_off.data(), cell_off.size());
        c.put(c.cell_idx, cell_idx.data(), cell_idx.size());
        // initialised with the inputs (no fills): the lister / fixed claims (0x7f..) and the overflow
        // word + counters (0), which the one download then reads back with the matches
        const size_t nk = (size_t)std::max(n, 1);
        memset(c.host(c.r.lf), 0x7f, nk * 8);
        memset(c.host(c.r.ovf), 0, 16);
        CandArgs ca;
        const ResolveArgs ra = stage(c, ca);
        bool ok = hipMemcpyAsync(c.d, c.h, reinterpret_cast<char*>(c.r.mp) - c.d, hipMemcpyHostToDevice, c.s) == hipSuccess;
        // candidates and the rounds back to back, one synchronisation
        if (ok) {
            if (np > 0) {
                hipLaunchKernelGGL(cand_kernel, dim3((np + kCandWaves - 1) / kCandWaves), dim3(64 * kCandWaves), 0, c.s, ca);
                hipLaunchKernelGGL(k_resolve_init, dim3((np + 255) / 256), dim3(256), 0, c.s, ra);
            }
            hipLaunchKernelGGL(k_resolve_rounds, dim3(1), dim3(kResolveThreads), ra.lds_keypoints ? 8 * (size_t)n : 0, c.s,
                               ra);
        }
        const size_t back = reinterpret_cast<char*>(c.r.mp + nk) - reinterpret_cast<char*>(c.r.ovf);
        ok = ok && hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(c.host(c.r.ovf), c.r.ovf, back, hipMemcpyDeviceToHost, c.s) == hipSuccess &&
             hipStreamSynchronize(c.s) == hipSuccess;
        if (!ok) return sbp_fail(ORB_ERR_DEVICE, "", name, " failed");
        const int32_t ovf = c.host(c.r.ovf)[0];
        if (ovf > c.cap) {
            c.cap = (ovf + 63) & ~63;
            continue;
        }
        if (n) memcpy(match, c.host(c.r.mp), (size_t)n * 4);
        *n_matches = c.host(c.r.ovf)[1];
        return ORB_OK;
    }
    return sbp_fail(ORB_ERR_INTERNAL, "", name, " candidate capacity");
}

}  // namespace

extern "C" int orb_search_by_projection_frame(orb_matcher_t m, const orb_frame_view_t* cur, const orb_last_points_t* last,
                                              float th, int mono, int32_t* match, int32_t* n_matches) {
    if (!m || !cur || !last || !match || !n_matches || cur->n < 0 || last->n < 0 || cur->nlevels <= 0 ||
        cur->nlevels > kMaxLevels || (cur->n && (!cur->kps_un || !cur->desc)) ||
        (last->n && (!last->valid || !last->observed || !last->xyz || !last->desc || !last->kps_un)) ||
        !cur->scale_factors || !(cur->grid_inv_w > 0) || !(cur->grid_inv_h > 0))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByProjection arguments");
    for (int i = 0; i < last->n; ++i)
        if (last->valid[i] && (last->kps_un[i].octave < 0 || last->kps_un[i].octave >= cur->nlevels))
            return orbgpu_fail(ORB_ERR_ARG, "last-frame octave out of range");
    const int nl = last->n;
    uint8_t *valid, *observed;
    float *xyz, *angle;
    uint4* desc;
    int32_t* octave;
    return host_search<k_proj_candidates_args>(
        m, cur, nullptr, nl, match, n_matches, "SearchByProjection", k_proj_candidates,
        [&](DevScratch& z) {
            valid = z.take<uint8_t>(nl);
            observed = z.take<uint8_t>(nl);
            xyz = z.take<float>(3 * (size_t)nl);
            desc = z.take<uint4>(2 * (size_t)nl);
            octave = z.take<int32_t>(nl);
            angle = z.take<float>(nl);
        },
        [&](const HostCall& c, k_proj_candidates_args& ca) {
            c.put(valid, last->valid, nl);
            c.put(observed, last->observed, nl);
            c.put(xyz, last->xyz, 3 * (size_t)nl);
            c.put(desc, last->desc, (size_t)nl * 32);
            for (int i = 0; i < nl; ++i) {
                c.host(octave)[i] = last->kps_un[i].octave;
                c.host(angle)[i] = last->kps_un[i].angle;
            }
            const ProjParams P = make_proj_params(cur, last->Tcw, th, mono, cur->n, nl, c.cap, c.check_ori);
            ca = k_proj_candidates_args{P, nullptr, valid, xyz, desc, octave, c.cur(), c.r.cands, c.r.ncand, c.r.ovf,
                                        observed, c.r.lf};
            return make_resolve_args(c.r, nl, cur->n, c.cap, 0, c.check_ori, 0.f, observed, nullptr, c.kp4, angle, c.r.mp,
                                     nullptr, nullptr);
        });
}

extern "C" int orb_search_by_projection_local(orb_matcher_t m, const orb_frame_view_t* F, const uint8_t* frame_taken,
                                              const orb_local_points_t* pts, float th, int far_points, float th_far_points,
                                              int32_t* match, int32_t* n_matches) {
    if (!m || !F || !pts || !match || !n_matches || F->n < 0 || pts->n < 0 || F->nlevels <= 0 ||
        F->nlevels > kMaxLevels || (F->n && (!F->kps_un || !F->desc)) || !F->scale_factors ||
        (pts->n && (!pts->track_in_view || !pts->is_bad || !pts->observed || !pts->track_proj || !pts->track_view_cos ||
                    !pts->track_depth || !pts->track_level || !pts->desc)) ||
        !(F->grid_inv_w > 0) || !(F->grid_inv_h > 0))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByProjection(local map) arguments");
    for (int i = 0; i < pts->n; ++i)
        if (pts->track_in_view[i] && (pts->track_level[i] < 0 || pts->track_level[i] >= F->nlevels))
            return orbgpu_fail(ORB_ERR_ARG, "predicted level out of range");
    const int np = pts->n;
    uint8_t *in_view, *bad, *observed;
    float *proj, *view_cos, *depth;
    int32_t* level;
    uint4* desc;
    return host_search<k_lmp_candidates_args>(
        m, F, frame_taken, np, match, n_matches, "SearchByProjection(local map)", k_lmp_candidates,
        [&](DevScratch& z) {
            in_view = z.take<uint8_t>(np);
            bad = z.take<uint8_t>(np);
            observed = z.take<uint8_t>(np);
            proj = z.take<float>(3 * (size_t)np);
            view_cos = z.take<float>(np);
            depth = z.take<float>(np);
            level = z.take<int32_t>(np);
            desc = z.take<uint4>(2 * (size_t)np);
        },
        [&](const HostCall& c, k_lmp_candidates_args& ca) {
            c.put(in_view, pts->track_in_view, np);
            c.put(bad, pts->is_bad, np);
            c.put(observed, pts->observed, np);
            c.put(proj, pts->track_proj, 3 * (size_t)np);
            c.put(view_cos, pts->track_view_cos, np);
            c.put(depth, pts->track_depth, np);
            c.put(level, pts->track_level, np);
            c.put(desc, pts->desc, (size_t)np * 32);
            const float nnratio = orbgpu_matcher_nnratio(m);
            const LocalParams P = make_local_params(F, th, far_points, th_far_points, F->n, np, c.cap, nnratio);
            ca = k_lmp_candidates_args{P, in_view, bad, proj, view_cos, depth, level, desc, c.cur(), c.r.cands, c.r.ncand,
                                       c.r.ovf, observed, c.taken, c.r.lf};
            return make_resolve_args(c.r, np, F->n, c.cap, 1, 0, nnratio, observed, c.taken, c.kp4, nullptr, c.r.mp,
                                     nullptr, nullptr);
        });
}

// ---- device forms: single calls and the tracking chain's batches --------------------------------

namespace {

bool frame_device_ok(const orb_frame_device_t* F) {
    return F && F->kps_un && F->desc && F->n && F->cap > 0 && F->cap <= kResolveLdsKeypoints && F->nlevels > 0 &&
           F->nlevels <= kMaxLevels && F->scale_factors && F->grid_inv_w > 0 && F->grid_inv_h > 0 &&
           (reinterpret_cast<uintptr_t>(F->desc) & 15) == 0;
}

// the frame's grid, built by k_frame_prep: dims ([0] points, [1] keypoints) | kp4 | cells | cell_of
struct GridScratch {
    int32_t* dims;
    float4* kp4;
    int32_t* cell_off;
    int32_t* cell_idx;
    int32_t* cell_of;
};
GridScratch carve_grid(DevScratch& z, int C) {
    GridScratch g;
    g.dims = z.take<int32_t>(2);
    g.kp4 = z.take<float4>(C);
    g.cell_off = z.take<int32_t>(kCells + 1);
    g.cell_idx = z.take<int32_t>(C);
    g.cell_of = z.take<int32_t>(C);
    return g;
}
CurRecords<> cur_records(const orb_frame_device_t* F, const GridScratch& g) {
    return CurRecords<>{g.kp4, F->u_right, (const uint4*)F->desc, g.cell_off, g.cell_idx};
}
// k_frame_prep's arguments; it also initialises the call's scratch words (dims0: ScratchInit)
k_frame_prep_args frame_prep_args(const orb_frame_device_t* F, const GridScratch& g, const ResolveScratch& r,
                                  int32_t* d_match, int dims0) {
    const int C = F->cap;
    const ScratchInit zi{r.lf, 2 * C, d_match, C, r.ovf, g.dims, dims0};
    return k_frame_prep_args{F->kps_un, F->n, C, F->min_x, F->min_y, F->grid_inv_w, F->grid_inv_h, g.kp4,
                             g.cell_off, g.cell_idx, g.cell_of, g.dims + 1, nullptr, zi};
}

// One frame's launches of a device SearchByProjection form, as argument blocks (the single-frame call
// launches them by value, the batch copies them to the device and launches one grid row per frame).
// T: the overload (FrameSearch, LocalSearch below).
template <class T>
struct SbpPlan {
    k_frame_prep_args prep;
    typename T::PrepArgs pprep;
    typename T::CandArgs cand;
    k_resolve_init_args init;
    k_resolve_rounds_args rounds;
};

// What the two overloads do not share: their points and call parameters, the argument check, the
// scratch layout and the plan, the points' prep kernel and the three candidate kernels.
struct FrameSearch {
    using Points = orb_last_points_device_t;
    using PrepArgs = k_last_prep_args;
    using CandArgs = k_proj_candidates_args;
    struct Call {
        float th;
        int mono;
    };
    static constexpr const char* kName = "SearchByProjection";
    static constexpr auto k_prep = k_last_prep;
    static constexpr auto k_prep_b = k_last_prep_b;
    static constexpr auto k_cand = k_proj_candidates;
    static constexpr auto k_cand_t_b = k_proj_candidates_t_b;
    static void launch_cand_l_b(int B, int C, hipStream_t s, const CandArgs* ca, const k_resolve_init_args*) {
        hipLaunchKernelGGL(k_proj_candidates_l_b, dim3(B), dim3(kCandLdsThreads), cand_lds_bytes(C), s, ca);
    }
    static int n_points(const Points* last) { return last->cap; }
    static bool args_ok(orb_matcher_t m, const orb_frame_device_t* cur, const Points* last, const int32_t* d_match,
                        const int32_t* d_n_matches) {
        return m && frame_device_ok(cur) && last && d_match && d_n_matches && last->n && last->cap >= 0 &&
               (last->cap == 0 || (last->valid && last->observed && last->xyz && last->desc && last->kps_un)) &&
               (reinterpret_cast<uintptr_t>(last->desc) & 15) == 0;
    }
    // grid | the last frame's prepared points | candidates and resolver
    struct Scratch {
        GridScratch g;
        uint8_t* valid2;
        int32_t* loct;
        float* lang;
        ResolveScratch r;
    };
    static Scratch carve(DevScratch& z, int C, int NL) {
        Scratch x;
        x.g = carve_grid(z, C);
        x.valid2 = z.take<uint8_t>(NL);
        x.loct = z.take<int32_t>(NL);
        x.lang = z.take<float>(NL);
        x.r = carve_resolve(z, C, NL, C, false);
        return x;
    }
    static void plan(orb_matcher_t m, const orb_frame_device_t* cur, const uint8_t*, const Points* last, const Call& call,
                     int32_t* d_match, int32_t* d_n_matches, char* base, SbpPlan<FrameSearch>& pl) {
        const int C = cur->cap, NL = last->cap;
        DevScratch z;
        z.base = base;
        const Scratch x = carve(z, C, NL);
        // cap = C: a point's candidates are distinct current keypoints, never more than the frame holds
        const ProjParams P = make_proj_params(cur, last->Tcw, call.th, call.mono, 0, 0, C, orbgpu_matcher_check_ori(m));
        pl.prep = frame_prep_args(cur, x.g, x.r, d_match, NL > 0 ? -1 : 0);
        pl.pprep = k_last_prep_args{last->kps_un, last->valid, last->n, NL, cur->nlevels, x.valid2, x.loct, x.lang,
                                    x.g.dims, nullptr};
        pl.cand = k_proj_candidates_args{P, x.g.dims, x.valid2, last->xyz, (const uint4*)last->desc, x.loct,
                                         cur_records(cur, x.g), x.r.cands, x.r.ncand, x.r.ovf, last->observed, x.r.lf};
        pl.init.a = make_resolve_args(x.r, NL, C, C, 0, P.check_ori, 0.f, last->observed, nullptr, x.g.kp4, x.lang,
                                      d_match, x.g.dims, d_n_matches);
        pl.rounds.a = pl.init.a;
    }
};

struct LocalSearch {
    using Points = orb_local_points_device_t;
    using PrepArgs = k_local_prep_args;
    using CandArgs = k_lmp_candidates_args;
    struct Call {
        float th;
        int far_points;
        float th_far_points;
    };
    static constexpr const char* kName = "SearchByProjection(local map)";
    static constexpr auto k_prep = k_local_prep;
    static constexpr auto k_prep_b = k_local_prep_b;
    static constexpr auto k_cand = k_lmp_candidates;
    static constexpr auto k_cand_t_b = k_lmp_candidates_t_b;
    // (ri: the frame's keypoint count, for the gated frames, is in the init block's dims)
    static void launch_cand_l_b(int B, int C, hipStream_t s, const CandArgs* ca, const k_resolve_init_args* ri) {
        hipLaunchKernelGGL(k_lmp_candidates_l_b, dim3(B), dim3(kCandLdsThreads), cand_lds_bytes(C), s, ca, ri);
    }
    static int n_points(const Points* pts) { return pts->n; }
    static bool args_ok(orb_matcher_t m, const orb_frame_device_t* F, const Points* pts, const int32_t* d_match,
                        const int32_t* d_n_matches) {
        return m && frame_device_ok(F) && pts && pts->n >= 0 && d_match && d_n_matches &&
               (pts->n == 0 || (pts->track_in_view && pts->is_bad && pts->observed && pts->track_proj && pts->track_view_cos &&
                                pts->track_depth && pts->track_level && pts->desc)) &&
               (reinterpret_cast<uintptr_t>(pts->desc) & 15) == 0;
    }
    // grid | the points' in-view flags with the level check | candidates and resolver
    struct Scratch {
        GridScratch g;
        uint8_t* iv2;
        ResolveScratch r;
    };
    static Scratch carve(DevScratch& z, int C, int np) {
        Scratch x;
        x.g = carve_grid(z, C);
        x.iv2 = z.take<uint8_t>(np);
        x.r = carve_resolve(z, C, np, C, false);
        return x;
    }
    static void plan(orb_matcher_t m, const orb_frame_device_t* F, const uint8_t* d_frame_taken, const Points* pts,
                     const Call& call, int32_t* d_match, int32_t* d_n_matches, char* base, SbpPlan<LocalSearch>& pl) {
        const int C = F->cap, np = pts->n;
        DevScratch z;
        z.base = base;
        const Scratch x = carve(z, C, np);
        const LocalParams P = make_local_params(F, call.th, call.far_points, call.th_far_points, 0, np, C,
                                                orbgpu_matcher_nnratio(m));
        pl.prep = frame_prep_args(F, x.g, x.r, d_match, np);
        pl.pprep = k_local_prep_args{pts->track_in_view, pts->track_level, np, F->nlevels, x.iv2};
        pl.cand = k_lmp_candidates_args{P, x.iv2, pts->is_bad, pts->track_proj, pts->track_view_cos, pts->track_depth,
                                        pts->track_level, (const uint4*)pts->desc, cur_records(F, x.g), x.r.cands,
                                        x.r.ncand, x.r.ovf, pts->observed, d_frame_taken, x.r.lf};
        pl.init.a = make_resolve_args(x.r, np, C, C, 1, 0, P.nnratio, pts->observed, d_frame_taken, x.g.kp4, nullptr,
                                      d_match, x.g.dims, d_n_matches);
        pl.rounds.a = pl.init.a;
    }
};

template <class T>
size_t sbp_scratch_bytes(int C, int np) {
    DevScratch z;
    T::carve(z, C, np);
    return z.off;
}

// A single device call: the wave candidate kernel.  scratch: the caller's (sbp_scratch_bytes), else
// stream-ordered.
template <class T>
int sbp_device(orb_matcher_t m, const orb_frame_device_t* F, const uint8_t* d_frame_taken, const typename T::Points* pts,
               const typename T::Call& call, int32_t* d_match, int32_t* d_n_matches, void* stream, void* scratch) {
    if (!T::args_ok(m, F, pts, d_match, d_n_matches)) return sbp_fail(ORB_ERR_ARG, "bad ", T::kName, " device arguments");
    hipStream_t s = (hipStream_t)stream;
    const int C = F->cap, np = T::n_points(pts);
    char* base = static_cast<char*>(scratch);
    if (!base && hipMallocAsync(reinterpret_cast<void**>(&base), sbp_scratch_bytes<T>(C, np), s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    SbpPlan<T> pl;
    T::plan(m, F, d_frame_taken, pts, call, d_match, d_n_matches, base, pl);
    hipLaunchKernelGGL(k_frame_prep, dim3(1), dim3(kPrepThreads), 0, s, pl.prep);
    if (np > 0) {
        hipLaunchKernelGGL(T::k_prep, dim3((np + 255) / 256), dim3(256), 0, s, pl.pprep);
        hipLaunchKernelGGL(T::k_cand, dim3((np + kCandWaves - 1) / kCandWaves), dim3(64 * kCandWaves), 0, s, pl.cand);
        hipLaunchKernelGGL(k_resolve_init, dim3((np + 255) / 256), dim3(256), 0, s, pl.init.a);
    }
    hipLaunchKernelGGL(k_resolve_rounds, dim3(1), dim3(kResolveThreads), pl.rounds.a.lds_keypoints ? 8 * (size_t)C : 0, s,
                       pl.rounds.a);
    bool ok = hipGetLastError() == hipSuccess;
    if (!scratch && hipFreeAsync(base, s) != hipSuccess) ok = false;
    return ok ? ORB_OK : sbp_fail(ORB_ERR_DEVICE, "", T::kName, " device failed");
}

// Argument blocks of B frames into one host block (each kernel's B blocks contiguous, 256-B aligned),
// copied once; pointers of each kernel's array on the device.
struct ArgPacker {
    std::vector<char> host;
    template <class T>
    size_t add(const std::vector<T>& v) {
        const size_t off = align256(host.size());
        host.resize(off + v.size() * sizeof(T));
        memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
        return off;
    }
};

// A batch: every stage one launch, frame b on grid row b (the LDS-staged candidates: workgroup b).
// d_frame_taken may be NULL (no frame has flags).
template <class T>
int sbp_batch(orb_matcher_t m, int B, const orb_frame_device_t* const* F, const uint8_t* const* d_frame_taken,
              const typename T::Points* const* pts, const typename T::Call& call, int32_t* const* d_match,
              int32_t* const* d_n_matches, char* scratch, size_t stride, void* d_args, void* h_args, size_t args_cap,
              void* stream) {
    if (B <= 0 || !scratch || !d_args || !h_args) return sbp_fail(ORB_ERR_ARG, "bad ", T::kName, " batch arguments");
    hipStream_t s = (hipStream_t)stream;
    std::vector<k_frame_prep_args> fp(B);
    std::vector<typename T::PrepArgs> pp(B);
    std::vector<typename T::CandArgs> ca(B);
    std::vector<k_resolve_init_args> ri(B);
    std::vector<k_resolve_rounds_args> rr(B);
    int C = -1, maxNp = 0;
    for (int b = 0; b < B; ++b) {
        if (!T::args_ok(m, F[b], pts[b], d_match[b], d_n_matches[b]) || (C >= 0 && F[b]->cap != C) ||
            sbp_scratch_bytes<T>(F[b]->cap, T::n_points(pts[b])) > stride)
            return sbp_fail(ORB_ERR_ARG, "bad ", T::kName, " batch frame (caps must agree, scratch stride)");
        C = F[b]->cap;
        SbpPlan<T> pl;
        T::plan(m, F[b], d_frame_taken ? d_frame_taken[b] : nullptr, pts[b], call, d_match[b], d_n_matches[b],
                scratch + (size_t)b * stride, pl);
        fp[b] = pl.prep; pp[b] = pl.pprep; ca[b] = pl.cand; ri[b] = pl.init; rr[b] = pl.rounds;
        maxNp = std::max(maxNp, T::n_points(pts[b]));
    }
    ArgPacker pk;
    const size_t o_fp = pk.add(fp), o_pp = pk.add(pp), o_ca = pk.add(ca), o_ri = pk.add(ri), o_rr = pk.add(rr);
    if (pk.host.size() > args_cap) return sbp_fail(ORB_ERR_ARG, "", T::kName, " batch: argument area too small");
    char* d = static_cast<char*>(d_args);
    memcpy(h_args, pk.host.data(), pk.host.size());  // pinned staging: the copy reads it when the stream runs it
    if (hipMemcpyAsync(d, h_args, pk.host.size(), hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "batch argument upload failed");
    hipLaunchKernelGGL(k_frame_prep_b, dim3(1, B), dim3(kPrepThreads), 0, s, (const k_frame_prep_args*)(d + o_fp));
    if (maxNp > 0) {  // grids sized for the largest frame; the kernels bound themselves by their own counts
        hipLaunchKernelGGL(T::k_prep_b, dim3((maxNp + 255) / 256, B), dim3(256), 0, s,
                           (const typename T::PrepArgs*)(d + o_pp));
        if (cand_lds_mode(C))
            T::launch_cand_l_b(B, C, s, (const typename T::CandArgs*)(d + o_ca), (const k_resolve_init_args*)(d + o_ri));
        else
            hipLaunchKernelGGL(T::k_cand_t_b, dim3((maxNp + kCandThreads - 1) / kCandThreads, B), dim3(kCandThreads), 0, s,
                               (const typename T::CandArgs*)(d + o_ca));
        hipLaunchKernelGGL(k_resolve_init_b, dim3((maxNp + 255) / 256, B), dim3(256), 0, s,
                           (const k_resolve_init_args*)(d + o_ri));
    }
    hipLaunchKernelGGL(k_resolve_rounds_b, dim3(1, B), dim3(kResolveThreads), rr[0].a.lds_keypoints ? 8 * (size_t)C : 0, s,
                       (const k_resolve_rounds_args*)(d + o_rr));
    return hipGetLastError() == hipSuccess ? ORB_OK : sbp_fail(ORB_ERR_DEVICE, "", T::kName, " batch launch failed");
}

}  // namespace

size_t orbgpu_sbp_frame_scratch_bytes(int C, int NL) { return sbp_scratch_bytes<FrameSearch>(C, NL); }
size_t orbgpu_sbp_local_scratch_bytes(int C, int np) { return sbp_scratch_bytes<LocalSearch>(C, np); }

int orbgpu_sbp_frame_device_scratch(orb_matcher_t m, const orb_frame_device_t* cur, const orb_last_points_device_t* last,
                                    float th, int mono, int32_t* d_match, int32_t* d_n_matches, void* stream,
                                    void* scratch) {
    return sbp_device<FrameSearch>(m, cur, nullptr, last, {th, mono}, d_match, d_n_matches, stream, scratch);
}
int orbgpu_sbp_local_device_scratch(orb_matcher_t m, const orb_frame_device_t* F, const uint8_t* d_frame_taken,
                                    const orb_local_points_device_t* pts, float th, int far_points, float th_far_points,
                                    int32_t* d_match, int32_t* d_n_matches, void* stream, void* scratch) {
    return sbp_device<LocalSearch>(m, F, d_frame_taken, pts, {th, far_points, th_far_points}, d_match, d_n_matches, stream,
                                   scratch);
}

extern "C" int orb_search_by_projection_frame_device(orb_matcher_t m, const orb_frame_device_t* cur,
                                                     const orb_last_points_device_t* last, float th, int mono,
                                                     int32_t* d_match, int32_t* d_n_matches, void* stream) {
    return orbgpu_sbp_frame_device_scratch(m, cur, last, th, mono, d_match, d_n_matches, stream, nullptr);
}
extern "C" int orb_search_by_projection_local_device(orb_matcher_t m, const orb_frame_device_t* F,
                                                     const uint8_t* d_frame_taken, const orb_local_points_device_t* pts,
                                                     float th, int far_points, float th_far_points, int32_t* d_match,
                                                     int32_t* d_n_matches, void* stream) {
    return orbgpu_sbp_local_device_scratch(m, F, d_frame_taken, pts, th, far_points, th_far_points, d_match, d_n_matches,
                                           stream, nullptr);
}

int orbgpu_sbp_frame_batch(orb_matcher_t m, int B, const orb_frame_device_t* const* cur,
                           const orb_last_points_device_t* const* last, float th, int mono, int32_t* const* d_match,
                           int32_t* const* d_n_matches, char* scratch, size_t stride, void* d_args, void* h_args,
                           size_t args_cap, void* stream) {
    return sbp_batch<FrameSearch>(m, B, cur, nullptr, last, {th, mono}, d_match, d_n_matches, scratch, stride, d_args,
                                  h_args, args_cap, stream);
}
int orbgpu_sbp_local_batch(orb_matcher_t m, int B, const orb_frame_device_t* const* F, const uint8_t* const* d_frame_taken,
                           const orb_local_points_device_t* const* pts, float th, int far_points, float th_far_points,
                           int32_t* const* d_match, int32_t* const* d_n_matches, char* scratch, size_t stride,
                           void* d_args, void* h_args, size_t args_cap, void* stream) {
    return sbp_batch<LocalSearch>(m, B, F, d_frame_taken, pts, {th, far_points, th_far_points}, d_match, d_n_matches,
                                  scratch, stride, d_args, h_args, args_cap, stream);
}
