// The 64 x 48 feature grid of a device-resident frame or keyframe (Frame::AssignFeaturesToGrid,
// src/Frame.cc:1418-1440; KeyFrame::mGrid is the same grid of mvKeysUn for NLeft == -1), built on the
// device, and the 256-bit Hamming distance -- shared by SearchByProjection (orb_projection.hip) and
// Fuse (orb_fuse.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orbgpu.h"

namespace {

constexpr int kGridCols = 64, kGridRows = 48;  // include/Frame.h:44-45

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// scratch initialisation done by k_frame_prep (the device forms launch no fills): fill_7f (lister /
// fixed claims) with 0x7f7f7f7f, fill_m1 (the match array) with -1, the 4 overflow / counter words
// zero, and dims[0] = dims0 when dims0 >= 0 (the local-map form's point count)
struct ScratchInit {
    int32_t* fill_7f;
    int n_7f;
    int32_t* fill_m1;
    int n_m1;
    int32_t* zero4;
    int32_t* dims;
    int dims0;
};

// Frame::AssignFeaturesToGrid (src/Frame.cc:1418-1440) on a device frame, one workgroup: cell
// (round((x - mnMinX) inv_w), round((y - mnMinY) inv_h)), keypoints in index order inside each cell
// (counting sort, then each cell's few entries put back in index order); the (x, y, angle, octave) float4
// rows the candidate kernels read; the clamped count into n_out[0] and n_out[1].  The counts, offsets
// and (up to kPrepLds keypoints) the cell lists are built in LDS and written out once; a thread keeps its
// keypoints' cells in registers.
constexpr int kPrepThreads = 1024, kCells = kGridCols * kGridRows, kPrepLds = 8192;
constexpr int kPrepPer = 16;  // keypoints per thread: cap <= 16384
__device__ __forceinline__ void k_frame_prep_body(const orb_keypoint_t* __restrict__ kps,
                                                             const int32_t* __restrict__ n_ptr, int cap, float min_x,
                                                             float min_y, float inv_w, float inv_h,
                                                             float4* __restrict__ kp4, int32_t* __restrict__ cell_off,
                                                             int32_t* __restrict__ cell_idx, int32_t* __restrict__ cell_of,
                                                             int32_t* n_out0, int32_t* n_out1, ScratchInit z) {
    __shared__ int cnt[kCells];       // counts, then fill cursors
    __shared__ int off[kCells + 1];   // cell offsets
    __shared__ int wtot[kPrepThreads / 64];
    __shared__ int sidx[kPrepLds];    // the cell lists (n <= kPrepLds)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = min(max(*n_ptr, 0), cap);
    const bool lds = n <= kPrepLds;
    int* const idx = lds ? sidx : cell_idx;
    // the call's scratch words, in place of fill launches (the later kernels of the call read them)
    for (int i = tid; i < z.n_7f; i += kPrepThreads) z.fill_7f[i] = 0x7f7f7f7f;
    for (int i = tid; i < z.n_m1; i += kPrepThreads) z.fill_m1[i] = -1;
    if (tid < 4) z.zero4[tid] = 0;
    if (tid == 0 && z.dims0 >= 0) z.dims[0] = z.dims0;
    for (int c = tid; c < kCells; c += kPrepThreads) cnt[c] = 0;
    __syncthreads();
    int mine[kPrepPer];
#pragma unroll
    for (int k = 0; k < kPrepPer; ++k) {
        const int i = tid + k * kPrepThreads;
        int cell = -1;
        if (i < n) {
            const orb_keypoint_t kp = kps[i];
            kp4[i] = make_float4(kp.x, kp.y, kp.angle, __int_as_float(kp.octave));
            const int px = (int)roundf((kp.x - min_x) * inv_w);
            const int py = (int)roundf((kp.y - min_y) * inv_h);
            if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) {
                cell = px * kGridRows + py;
                atomicAdd(&cnt[cell], 1);
            }
            cell_of[i] = cell;
        }
        mine[k] = cell;
    }
    __syncthreads();
    // exclusive scan of the 3072 counts: three cells per thread, a wave scan, the wave totals
    constexpr int kPer = kCells / kPrepThreads;
    static_assert(kCells % kPrepThreads == 0, "cells per thread");
    int loc[kPer], sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        loc[q] = sum;
        sum += cnt[tid * kPer + q];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int base = incl - sum;
    for (int w = 0; w < wv; ++w) base += wtot[w];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        off[tid * kPer + q] = base + loc[q];
        cnt[tid * kPer + q] = base + loc[q];  // becomes the fill cursor
    }
    if (tid == kPrepThreads - 1) off[kCells] = base + sum;
    if (tid == 0) {
        *n_out0 = n;
        if (n_out1) *n_out1 = n;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPrepPer; ++k)
        if (mine[k] >= 0) idx[atomicAdd(&cnt[mine[k]], 1)] = tid + k * kPrepThreads;
    __threadfence_block();
    __syncthreads();
    for (int c = tid; c < kCells; c += kPrepThreads) {  // index order inside each cell (insertion sort)
        const int b = off[c], e = off[c + 1];
        for (int a = b + 1; a < e; ++a) {
            const int v = idx[a];
            int k = a;
            for (; k > b && idx[k - 1] > v; --k) idx[k] = idx[k - 1];
            idx[k] = v;
        }
    }
    for (int c = tid; c <= kCells; c += kPrepThreads) cell_off[c] = off[c];
    if (lds) {
        __syncthreads();
        for (int i = tid; i < n; i += kPrepThreads) cell_idx[i] = sidx[i];
    }
}

// Readers of records staged in LDS through address-space-3 pointers, so that a window walk issues
// ds_read (the compiler does not infer the address space through generic pointers otherwise: flat loads)
#define ORB_LDS __attribute__((address_space(3)))
struct LdsF4 {
    const ORB_LDS float* p;
    __device__ float4 operator[](int j) const { const ORB_LDS float* q = p + 4 * j; return make_float4(q[0], q[1], q[2], q[3]); }
};
struct LdsU4 {
    const ORB_LDS uint32_t* p;
    __device__ uint4 operator[](size_t j) const { const ORB_LDS uint32_t* q = p + 4 * j; return make_uint4(q[0], q[1], q[2], q[3]); }
};
template <class T>
struct LdsArr {
    const ORB_LDS T* p;
    __device__ T operator[](int k) const { return p[k]; }
};

}  // namespace
