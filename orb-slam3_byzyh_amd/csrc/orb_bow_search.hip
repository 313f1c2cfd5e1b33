// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) on MI355X (reference
// src/ORBmatcher.cc:260-494), single-camera branch (F.Nleft == -1, mpCamera2 == NULL): the matcher of
// Tracking::TrackReferenceKeyFrame and, once per candidate keyframe, of Tracking::Relocalization.
//
// The reference walks the keyframe's and the frame's DBoW2 FeatureVectors in step and matches only
// inside the nodes both hold.  Inside a node it is a greedy serial walk: the keyframe's features in
// stored order (those with a usable map point), each scanning the node's frame features in stored
// order for the best and second-best Hamming distance (strict `<` updates from 256 / -1 / 256) and
// skipping every frame feature an earlier keyframe feature took.  A frame feature lies in exactly one
// node, so nodes are independent of each other and only the walk inside one is ordered:
//
//   k_bow_match   one wave per (pair, keyframe node): binary-search the node id in the frame's sorted
//                 node ids; then the serial walk over the node's keyframe features, each with the
//                 frame features of the node spread over the 64 lanes (position j of the node's list
//                 on lane j % 64).  A lane keeps (best distance, first position) as one key and its
//                 second distance; a 6-step butterfly merges them: key = min (distance, then position:
//                 the reference's first-index tie rule), second = min(max of the two bests, min of the
//                 two seconds) -- the two smallest of the multiset, as the strict updates leave them.
//                 The taken mark is the match row itself, read and written only by the lane that owns
//                 the position, so no memory ordering between lanes is needed; the first 64 positions'
//                 descriptors and marks stay in registers (a typical node holds ~10 features), later
//                 positions are read from memory, so a node of any size is walked (a degenerate
//                 vocabulary can put the whole frame into one).
//   k_bow_finish  one block per pair: the count and, with mbCheckOrientation, the rotation histogram
//                 with ComputeThreeMaxima (src:467-491, 2336-2378; orb_rot_hist.h).  A match the check
//                 removes stays taken during the walk, as in the reference, because it runs afterwards.
//
// Everything is integer work apart from the ratio test and the angle bin, both single float operations
// (-ffp-contract=off): the results equal the reference's bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbgpu.h"
#include "orb_rot_hist.h"
#include "orbgpu_internal.h"

int orbgpu_matcher_reserve(orb_matcher_t m, size_t bytes, char** d_buf, char** h_buf, hipStream_t* stream,
                           int* check_ori);
int orbgpu_matcher_upload_slot(orb_matcher_t m, size_t bytes, char** h);
int orbgpu_matcher_upload_mark(orb_matcher_t m, hipStream_t s);
float orbgpu_matcher_nnratio(orb_matcher_t m);
int orbgpu_matcher_check_ori(orb_matcher_t m);

namespace {

constexpr int kThLow = 50;  // src/ORBmatcher.cc:37
constexpr int kWaves = 4;
constexpr int kPosBits = 20;  // a node position inside the (distance, position) key
constexpr int kMaxCap = 1 << kPosBits;
constexpr uint32_t kPosMask = (1u << kPosBits) - 1;
constexpr uint32_t kNoKey = (256u << kPosBits) | kPosMask;  // bestDist1 = 256, bestIdxF = -1

// One side of a search (a keyframe or a frame), device pointers.  The counts are read on the device.
struct BowSide {
    const orb_keypoint_t* kps;
    const uint4* desc;
    const int32_t* n;
    const uint8_t* ok;  // keyframe: map point usable (non-NULL and not isBad()); NULL = none is
    const int32_t* fv_node;
    const int32_t* fv_begin;
    const int32_t* fv_feat;
    const int32_t* n_nodes;
    int32_t cap, pad;
};

// A side whose producer flagged it (count above the capacity, negative FeatureVector size) fails.
__device__ __forceinline__ bool side_failed(const BowSide& s) {
    const int c = *s.n, nn = *s.n_nodes;
    return c < 0 || c > s.cap || nn < 0 || nn > s.cap;
}

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// sides: [the pairs' keyframes | the frames from fbase on]; pair p searches frame pair_frame[p] (0
// without the table).  matches row p starts at p * mstride and is -1 on entry.
__global__ __launch_bounds__(64 * kWaves) void k_bow_match(const BowSide* __restrict__ sides,
                                                         const int32_t* __restrict__ pair_frame, int fbase,
                                                         float nnratio, int mstride, int32_t* matches) {
    const int lane = threadIdx.x & 63;
    const int node = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    const BowSide K = sides[p], F = sides[fbase + (pair_frame ? pair_frame[p] : 0)];
    if (side_failed(K) || side_failed(F)) return;
    const int nK = *K.n, nF = min(*F.n, mstride), nnK = *K.n_nodes, nnF = *F.n_nodes;
    if (node >= nnK || !K.ok) return;
    // the merge walk with lower_bound (src:290-465) visits exactly the node ids both maps hold
    const uint32_t id = (uint32_t)K.fv_node[node];
    int lo = 0, hi = nnF;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)F.fv_node[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nnF || (uint32_t)F.fv_node[lo] != id) return;
    const int b1 = min(max(K.fv_begin[node], 0), K.cap), e1 = min(max(K.fv_begin[node + 1], b1), K.cap);
    const int b2 = min(max(F.fv_begin[lo], 0), F.cap), e2 = min(max(F.fv_begin[lo + 1], b2), F.cap);
    const int nf = e2 - b2;
    if (e1 <= b1 || nf <= 0) return;
    int32_t* m = matches + (size_t)p * mstride;
    // the node's first 64 frame features: one per lane, descriptor and taken mark in registers
    int idx0 = -1;
    bool free0 = false;
    uint4 f0a = {}, f0b = {};
    if (lane < nf) {
        idx0 = F.fv_feat[b2 + lane];
        if ((unsigned)idx0 < (unsigned)nF) {
            f0a = F.desc[2 * (size_t)idx0];
            f0b = F.desc[2 * (size_t)idx0 + 1];
            free0 = true;
        }
    }
    for (int base = b1; base < e1; base += 64) {  // the keyframe's features of the node, 64 at a time
        int kidx = -1;
        bool usable = false;
        if (base + lane < e1) {
            kidx = K.fv_feat[base + lane];
            usable = (unsigned)kidx < (unsigned)nK && K.ok[kidx] != 0;  // pMP && !pMP->isBad() (src:307-313)
        }
        unsigned long long todo = __ballot(usable);
        while (todo) {  // ... in stored order, one after the other (src:301)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int real_kf = __shfl(kidx, src, 64);
            const uint4 ka = K.desc[2 * (size_t)real_kf], kb = K.desc[2 * (size_t)real_kf + 1];
            uint32_t key = kNoKey;
            int d2 = 256;
            if (free0) key = ((uint32_t)hamming(ka, kb, f0a, f0b) << kPosBits) | (uint32_t)lane;
            for (int j = lane + 64; j < nf; j += 64) {  // this lane's later positions, ascending
                const int idx = F.fv_feat[b2 + j];
                if ((unsigned)idx >= (unsigned)nF || m[idx] >= 0) continue;  // vpMapPointMatches[realIdxF] (src:332)
                const int d = hamming(ka, kb, F.desc[2 * (size_t)idx], F.desc[2 * (size_t)idx + 1]);
                const int d1 = (int)(key >> kPosBits);
                if (d < d1) {  // src:341-351
                    d2 = d1;
                    key = ((uint32_t)d << kPosBits) | (uint32_t)j;
                } else if (d < d2) {
                    d2 = d;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t okey = (uint32_t)__shfl_xor((int)key, off, 64);
                const int od2 = __shfl_xor(d2, off, 64);
                d2 = min(max((int)(key >> kPosBits), (int)(okey >> kPosBits)), min(d2, od2));
                key = min(key, okey);
            }
            const int best1 = (int)(key >> kPosBits);
            if (best1 <= kThLow && (float)best1 < nnratio * (float)d2) {  // src:385-391
                const int pos = (int)(key & kPosMask);
                if ((pos & 63) == lane) {  // the owner of the position marks it and writes the match
                    if (pos < 64) {
                        m[idx0] = real_kf;
                        free0 = false;
                    } else {
                        m[F.fv_feat[b2 + pos]] = real_kf;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bow_finish(const BowSide* __restrict__ sides,
                                                    const int32_t* __restrict__ pair_frame, int fbase, int check_ori,
                                                    int mstride, int32_t* __restrict__ matches,
                                                    int32_t* __restrict__ counts) {
    __shared__ int hist[kOrbHistoLength];
    __shared__ int keep[3];
    __shared__ int total;
    const int p = blockIdx.x;
    const BowSide K = sides[p], F = sides[fbase + (pair_frame ? pair_frame[p] : 0)];
    if (side_failed(K) || side_failed(F)) {  // no matches (the row stays -1), the pair reports the failure
        if (threadIdx.x == 0) counts[p] = ORB_ERR_CAPACITY;
        return;
    }
    const int nF = min(*F.n, mstride), nK = *K.n;
    int32_t* m = matches + (size_t)p * mstride;
    if (threadIdx.x < kOrbHistoLength) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < nF; i += blockDim.x) {
        const int j = m[i];
        if (j < 0 || j >= nK) continue;
        ++cnt;
        // kp = pKF->mvKeysUn[realIdxKF], Fkp = F.mvKeys[bestIdxF] (src:394-413; the angle is the same in
        // mvKeys and mvKeysUn)
        if (check_ori) {
            const int bin = orb_rot_bin(K.kps[j].angle, F.kps[i].angle);
            if (bin >= 0 && bin < kOrbHistoLength) atomicAdd(&hist[bin], 1);
        }
    }
    if (check_ori) {
        __syncthreads();
        if (threadIdx.x == 0) orb_three_maxima(hist, keep);
        __syncthreads();
        for (int i = threadIdx.x; i < nF; i += blockDim.x) {
            const int j = m[i];
            if (j < 0 || j >= nK) continue;
            const int bin = orb_rot_bin(K.kps[j].angle, F.kps[i].angle);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {  // src:478-490
                m[i] = -1;
                --cnt;
            }
        }
    }
    atomicAdd(&total, cnt);
    __syncthreads();
    if (threadIdx.x == 0) counts[p] = total;
}

// A host view as SearchByBoW reads it: n, keypoints, descriptors and the FeatureVector, in which a
// feature is listed once (a DBoW2 FeatureVector) and every index is below n.
bool check_view(const orb_kf_view_t* v) {
    if (!v || v->n < 0 || v->n >= kMaxCap || v->n_nodes < 0) return false;
    if (v->n > 0 && (!v->kps_un || !v->desc)) return false;
    if (v->n_nodes > 0 && (!v->fv_node || !v->fv_offset || !v->fv_index)) return false;
    if (v->n_nodes > 0 && v->fv_offset[0] != 0) return false;
    for (int i = 0; i < v->n_nodes; ++i) {
        if (v->fv_offset[i + 1] < v->fv_offset[i]) return false;
        if (i > 0 && v->fv_node[i] <= v->fv_node[i - 1]) return false;
    }
    const int nidx = v->n_nodes > 0 ? v->fv_offset[v->n_nodes] : 0;
    if (nidx > v->n) return false;
    std::vector<uint8_t> seen(v->n, 0);
    for (int i = 0; i < nidx; ++i) {
        const int j = v->fv_index[i];
        if (j < 0 || j >= v->n || seen[j]) return false;
        seen[j] = 1;
    }
    return true;
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

void launch(const BowSide* d_sides, const int32_t* d_pair_frame, int n_pairs, int max_nodes, float nnratio, int check_ori,
            int mstride, int32_t* d_matches, int32_t* d_counts, hipStream_t s) {
    if (max_nodes > 0)
        hipLaunchKernelGGL(k_bow_match, dim3((max_nodes + kWaves - 1) / kWaves, n_pairs), dim3(64 * kWaves), 0, s, d_sides,
                           d_pair_frame, n_pairs, nnratio, mstride, d_matches);
    hipLaunchKernelGGL(k_bow_finish, dim3(n_pairs), dim3(256), 0, s, d_sides, d_pair_frame, n_pairs, check_ori, mstride,
                       d_matches, d_counts);
}

}  // namespace

extern "C" {

int orb_search_by_bow(orb_matcher_t m, const orb_kf_view_t* kfs, const uint8_t* const* point_ok, int n_kfs,
                      const orb_kf_view_t* frame, int32_t* matches, int32_t* n_matches) {
    if (!m || !frame || n_kfs < 0 || n_kfs > 65535 || (n_kfs > 0 && (!kfs || !n_matches)))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByBoW arguments");
    if (n_kfs == 0) return ORB_OK;
    if (!check_view(frame)) return orbgpu_fail(ORB_ERR_ARG, "invalid frame view");
    if (frame->n > 0 && !matches) return orbgpu_fail(ORB_ERR_ARG, "null matches");
    for (int p = 0; p < n_kfs; ++p)
        if (!check_view(&kfs[p])) return orbgpu_fail(ORB_ERR_ARG, "invalid keyframe view");

    // packed layout (one H2D copy): sides | per side: counts, kps, desc, flags, nodes, csr, idx | matches;
    // then the counts (output only)
    const int ns = n_kfs + 1;
    auto view = [&](int k) -> const orb_kf_view_t& { return k < n_kfs ? kfs[k] : *frame; };
    struct Off { size_t cnt, kps, desc, ok, node, csr, idx; };
    std::vector<Off> offs(ns);
    size_t off = align256(ns * sizeof(BowSide));
    int max_nodes = 0;
    for (int k = 0; k < ns; ++k) {
        const orb_kf_view_t& v = view(k);
        const size_t nidx = v.n_nodes ? v.fv_offset[v.n_nodes] : 0;
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 8);
        o.kps = off; off = align256(off + (size_t)v.n * sizeof(orb_keypoint_t));
        o.desc = off; off = align256(off + (size_t)v.n * 32);
        o.ok = off; off = align256(off + (size_t)v.n);
        o.node = off; off = align256(off + (size_t)v.n_nodes * 4);
        o.csr = off; off = align256(off + ((size_t)v.n_nodes + 1) * 4);
        o.idx = off; off = align256(off + nidx * 4);
        if (k < n_kfs) max_nodes = std::max(max_nodes, v.n_nodes);
    }
    const size_t mbytes = (size_t)n_kfs * frame->n * 4;
    const size_t o_match = off; off = align256(off + mbytes);
    const size_t in_bytes = off;
    const size_t o_cnt = off; off = align256(off + (size_t)n_kfs * 4);
    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int rc = orbgpu_matcher_reserve(m, off, &d, &h, &s, &check_ori)) return rc;

    auto* sides = reinterpret_cast<BowSide*>(h);
    for (int k = 0; k < ns; ++k) {
        const orb_kf_view_t& v = view(k);
        const Off& o = offs[k];
        const size_t nidx = v.n_nodes ? v.fv_offset[v.n_nodes] : 0;
        auto* cnt = reinterpret_cast<int32_t*>(h + o.cnt);
        cnt[0] = v.n;
        cnt[1] = v.n_nodes;
        if (v.n) {
            memcpy(h + o.kps, v.kps_un, (size_t)v.n * sizeof(orb_keypoint_t));
            memcpy(h + o.desc, v.desc, (size_t)v.n * 32);
        }
        // the usable flags: the caller's array for this keyframe, else the view's has_mappoint
        const uint8_t* ok = k < n_kfs ? (point_ok && point_ok[k] ? point_ok[k] : v.has_mappoint) : nullptr;
        if (ok && v.n) memcpy(h + o.ok, ok, (size_t)v.n);
        if (v.n_nodes) {
            memcpy(h + o.node, v.fv_node, (size_t)v.n_nodes * 4);
            memcpy(h + o.csr, v.fv_offset, ((size_t)v.n_nodes + 1) * 4);
            memcpy(h + o.idx, v.fv_index, nidx * 4);
        } else {
            *reinterpret_cast<int32_t*>(h + o.csr) = 0;
        }
        sides[k] = BowSide{reinterpret_cast<const orb_keypoint_t*>(d + o.kps), reinterpret_cast<const uint4*>(d + o.desc),
                           reinterpret_cast<const int32_t*>(d + o.cnt), ok ? reinterpret_cast<const uint8_t*>(d + o.ok) : nullptr,
                           reinterpret_cast<const int32_t*>(d + o.node), reinterpret_cast<const int32_t*>(d + o.csr),
                           reinterpret_cast<const int32_t*>(d + o.idx), reinterpret_cast<const int32_t*>(d + o.cnt) + 1,
                           std::max(v.n, v.n_nodes), 0};
    }
    memset(h + o_match, 0xFF, mbytes);
    bool ok = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        launch(reinterpret_cast<const BowSide*>(d), nullptr, n_kfs, max_nodes, orbgpu_matcher_nnratio(m), check_ori,
               frame->n, reinterpret_cast<int32_t*>(d + o_match), reinterpret_cast<int32_t*>(d + o_cnt), s);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(h + o_match, d + o_match, o_cnt + (size_t)n_kfs * 4 - o_match, hipMemcpyDeviceToHost, s) ==
                   hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return orbgpu_fail(ORB_ERR_DEVICE, "SearchByBoW device error");
    if (mbytes) memcpy(matches, h + o_match, mbytes);
    memcpy(n_matches, h + o_cnt, (size_t)n_kfs * 4);
    return ORB_OK;
}

int orb_search_by_bow_device(orb_matcher_t m, const orb_kf_device_t* kfs, const uint8_t* const* d_point_ok, int n_pairs,
                             const orb_kf_device_t* frames, int n_frames, const int32_t* pair_frame,
                             int32_t* d_matches, int32_t* d_n_matches, void* stream) {
    if (!m || n_pairs < 0 || n_pairs > 65535 || n_frames <= 0 || !frames ||
        (n_pairs > 0 && (!kfs || !d_matches || !d_n_matches)))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByBoW arguments");
    if (n_pairs == 0) return ORB_OK;
    auto bad = [](const orb_kf_device_t& k) {
        return k.cap <= 0 || k.cap >= kMaxCap || !k.kps || !k.desc || !k.n || !k.fv_node || !k.fv_begin || !k.fv_feat ||
               !k.n_nodes || (reinterpret_cast<uintptr_t>(k.desc) & 15) != 0;
    };
    int C = 0, CK = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (bad(frames[f])) return orbgpu_fail(ORB_ERR_ARG, "invalid frame device view");
        C = std::max(C, frames[f].cap);
    }
    for (int p = 0; p < n_pairs; ++p) {
        if (bad(kfs[p])) return orbgpu_fail(ORB_ERR_ARG, "invalid keyframe device view");
        if (pair_frame && (pair_frame[p] < 0 || pair_frame[p] >= n_frames)) return orbgpu_fail(ORB_ERR_ARG, "bad pair_frame");
        CK = std::max(CK, kfs[p].cap);
    }
    hipStream_t s = (hipStream_t)stream;
    const int ns = n_pairs + n_frames;
    // upload: BowSide [the pairs' keyframes | the frames] | frame index per pair
    const size_t o_pf = align256(ns * sizeof(BowSide));
    const size_t bytes = o_pf + align256(4 * (size_t)n_pairs);
    char* h = nullptr;
    if (int rc = orbgpu_matcher_upload_slot(m, bytes, &h)) return rc;
    auto* sides = reinterpret_cast<BowSide*>(h);
    auto* pf = reinterpret_cast<int32_t*>(h + o_pf);
    for (int k = 0; k < ns; ++k) {
        const orb_kf_device_t& v = k < n_pairs ? kfs[k] : frames[k - n_pairs];
        const uint8_t* ok = k < n_pairs ? (d_point_ok && d_point_ok[k] ? d_point_ok[k] : v.has_mappoint) : nullptr;
        sides[k] = BowSide{v.kps, reinterpret_cast<const uint4*>(v.desc), v.n, ok, v.fv_node, v.fv_begin, v.fv_feat,
                           v.n_nodes, v.cap, 0};
    }
    for (int p = 0; p < n_pairs; ++p) pf[p] = pair_frame ? pair_frame[p] : 0;
    // device copy, stream-ordered (calls on different streams do not share it)
    char* d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d), bytes, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    bool ok = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
              orbgpu_matcher_upload_mark(m, s) == ORB_OK &&
              hipMemsetAsync(d_matches, 0xFF, (size_t)n_pairs * C * 4, s) == hipSuccess;
    if (ok) {  // node < *n_nodes <= cap: the grid covers the capacity, waves past the count return
        launch(reinterpret_cast<const BowSide*>(d), reinterpret_cast<const int32_t*>(d + o_pf), n_pairs, CK,
               orbgpu_matcher_nnratio(m), orbgpu_matcher_check_ori(m), C, d_matches, d_n_matches, s);
        ok = hipGetLastError() == hipSuccess;
    }
    if (hipFreeAsync(d, s) != hipSuccess) ok = false;
    return ok ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "SearchByBoW device error");
}

}  // extern "C"

// ---- ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (reference src/ORBmatcher.cc:893-1044) ----
// Loop closing's matcher of the current keyframe against each keyframe of a candidate's window
// (src/LoopClosing.cc:840-851).  The same node walk as above with three differences: the second side has a
// map-point mask too (ok2: vpMapPoints2[idx2] non-NULL and not isBad(), src:960-967), the result is indexed
// by the first side's features (vpMatches12[idx1]), and the acceptance is bestDist1 < TH_LOW, strict
// (src:986).  The claim mark (vbMatched2) therefore lives on the second side:
//
//   k_bowkf_match   one wave per (pair, KF1 node), the serial walk over the node's KF1 features with the
//                   node's KF2 features on the lanes, as k_bow_match.  A KF2 feature lies in exactly one node
//                   and position j of a node's list belongs to lane j % 64, so a claim is read and written by
//                   one lane of one wave only: the first 64 positions keep it in a register, later positions
//                   in the pair's byte row claimed[p * cstride + idx2] (zero on entry).  The owner of the
//                   winning position also writes matches12[idx1] = idx2.
//   k_bowkf_finish  one block per pair: the count and the rotation histogram over idx1 (src:993-1003,
//                   1023-1041).  The claim row is not touched: a match the check removes stays claimed.
namespace {

// sides: [the kf1s | the pairs' second keyframes from base2 on]; pair p searches kf1 pair_kf1[p] (0 without
// the table).  matches12 row p starts at p * mstride and is -1 on entry.
__global__ __launch_bounds__(64 * kWaves) void k_bowkf_match(const BowSide* __restrict__ sides,
                                                           const int32_t* __restrict__ pair_kf1, int base2,
                                                           float nnratio, int mstride, int32_t* matches12,
                                                           int cstride, uint8_t* claimed) {
    const int lane = threadIdx.x & 63;
    const int node = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    const BowSide K = sides[pair_kf1 ? pair_kf1[p] : 0], F = sides[base2 + p];
    if (side_failed(K) || side_failed(F)) return;
    const int nK = min(*K.n, mstride), nF = min(*F.n, cstride), nnK = *K.n_nodes, nnF = *F.n_nodes;
    if (node >= nnK || !K.ok || !F.ok) return;
    const uint32_t id = (uint32_t)K.fv_node[node];  // the node ids both maps hold (src:926-1020)
    int lo = 0, hi = nnF;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)F.fv_node[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nnF || (uint32_t)F.fv_node[lo] != id) return;
    const int b1 = min(max(K.fv_begin[node], 0), K.cap), e1 = min(max(K.fv_begin[node + 1], b1), K.cap);
    const int b2 = min(max(F.fv_begin[lo], 0), F.cap), e2 = min(max(F.fv_begin[lo + 1], b2), F.cap);
    const int nf = e2 - b2;
    if (e1 <= b1 || nf <= 0) return;
    int32_t* m = matches12 + (size_t)p * mstride;
    uint8_t* cl = claimed + (size_t)p * cstride;
    // the node's first 64 KF2 features: one per lane, descriptor and claim in registers
    int idx0 = -1;
    bool free0 = false;
    uint4 f0a = {}, f0b = {};
    if (lane < nf) {
        idx0 = F.fv_feat[b2 + lane];
        if ((unsigned)idx0 < (unsigned)nF && F.ok[idx0] != 0) {  // pMP2 && !pMP2->isBad() (src:960-967)
            f0a = F.desc[2 * (size_t)idx0];
            f0b = F.desc[2 * (size_t)idx0 + 1];
            free0 = true;
        }
    }
    for (int base = b1; base < e1; base += 64) {  // KF1's features of the node, 64 at a time
        int kidx = -1;
        bool usable = false;
        if (base + lane < e1) {
            kidx = K.fv_feat[base + lane];
            usable = (unsigned)kidx < (unsigned)nK && K.ok[kidx] != 0;  // pMP1 && !pMP1->isBad() (src:939-943)
        }
        unsigned long long todo = __ballot(usable);
        while (todo) {  // ... in stored order, one after the other (src:932)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int idx1 = __shfl(kidx, src, 64);
            const uint4 ka = K.desc[2 * (size_t)idx1], kb = K.desc[2 * (size_t)idx1 + 1];
            uint32_t key = kNoKey;
            int d2 = 256;
            if (free0) key = ((uint32_t)hamming(ka, kb, f0a, f0b) << kPosBits) | (uint32_t)lane;
            for (int j = lane + 64; j < nf; j += 64) {  // this lane's later positions, ascending
                const int idx = F.fv_feat[b2 + j];
                if ((unsigned)idx >= (unsigned)nF || F.ok[idx] == 0 || cl[idx] != 0) continue;  // src:963-967
                const int d = hamming(ka, kb, F.desc[2 * (size_t)idx], F.desc[2 * (size_t)idx + 1]);
                const int d1 = (int)(key >> kPosBits);
                if (d < d1) {  // src:973-982
                    d2 = d1;
                    key = ((uint32_t)d << kPosBits) | (uint32_t)j;
                } else if (d < d2) {
                    d2 = d;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t okey = (uint32_t)__shfl_xor((int)key, off, 64);
                const int od2 = __shfl_xor(d2, off, 64);
                d2 = min(max((int)(key >> kPosBits), (int)(okey >> kPosBits)), min(d2, od2));
                key = min(key, okey);
            }
            const int best1 = (int)(key >> kPosBits);
            if (best1 < kThLow && (float)best1 < nnratio * (float)d2) {  // src:986-991
                const int pos = (int)(key & kPosMask);
                if ((pos & 63) == lane) {  // the owner of the position claims it and writes the match
                    if (pos < 64) {
                        m[idx1] = idx0;
                        free0 = false;
                    } else {
                        const int idx = F.fv_feat[b2 + pos];
                        m[idx1] = idx;
                        cl[idx] = 1;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_bowkf_finish(const BowSide* __restrict__ sides,
                                                      const int32_t* __restrict__ pair_kf1, int base2, int check_ori,
                                                      int mstride, int cstride, int32_t* __restrict__ matches12,
                                                      int32_t* __restrict__ counts) {
    __shared__ int hist[kOrbHistoLength];
    __shared__ int keep[3];
    __shared__ int total;
    const int p = blockIdx.x;
    const BowSide K = sides[pair_kf1 ? pair_kf1[p] : 0], F = sides[base2 + p];
    if (side_failed(K) || side_failed(F)) {  // no matches (the row stays -1), the pair reports the failure
        if (threadIdx.x == 0) counts[p] = ORB_ERR_CAPACITY;
        return;
    }
    const int n1 = min(*K.n, mstride), n2 = min(*F.n, cstride);
    int32_t* m = matches12 + (size_t)p * mstride;
    if (threadIdx.x < kOrbHistoLength) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < n1; i += blockDim.x) {
        const int j = m[i];
        if (j < 0 || j >= n2) continue;
        ++cnt;
        if (check_ori) {  // vKeysUn1[idx1].angle - vKeysUn2[bestIdx2].angle, rotHist[bin].push_back(idx1) (src:995-1002)
            const int bin = orb_rot_bin(K.kps[i].angle, F.kps[j].angle);
            if (bin >= 0 && bin < kOrbHistoLength) atomicAdd(&hist[bin], 1);
        }
    }
    if (check_ori) {
        __syncthreads();
        if (threadIdx.x == 0) orb_three_maxima(hist, keep);
        __syncthreads();
        for (int i = threadIdx.x; i < n1; i += blockDim.x) {
            const int j = m[i];
            if (j < 0 || j >= n2) continue;
            const int bin = orb_rot_bin(K.kps[i].angle, F.kps[j].angle);
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {  // src:1031-1040
                m[i] = -1;
                --cnt;
            }
        }
    }
    atomicAdd(&total, cnt);
    __syncthreads();
    if (threadIdx.x == 0) counts[p] = total;
}

// -1 rows, zero claims, the two kernels: four stream operations whatever n_pairs is
bool launch_kf(const BowSide* d_sides, const int32_t* d_pair_kf1, int base2, int n_pairs, int max_nodes, float nnratio,
               int check_ori, int mstride, int32_t* d_matches12, int cstride, uint8_t* d_claimed, int32_t* d_counts,
               hipStream_t s) {
    if (mstride > 0 && hipMemsetAsync(d_matches12, 0xFF, (size_t)n_pairs * mstride * 4, s) != hipSuccess) return false;
    if (hipMemsetAsync(d_claimed, 0, (size_t)n_pairs * cstride, s) != hipSuccess) return false;
    if (max_nodes > 0)
        hipLaunchKernelGGL(k_bowkf_match, dim3((max_nodes + kWaves - 1) / kWaves, n_pairs), dim3(64 * kWaves), 0, s,
                           d_sides, d_pair_kf1, base2, nnratio, mstride, d_matches12, cstride, d_claimed);
    hipLaunchKernelGGL(k_bowkf_finish, dim3(n_pairs), dim3(256), 0, s, d_sides, d_pair_kf1, base2, check_ori, mstride,
                       cstride, d_matches12, d_counts);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

extern "C" {

int orb_search_by_bow_kf(orb_matcher_t m, const orb_kf_view_t* kf1, const uint8_t* ok1, const orb_kf_view_t* kf2s,
                         const uint8_t* const* ok2s, int n_pairs, int32_t* matches12, int32_t* n_matches) {
    if (!m || !kf1 || n_pairs < 0 || n_pairs > 65535 || (n_pairs > 0 && (!kf2s || !n_matches)))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByBoW(KF, KF) arguments");
    if (n_pairs == 0) return ORB_OK;
    if (!check_view(kf1)) return orbgpu_fail(ORB_ERR_ARG, "invalid keyframe view");
    if (kf1->n > 0 && !matches12) return orbgpu_fail(ORB_ERR_ARG, "null matches12");
    for (int p = 0; p < n_pairs; ++p)
        if (!check_view(&kf2s[p])) return orbgpu_fail(ORB_ERR_ARG, "invalid second keyframe view");

    // packed layout (one H2D copy): sides [kf1 | kf2s] | per side: counts, kps, desc, flags, nodes, csr, idx;
    // then, device only: the claim rows; then the outputs: matches12 | counts
    const int ns = n_pairs + 1;
    auto view = [&](int k) -> const orb_kf_view_t& { return k == 0 ? *kf1 : kf2s[k - 1]; };
    struct Off { size_t cnt, kps, desc, ok, node, csr, idx; };
    std::vector<Off> offs(ns);
    size_t off = align256(ns * sizeof(BowSide));
    int C2 = 1;
    for (int k = 0; k < ns; ++k) {
        const orb_kf_view_t& v = view(k);
        const size_t nidx = v.n_nodes ? v.fv_offset[v.n_nodes] : 0;
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 8);
        o.kps = off; off = align256(off + (size_t)v.n * sizeof(orb_keypoint_t));
        o.desc = off; off = align256(off + (size_t)v.n * 32);
        o.ok = off; off = align256(off + (size_t)v.n);
        o.node = off; off = align256(off + (size_t)v.n_nodes * 4);
        o.csr = off; off = align256(off + ((size_t)v.n_nodes + 1) * 4);
        o.idx = off; off = align256(off + nidx * 4);
        if (k > 0) C2 = std::max(C2, v.n);
    }
    const size_t in_bytes = off;
    const size_t o_claim = off; off = align256(off + (size_t)n_pairs * C2);
    const size_t mbytes = (size_t)n_pairs * kf1->n * 4;
    const size_t o_match = off; off = align256(off + mbytes);
    const size_t o_cnt = off; off = align256(off + (size_t)n_pairs * 4);
    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int rc = orbgpu_matcher_reserve(m, off, &d, &h, &s, &check_ori)) return rc;

    auto* sides = reinterpret_cast<BowSide*>(h);
    for (int k = 0; k < ns; ++k) {
        const orb_kf_view_t& v = view(k);
        const Off& o = offs[k];
        const size_t nidx = v.n_nodes ? v.fv_offset[v.n_nodes] : 0;
        auto* cnt = reinterpret_cast<int32_t*>(h + o.cnt);
        cnt[0] = v.n;
        cnt[1] = v.n_nodes;
        if (v.n) {
            memcpy(h + o.kps, v.kps_un, (size_t)v.n * sizeof(orb_keypoint_t));
            memcpy(h + o.desc, v.desc, (size_t)v.n * 32);
        }
        // the usable flags: the caller's array for this side, else the view's has_mappoint
        const uint8_t* ok = k == 0 ? ok1 : (ok2s ? ok2s[k - 1] : nullptr);
        if (!ok) ok = v.has_mappoint;
        if (ok && v.n) memcpy(h + o.ok, ok, (size_t)v.n);
        if (v.n_nodes) {
            memcpy(h + o.node, v.fv_node, (size_t)v.n_nodes * 4);
            memcpy(h + o.csr, v.fv_offset, ((size_t)v.n_nodes + 1) * 4);
            memcpy(h + o.idx, v.fv_index, nidx * 4);
        } else {
            *reinterpret_cast<int32_t*>(h + o.csr) = 0;
        }
        sides[k] = BowSide{reinterpret_cast<const orb_keypoint_t*>(d + o.kps), reinterpret_cast<const uint4*>(d + o.desc),
                           reinterpret_cast<const int32_t*>(d + o.cnt), ok ? reinterpret_cast<const uint8_t*>(d + o.ok) : nullptr,
                           reinterpret_cast<const int32_t*>(d + o.node), reinterpret_cast<const int32_t*>(d + o.csr),
                           reinterpret_cast<const int32_t*>(d + o.idx), reinterpret_cast<const int32_t*>(d + o.cnt) + 1,
                           std::max(v.n, v.n_nodes), 0};
    }
    bool ok = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    // (mstride = kf1->n may be 0: then no wave finds a usable feature and no row is written)
    ok = ok && launch_kf(reinterpret_cast<const BowSide*>(d), nullptr, 1, n_pairs, kf1->n_nodes, orbgpu_matcher_nnratio(m),
                         check_ori, kf1->n, reinterpret_cast<int32_t*>(d + o_match), C2,
                         reinterpret_cast<uint8_t*>(d + o_claim), reinterpret_cast<int32_t*>(d + o_cnt), s);
    ok = ok && hipMemcpyAsync(h + o_match, d + o_match, o_cnt + (size_t)n_pairs * 4 - o_match, hipMemcpyDeviceToHost, s) ==
                   hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return orbgpu_fail(ORB_ERR_DEVICE, "SearchByBoW(KF, KF) device error");
    if (mbytes) memcpy(matches12, h + o_match, mbytes);
    memcpy(n_matches, h + o_cnt, (size_t)n_pairs * 4);
    return ORB_OK;
}

int orb_search_by_bow_kf_device(orb_matcher_t m, const orb_kf_device_t* kf1s, int n_kf1, const uint8_t* const* d_ok1,
                                const orb_kf_device_t* kf2s, const uint8_t* const* d_ok2, const int32_t* pair_kf1,
                                int n_pairs, int32_t* d_matches12, int32_t* d_n_matches, void* stream) {
    if (!m || n_pairs < 0 || n_pairs > 65535 || n_kf1 <= 0 || n_kf1 > 65535 || !kf1s ||
        (n_pairs > 0 && (!kf2s || !d_matches12 || !d_n_matches)))
        return orbgpu_fail(ORB_ERR_ARG, "bad SearchByBoW(KF, KF) arguments");
    if (n_pairs == 0) return ORB_OK;
    auto bad = [](const orb_kf_device_t& k) {
        return k.cap <= 0 || k.cap >= kMaxCap || !k.kps || !k.desc || !k.n || !k.fv_node || !k.fv_begin || !k.fv_feat ||
               !k.n_nodes || (reinterpret_cast<uintptr_t>(k.desc) & 15) != 0;
    };
    int C = 0, C2 = 0;
    for (int k = 0; k < n_kf1; ++k) {
        if (bad(kf1s[k])) return orbgpu_fail(ORB_ERR_ARG, "invalid keyframe device view");
        C = std::max(C, kf1s[k].cap);
    }
    for (int p = 0; p < n_pairs; ++p) {
        if (bad(kf2s[p])) return orbgpu_fail(ORB_ERR_ARG, "invalid second keyframe device view");
        if (pair_kf1 && (pair_kf1[p] < 0 || pair_kf1[p] >= n_kf1)) return orbgpu_fail(ORB_ERR_ARG, "bad pair_kf1");
        C2 = std::max(C2, kf2s[p].cap);
    }
    hipStream_t s = (hipStream_t)stream;
    const int ns = n_kf1 + n_pairs;
    // upload: BowSide [the kf1s | the pairs' second keyframes] | kf1 index per pair; device only: the claim rows
    const size_t o_pk = align256(ns * sizeof(BowSide));
    const size_t bytes = o_pk + align256(4 * (size_t)n_pairs);
    char* h = nullptr;
    if (int rc = orbgpu_matcher_upload_slot(m, bytes, &h)) return rc;
    auto* sides = reinterpret_cast<BowSide*>(h);
    auto* pk = reinterpret_cast<int32_t*>(h + o_pk);
    for (int k = 0; k < ns; ++k) {
        const orb_kf_device_t& v = k < n_kf1 ? kf1s[k] : kf2s[k - n_kf1];
        const uint8_t* const* oks = k < n_kf1 ? d_ok1 : d_ok2;
        const uint8_t* ok = oks ? oks[k < n_kf1 ? k : k - n_kf1] : nullptr;
        if (!ok) ok = v.has_mappoint;
        sides[k] = BowSide{v.kps, reinterpret_cast<const uint4*>(v.desc), v.n, ok, v.fv_node, v.fv_begin, v.fv_feat,
                           v.n_nodes, v.cap, 0};
    }
    int CK = 0;  // node < *n_nodes <= cap: the grid covers the capacity, waves past the count return
    for (int p = 0; p < n_pairs; ++p) {
        pk[p] = pair_kf1 ? pair_kf1[p] : 0;
        CK = std::max(CK, kf1s[pk[p]].cap);
    }
    // device copy and claim rows, stream-ordered (calls on different streams do not share them)
    char* d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d), bytes + (size_t)n_pairs * C2, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    bool ok = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
              orbgpu_matcher_upload_mark(m, s) == ORB_OK;
    ok = ok && launch_kf(reinterpret_cast<const BowSide*>(d), reinterpret_cast<const int32_t*>(d + o_pk), n_kf1, n_pairs, CK,
                         orbgpu_matcher_nnratio(m), orbgpu_matcher_check_ori(m), C, d_matches12, C2,
                         reinterpret_cast<uint8_t*>(d + bytes), d_n_matches, s);
    if (hipFreeAsync(d, s) != hipSuccess) ok = false;
    return ok ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "SearchByBoW(KF, KF) device error");
}

}  // extern "C"
