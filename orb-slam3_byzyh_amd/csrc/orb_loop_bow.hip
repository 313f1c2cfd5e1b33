// Loop closing's merge of the window's SearchByBoW matches and the Sim3Solver constructor's gather, batched
// over candidates (reference src/LoopClosing.cc:855-881 and src/Sim3Solver.cc:71-118), on MI355X.
//
// Input: the matches12 rows of orb_search_by_bow_kf[_device] (current keyframe KF1 against every keyframe
// of every candidate's window), the map points as indices into one pool.  Candidate c owns the pairs
// [group[c], group[c+1]) in window order j.
//
// Stage A, the merge.  The reference walks (j, k) in lexicographic order and inserts a non-bad point it has
// not seen yet for this candidate: numBoWMatches++, vpMatchedPoints[k] = point, vpKeyFrameMatchedMP[k] =
// window keyframe j; a later j that inserts another new point at the same k overwrites the slot while the
// count keeps both.  In parallel form: the first occurrence of a point is the minimum of j * C + k over its
// occurrences, and slot k takes the largest j whose (j, k) is a first occurrence.
//   k_lb_insert  one thread per (pair, k): the occurrence's key into the candidate's hash table (open
//                addressing on the point id; a slot holds (id + 1) << 32 | key, 0 = empty; claimed with a
//                compare-and-swap, lowered with a 64-bit atomic minimum).  Which slot an id lands in depends
//                on the arrival order, the minimum it ends with does not.  The tables are sized by the
//                candidates' pairs (2 * pairs * n1 slots rounded up to a power of two), not by the pool.
//   k_lb_first   one thread per (pair, k): an occurrence whose key is its point's minimum is a first one:
//                num_bow[c] += 1 (an integer sum), matched_pair[c][k] = max(.., j).
// Stage B, the gather.
//   k_lb_gather  one block per candidate: matched_point[c][k], then the slots the constructor keeps, in
//                increasing k, compacted by a block scan so that entry i is the reference's i-th: idx1,
//                x3dc1 = Rcw1 X1w + tcw1, x3dc2 = Rcw2[c] X2w + tcw2[c] (the candidate's pose for every window
//                keyframe's point, as the reference has it), max_err = (float)(9.210 * sigma2) of the
//                keypoint's octave.  Entries past n[c] are filled with idx1 -1 and zeros.
// The transform is float32 in the order orb_sim3_projection.hip uses for Pc = Rcw P + tcw:
// fma(r2, z, fma(r0, x, r1 * y)) + t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbgpu.h"
#include "orbgpu_internal.h"

int orbgpu_matcher_reserve(orb_matcher_t m, size_t bytes, char** d_buf, char** h_buf, hipStream_t* stream,
                           int* check_ori);
int orbgpu_matcher_upload_slot(orb_matcher_t m, size_t bytes, char** h);
int orbgpu_matcher_upload_mark(orb_matcher_t m, hipStream_t s);

namespace {

constexpr int kMaxStride = 1 << 20;
constexpr int kBlock = 256;

// What the kernels read: the caller's record with every array pointer a device pointer, plus the uploaded
// tables and the hash tables (one of 1 << tab_bits slots per candidate).
struct LbArgs {
    orb_loop_bow_in_t in;       // kf2s, pair_ok, group, Tcw2: the uploaded device copies
    const int32_t* pair_cand;   // candidate of a pair
    unsigned long long* tab;
    int tab_bits;
    orb_loop_bow_out_t out;
};

// The map point pair p gives KF1's feature k (vvpMatchedMPs[j][k], non-NULL and not bad), or -1.
__device__ __forceinline__ int lb_entry(const LbArgs& A, int p, int k, int& idx2) {
    idx2 = -1;
    if (A.in.pair_ok && A.in.pair_ok[p] == 0) return -1;  // !vpCovKFi[j] || isBad() (LoopClosing.cc:842)
    const orb_loop_bow_kf_t& F = A.in.kf2s[p];
    idx2 = A.in.matches12[(size_t)p * A.in.stride + k];
    if ((unsigned)idx2 >= (unsigned)F.n) return -1;
    const int id = F.mp_id[idx2];
    if ((unsigned)id >= (unsigned)A.in.n_points) return -1;
    if (A.in.bad && A.in.bad[id] != 0) return -1;  // pMPi_j->isBad() (:864)
    return id;
}

__device__ __forceinline__ uint32_t lb_hash(int id, int bits) { return ((uint32_t)id * 0x9E3779B1u) >> (32 - bits); }

__global__ __launch_bounds__(kBlock) void k_lb_insert(const LbArgs A) {
    const int k = blockIdx.x * kBlock + threadIdx.x, p = blockIdx.y;
    if (k >= A.in.kf1.n) return;
    int idx2;
    const int id = lb_entry(A, p, k, idx2);
    if (id < 0) return;
    const int c = A.pair_cand[p], j = p - A.in.group[c];
    const unsigned long long w = ((unsigned long long)(id + 1) << 32) | (uint32_t)(j * A.in.stride + k);
    unsigned long long* tab = A.tab + ((size_t)c << A.tab_bits);
    const uint32_t mask = (1u << A.tab_bits) - 1;
    for (uint32_t h = lb_hash(id, A.tab_bits);; h = (h + 1) & mask) {  // at most half the slots are ever taken
        unsigned long long cur = __hip_atomic_load(&tab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&tab[h], 0ull, w);
            if (cur == 0) return;
        }
        if ((cur >> 32) == (w >> 32)) {  // the id's slot (a slot never changes its id): keep the smallest key
            atomicMin(&tab[h], w);
            return;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_lb_first(const LbArgs A) {
    const int k = blockIdx.x * kBlock + threadIdx.x, p = blockIdx.y;
    if (k >= A.in.kf1.n) return;
    int idx2;
    const int id = lb_entry(A, p, k, idx2);
    if (id < 0) return;
    const int c = A.pair_cand[p], j = p - A.in.group[c];
    const unsigned long long* tab = A.tab + ((size_t)c << A.tab_bits);
    const uint32_t mask = (1u << A.tab_bits) - 1;
    uint32_t h = lb_hash(id, A.tab_bits);
    while ((uint32_t)(tab[h] >> 32) != (uint32_t)(id + 1)) h = (h + 1) & mask;  // k_lb_insert put it there
    if ((uint32_t)tab[h] != (uint32_t)(j * A.in.stride + k)) return;  // seen before (spMatchedMPi, :868)
    atomicAdd(&A.out.num_bow[c], 1);                                   // numBoWMatches++
    atomicMax(&A.out.matched_pair[(size_t)c * A.in.stride + k], j);   // the last insertion at k stays (:876-878)
}

__global__ __launch_bounds__(kBlock) void k_lb_gather(const LbArgs A) {
    __shared__ int wave_sum[kBlock / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = A.in.stride, n1 = A.in.kf1.n;
    const size_t row = (size_t)c * C;
    const float* T1 = A.in.Tcw1;
    const float* T2 = A.in.Tcw2 + 12 * (size_t)c;
    int base = 0;
    for (int k0 = 0; k0 < C; k0 += kBlock) {
        const int k = k0 + tid;
        bool keep = false;
        int id1 = -1, id2 = -1, idx2 = -1, p = 0;
        if (k < C) {
            const int j = k < n1 ? A.out.matched_pair[row + k] : -1;
            if (j >= 0) {
                p = A.in.group[c] + j;
                id2 = lb_entry(A, p, k, idx2);
            }
            A.out.matched_point[row + k] = id2;
        }
        float s1 = 0.0f, s2 = 0.0f;
        if (id2 >= 0) {  // vpMatched12[i1] (Sim3Solver.cc:73)
            const orb_loop_bow_kf_t& F = A.in.kf2s[p];
            id1 = A.in.kf1.mp_id[k];
            const bool in1 = (unsigned)id1 < (unsigned)A.in.n_points;
            // pMP1 non-NULL and not bad (:78-82; pMP2 is not bad, or the merge had not taken it)
            const bool ok = A.in.ok1 ? A.in.ok1[k] != 0 : in1 && !(A.in.bad && A.in.bad[id1] != 0);
            // indexKF1 = k, indexKF2 = idx2 by the map's invariant; obs_ok: GetIndexInKeyFrame >= 0 (:87-91)
            const bool obs = (!A.in.kf1.obs_ok || A.in.kf1.obs_ok[k] != 0) && (!F.obs_ok || F.obs_ok[idx2] != 0);
            const int o1 = A.in.kf1.kps[k].octave, o2 = F.kps[idx2].octave;
            keep = ok && in1 && obs && (unsigned)o1 < (unsigned)A.in.kf1.nlevels && (unsigned)o2 < (unsigned)F.nlevels;
            if (keep) {
                s1 = A.in.kf1.level_sigma2[o1];
                s2 = F.level_sigma2[o2];
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_sum[wave] = __popcll(mask);
        __syncthreads();
        int pos = base + __popcll(mask & ((1ull << lane) - 1)), total = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < wave) pos += wave_sum[w];
            total += wave_sum[w];
        }
        if (keep) {
            const float* X1 = A.in.xyz + 3 * (size_t)id1;
            const float* X2 = A.in.xyz + 3 * (size_t)id2;
            A.out.idx1[row + pos] = k;                            // mvnIndices1 (:104)
            A.out.max_err1[row + pos] = (float)(9.210 * (double)s1);  // :96-100
            A.out.max_err2[row + pos] = (float)(9.210 * (double)s2);
#pragma unroll
            for (int r = 0; r < 3; ++r) {  // :106-110
                A.out.x3dc1[3 * (row + pos) + r] =
                    fmaf(T1[4 * r + 2], X1[2], fmaf(T1[4 * r], X1[0], T1[4 * r + 1] * X1[1])) + T1[4 * r + 3];
                A.out.x3dc2[3 * (row + pos) + r] =
                    fmaf(T2[4 * r + 2], X2[2], fmaf(T2[4 * r], X2[0], T2[4 * r + 1] * X2[1])) + T2[4 * r + 3];
            }
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) A.out.n[c] = base;
    for (int i = base + tid; i < C; i += kBlock) {
        A.out.idx1[row + i] = -1;
        A.out.max_err1[row + i] = 0.0f;
        A.out.max_err2[row + i] = 0.0f;
        for (int r = 0; r < 3; ++r) {
            A.out.x3dc1[3 * (row + i) + r] = 0.0f;
            A.out.x3dc2[3 * (row + i) + r] = 0.0f;
        }
    }
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The uploaded tables of a call and the hash tables' size.
struct Plan {
    size_t o_kf2, o_pok, o_group, o_pcand, o_tcw2, bytes;
    int tab_bits;
    size_t tab_bytes;
};

bool bad_kf(const orb_loop_bow_kf_t& k) {
    return k.n < 0 || k.n >= kMaxStride || k.nlevels < 1 || k.nlevels > 12 || (k.n > 0 && (!k.mp_id || !k.kps));
}

// Every argument is checked here, before anything is launched or written.
int plan_call(const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out, Plan* pl) {
    if (!in || !out || in->n_cand < 0 || in->n_cand > 65535 || in->n_pairs < 0 || in->n_pairs > 65535)
        return orbgpu_fail(ORB_ERR_ARG, "bad loop BoW problem arguments");
    if (in->n_cand == 0) return in->n_pairs == 0 ? ORB_OK : orbgpu_fail(ORB_ERR_ARG, "pairs without a candidate");
    if (!in->group || !in->Tcw2 || in->stride <= 0 || in->stride >= kMaxStride || bad_kf(in->kf1) ||
        in->kf1.n > in->stride || in->n_points < 0 || (in->n_points > 0 && !in->xyz) ||
        (in->n_pairs > 0 && (!in->kf2s || !in->matches12)))
        return orbgpu_fail(ORB_ERR_ARG, "bad loop BoW problem arguments");
    if (!out->matched_point || !out->matched_pair || !out->num_bow || !out->n || !out->idx1 || !out->x3dc1 ||
        !out->x3dc2 || !out->max_err1 || !out->max_err2)
        return orbgpu_fail(ORB_ERR_ARG, "null loop BoW problem output");
    if (in->group[0] != 0 || in->group[in->n_cand] != in->n_pairs) return orbgpu_fail(ORB_ERR_ARG, "bad group table");
    int max_pairs = 0;
    for (int c = 0; c < in->n_cand; ++c) {
        if (in->group[c + 1] < in->group[c]) return orbgpu_fail(ORB_ERR_ARG, "bad group table");
        max_pairs = std::max(max_pairs, in->group[c + 1] - in->group[c]);
    }
    for (int p = 0; p < in->n_pairs; ++p)
        if (bad_kf(in->kf2s[p])) return orbgpu_fail(ORB_ERR_ARG, "bad window keyframe record");
    if ((long long)max_pairs * in->stride >= (1ll << 31)) return orbgpu_fail(ORB_ERR_ARG, "window too large");
    size_t off = 0;
    pl->o_kf2 = off; off = align256(off + (size_t)std::max(in->n_pairs, 1) * sizeof(orb_loop_bow_kf_t));
    pl->o_pok = off; off = align256(off + (size_t)std::max(in->n_pairs, 1));
    pl->o_group = off; off = align256(off + ((size_t)in->n_cand + 1) * 4);
    pl->o_pcand = off; off = align256(off + (size_t)std::max(in->n_pairs, 1) * 4);
    pl->o_tcw2 = off; off = align256(off + (size_t)in->n_cand * 48);
    pl->bytes = off;
    const long long slots = 2ll * max_pairs * std::max(in->kf1.n, 1);
    if (slots > (1ll << 28)) return orbgpu_fail(ORB_ERR_ARG, "window too large");  // 2 GiB of table per candidate
    pl->tab_bits = 6;
    while ((1ll << pl->tab_bits) < slots) ++pl->tab_bits;
    pl->tab_bytes = ((size_t)in->n_cand << pl->tab_bits) * 8;
    return 1;  // something to do
}

// The tables at h (their device copy will be at d); kf2s: the window records with device pointers.
void fill_tables(const orb_loop_bow_in_t* in, const orb_loop_bow_kf_t* kf2s, const Plan& pl, char* h) {
    if (in->n_pairs) memcpy(h + pl.o_kf2, kf2s, (size_t)in->n_pairs * sizeof(orb_loop_bow_kf_t));
    if (in->pair_ok && in->n_pairs) memcpy(h + pl.o_pok, in->pair_ok, in->n_pairs);
    memcpy(h + pl.o_group, in->group, ((size_t)in->n_cand + 1) * 4);
    auto* pc = reinterpret_cast<int32_t*>(h + pl.o_pcand);
    for (int c = 0; c < in->n_cand; ++c)
        for (int p = in->group[c]; p < in->group[c + 1]; ++p) pc[p] = c;
    memcpy(h + pl.o_tcw2, in->Tcw2, (size_t)in->n_cand * 48);
}

// dev: the caller's record with device array pointers; d: the tables' device copy; d_tab: the hash tables.
// Two memsets (three with pairs) and up to three kernels, whatever n_pairs and n_cand are.
bool launch(const orb_loop_bow_in_t& dev, const orb_loop_bow_out_t& out, const Plan& pl, char* d, char* d_tab,
            hipStream_t s) {
    LbArgs A;
    A.in = dev;
    A.in.kf2s = reinterpret_cast<const orb_loop_bow_kf_t*>(d + pl.o_kf2);
    A.in.pair_ok = dev.pair_ok ? reinterpret_cast<const uint8_t*>(d + pl.o_pok) : nullptr;
    A.in.group = reinterpret_cast<const int32_t*>(d + pl.o_group);
    A.in.Tcw2 = reinterpret_cast<const float*>(d + pl.o_tcw2);
    A.pair_cand = reinterpret_cast<const int32_t*>(d + pl.o_pcand);
    A.tab = reinterpret_cast<unsigned long long*>(d_tab);
    A.tab_bits = pl.tab_bits;
    A.out = out;
    if (hipMemsetAsync(out.matched_pair, 0xFF, (size_t)dev.n_cand * dev.stride * 4, s) != hipSuccess) return false;
    if (hipMemsetAsync(out.num_bow, 0, (size_t)dev.n_cand * 4, s) != hipSuccess) return false;
    if (dev.n_pairs > 0 && dev.kf1.n > 0) {
        if (hipMemsetAsync(d_tab, 0, pl.tab_bytes, s) != hipSuccess) return false;
        const dim3 grid((dev.kf1.n + kBlock - 1) / kBlock, dev.n_pairs);
        hipLaunchKernelGGL(k_lb_insert, grid, dim3(kBlock), 0, s, A);
        hipLaunchKernelGGL(k_lb_first, grid, dim3(kBlock), 0, s, A);
    }
    hipLaunchKernelGGL(k_lb_gather, dim3(dev.n_cand), dim3(kBlock), 0, s, A);
    return hipGetLastError() == hipSuccess;
}

}  // namespace

extern "C" {

int orb_loop_bow_problems_device(orb_matcher_t m, const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out,
                                 void* stream) {
    if (!m) return orbgpu_fail(ORB_ERR_ARG, "null matcher");
    Plan pl;
    const int rc = plan_call(in, out, &pl);
    if (rc <= 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* h = nullptr;
    if (int e = orbgpu_matcher_upload_slot(m, pl.bytes, &h)) return e;
    fill_tables(in, in->kf2s, pl, h);
    char* d = nullptr;  // stream-ordered: the tables' copy and the hash tables
    if (hipMallocAsync(reinterpret_cast<void**>(&d), pl.bytes + pl.tab_bytes, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    bool ok = hipMemcpyAsync(d, h, pl.bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
              orbgpu_matcher_upload_mark(m, s) == ORB_OK;
    ok = ok && launch(*in, *out, pl, d, d + pl.bytes, s);
    if (hipFreeAsync(d, s) != hipSuccess) ok = false;
    return ok ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "loop BoW problems device error");
}

int orb_loop_bow_problems(orb_matcher_t m, const orb_loop_bow_in_t* in, const orb_loop_bow_out_t* out) {
    if (!m) return orbgpu_fail(ORB_ERR_ARG, "null matcher");
    Plan pl;
    const int rc = plan_call(in, out, &pl);
    if (rc <= 0) return rc;
    // packed layout: tables | KF1's arrays | per pair: mp_id, kps, obs_ok | pool | matches12 (one H2D copy);
    // device only: the hash tables; outputs: the four int arrays and n, then the four float arrays
    const size_t C = (size_t)in->stride, nc = (size_t)in->n_cand;
    size_t off = pl.bytes;
    auto take = [&](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    struct KfOff { size_t id, kps, obs; };
    auto take_kf = [&](const orb_loop_bow_kf_t& k) {
        return KfOff{take((size_t)k.n * 4), take((size_t)k.n * sizeof(orb_keypoint_t)), take((size_t)k.n)};
    };
    const KfOff o1 = take_kf(in->kf1);
    const size_t o_ok1 = take((size_t)in->kf1.n);
    std::vector<KfOff> o2(in->n_pairs);
    for (int p = 0; p < in->n_pairs; ++p) o2[p] = take_kf(in->kf2s[p]);
    const size_t o_xyz = take((size_t)in->n_points * 12), o_bad = take((size_t)in->n_points);
    const size_t o_m12 = take((size_t)in->n_pairs * C * 4);
    const size_t in_bytes = off;
    const size_t o_tab = take(pl.tab_bytes);
    const size_t o_out = off;
    const size_t o_mpt = take(nc * C * 4), o_mpr = take(nc * C * 4), o_idx = take(nc * C * 4), o_nb = take(nc * 4),
                 o_n = take(nc * 4), o_x1 = take(nc * C * 12), o_x2 = take(nc * C * 12), o_e1 = take(nc * C * 4),
                 o_e2 = take(nc * C * 4);
    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int e = orbgpu_matcher_reserve(m, off, &d, &h, &s, &check_ori)) return e;

    auto stage_kf = [&](const orb_loop_bow_kf_t& k, const KfOff& o) {
        orb_loop_bow_kf_t v = k;
        if (k.n) {
            memcpy(h + o.id, k.mp_id, (size_t)k.n * 4);
            memcpy(h + o.kps, k.kps, (size_t)k.n * sizeof(orb_keypoint_t));
            if (k.obs_ok) memcpy(h + o.obs, k.obs_ok, (size_t)k.n);
        }
        v.mp_id = reinterpret_cast<const int32_t*>(d + o.id);
        v.kps = reinterpret_cast<const orb_keypoint_t*>(d + o.kps);
        v.obs_ok = k.obs_ok ? reinterpret_cast<const uint8_t*>(d + o.obs) : nullptr;
        return v;
    };
    orb_loop_bow_in_t dev = *in;
    dev.kf1 = stage_kf(in->kf1, o1);
    if (in->ok1 && in->kf1.n) memcpy(h + o_ok1, in->ok1, (size_t)in->kf1.n);
    dev.ok1 = in->ok1 ? reinterpret_cast<const uint8_t*>(d + o_ok1) : nullptr;
    std::vector<orb_loop_bow_kf_t> kf2s(in->n_pairs);
    for (int p = 0; p < in->n_pairs; ++p) kf2s[p] = stage_kf(in->kf2s[p], o2[p]);
    if (in->n_points) {
        memcpy(h + o_xyz, in->xyz, (size_t)in->n_points * 12);
        if (in->bad) memcpy(h + o_bad, in->bad, (size_t)in->n_points);
    }
    dev.xyz = reinterpret_cast<const float*>(d + o_xyz);
    dev.bad = in->bad ? reinterpret_cast<const uint8_t*>(d + o_bad) : nullptr;
    if (in->n_pairs) memcpy(h + o_m12, in->matches12, (size_t)in->n_pairs * C * 4);
    dev.matches12 = reinterpret_cast<const int32_t*>(d + o_m12);
    fill_tables(in, kf2s.data(), pl, h);
    orb_loop_bow_out_t dout;
    dout.matched_point = reinterpret_cast<int32_t*>(d + o_mpt);
    dout.matched_pair = reinterpret_cast<int32_t*>(d + o_mpr);
    dout.idx1 = reinterpret_cast<int32_t*>(d + o_idx);
    dout.num_bow = reinterpret_cast<int32_t*>(d + o_nb);
    dout.n = reinterpret_cast<int32_t*>(d + o_n);
    dout.x3dc1 = reinterpret_cast<float*>(d + o_x1);
    dout.x3dc2 = reinterpret_cast<float*>(d + o_x2);
    dout.max_err1 = reinterpret_cast<float*>(d + o_e1);
    dout.max_err2 = reinterpret_cast<float*>(d + o_e2);

    bool ok = hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && launch(dev, dout, pl, d, d + o_tab, s);
    ok = ok && hipMemcpyAsync(h + o_out, d + o_out, off - o_out, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return orbgpu_fail(ORB_ERR_DEVICE, "loop BoW problems device error");
    memcpy(out->matched_point, h + o_mpt, nc * C * 4);
    memcpy(out->matched_pair, h + o_mpr, nc * C * 4);
    memcpy(out->idx1, h + o_idx, nc * C * 4);
    memcpy(out->num_bow, h + o_nb, nc * 4);
    memcpy(out->n, h + o_n, nc * 4);
    memcpy(out->x3dc1, h + o_x1, nc * C * 12);
    memcpy(out->x3dc2, h + o_x2, nc * C * 12);
    memcpy(out->max_err1, h + o_e1, nc * C * 4);
    memcpy(out->max_err2, h + o_e2, nc * C * 4);
    return ORB_OK;
}

}  // extern "C"
