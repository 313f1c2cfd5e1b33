// LocalMapping::CreateNewMapPoints on MI355X: the triangulation half (reference src/LocalMapping.cc:626-910;
// GeometricTools::Triangulate src/GeometricTools.cc:63-90; KeyFrame::UnprojectStereo src/KeyFrame.cc:905-924;
// MapPoint::UpdateNormalAndDepth src/MapPoint.cc:567-642), batched over the neighbours of one keyframe.
// Single pinhole camera (NLeft == -1, mpCamera2 == NULL): the two-camera branch (:665-715) is out of scope.
// Step 6 (the map mutation, :888-909) stays with the caller.
//
// A job (pair p, idx1 i) with matches12[p][i] >= 0 depends on no other job until upstream's neighbour loop
// hands idx1 to the first neighbour that succeeds, so:
//   k_np_triangulate  blockIdx.y = pair, one thread per idx1: walks :640-884 in order, writes the first gate
//                     that rejected the job (ORB_NP_*), x3D and bPointStereo.  The 4x4 null vector is solved
//                     per thread in registers (orb_svd4.h: one-sided Jacobi on A, not on A^T A).
//   k_np_resolve      one thread per idx1: taken_by = the smallest p with ORB_NP_OK, later OKs become
//                     ORB_NP_TAKEN; per block and pair the number of survivors and each survivor's rank
//                     among its block's survivors of the same pair (wave ballots, no atomics).
//   k_np_emit         every block scans the (pair, block) counts in (p, block) order -- a few hundred
//                     integers -- for its own offsets, block 0 writes the total; each survivor writes its
//                     record at offset + rank: upstream's creation order, p ascending then idx1 ascending,
//                     deterministic.  The records with p < k are a prefix that later neighbours cannot
//                     change (a caller that stops at CheckNewKeyFrames(), :568, uses that prefix).
//
// Float arithmetic as the reference build (g++ -O3 -march=native) contracts it -- the rule is written down
// in oracle/orb_frustum_oracle.cpp and csrc/orb_fuse.hip: `a*b + c*d` becomes fma(a, b, c*d), `a - b*c`
// becomes fma(-b, c, a), `a*b + c` becomes fma(a, b, c).  This file is compiled with -ffp-contract=off and
// every fma is explicit:
//   dot3(a, b) = fma(a[2], b[2], fma(a[0], b[0], a[1] * b[1]))       (rays, Rcw rows . x3D, norms)
//   xn         = ((u - cx) / fx, (v - cy) / fy, 1)                   (Pinhole::unprojectEig)
//   ray        = Rwc xn by dot3 over Rcw's columns;  cos = dot3(r1, r2) / (sqrt(dot3(r1, r1)) * sqrt(dot3(r2, r2)))
//   cosStereo  = (float)((d*d - a*a) / (d*d + a*a)), a = mb / 2, d = mvDepth, in double: cos(2 atan2(a, d))
//                written without the two libm calls (the identity is exact; 1 for a = d = 0; an infinite a or
//                d takes the value the libm pair gives; a NaN stays a NaN), rounded once
//   A[r][c]    = fma(xn[k], T[2][c], -T[k][c])                        (GeometricTools.cc:73-76)
//   x3Dh       = the null vector of A: one-sided Jacobi in float (orb_svd4.h)
//   x3D        = x3Dh[0..2] / x3Dh[3]                                 (three divisions)
//   stereo     = dot3(Rwc[r], ((u - cx) * z * invfx, (v - cy) * z * invfy, z)) + Ow[r],  u, v from mvKeys
//   z, x, y    = dot3(Rcw[r], x3D) + tcw[r];  invz = (float)(1.0 / (double)z)
//   mono       u = fx * x / z + cx (Pinhole::project);  e2 = fma(ex, ex, ey * ey);  (double)e2 > 5.991 * (double)sigma2
//   stereo     u = fma(fx * x, invz, cx);  u_r = fma(-mbf, invz, u) with keyframe 1's mbf for both keyframes (:826,
//              :853);  e2 = fma(er, er, fma(ex, ex, ey * ey));  (double)e2 > 7.8 * (double)sigma2
//   dist       = sqrt(dot3(x3D - Ow, x3D - Ow));  ratioDist = dist2 / dist1;  ratioOctave = sf1[o1] / sf2[o2];
//              ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor  (plain products)
//   record     normal = (n1 / dist1 + n2 / dist2) / 2;  max = dist1 * sf1[o1];  min = max / sf1[nlevels - 1]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orb_svd4.h"
#include "orbgpu.h"
#include "orbgpu_internal.h"

// Defined in orb_triangulation.hip: the matcher handle's staging buffers.
int orbgpu_matcher_reserve(orb_matcher_t m, size_t bytes, char** d_buf, char** h_buf, hipStream_t* stream,
                           int* check_ori);
int orbgpu_matcher_upload_slot(orb_matcher_t m, size_t bytes, char** h);
int orbgpu_matcher_upload_mark(orb_matcher_t m, hipStream_t s);

namespace {

constexpr int kNpMaxLevels = 12;
constexpr int kNpThreads = 256;
constexpr int kNpWaves = kNpThreads / 64;
constexpr int kNpMaxPairs = 1024;      // k_np_resolve keeps 4 x this many wave counts in LDS (16 KB)
constexpr int kNpMaxCap = 1 << 20;
constexpr int kNpMaxScan = 1 << 16;    // pairs x blocks of 256 idx1: every block of k_np_emit scans that many counts

// one keyframe as the kernels read it (an array in device memory: [0] keyframe 1, [1 + p] neighbour p)
struct NpKf {
    const orb_keypoint_t* kps;      // mvKeysUn
    const orb_keypoint_t* kps_raw;  // mvKeys (never null here)
    const int32_t* n_raw;           // KeyFrame::N as its producer left it
    const float* ur;                // mvuRight or null
    const float* depth;             // mvDepth (non-null where ur is)
    int cap, nlevels;
    float Tcw[12], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
    float scale[kNpMaxLevels], sigma2[kNpMaxLevels];
};

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) {
    return fmaf(a[2], b[2], fmaf(a[0], b[0], a[1] * b[1]));
}

// the keyframe's count, or -1 when its producer flagged it
__device__ __forceinline__ int np_count(const NpKf& K) {
    const int raw = *K.n_raw;
    return raw < 0 || raw > K.cap ? -1 : raw;
}

// Rwc * xn (:723-724): Rwc's row r is Rcw's column r
__device__ __forceinline__ void ray_of(const NpKf& K, const float xn[3], float ray[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float row[3] = {K.Tcw[r], K.Tcw[4 + r], K.Tcw[8 + r]};
        ray[r] = dot3(row, xn);
    }
}

// cos(2 * atan2(mb / 2, depth)) (:739, :742) in double, rounded once
__device__ __forceinline__ float cos_parallax_stereo(float mb, float depth) {
    const double a = (double)(mb / 2), d = (double)depth;
    if (isinf(d)) return isinf(a) ? 0.0f : 1.0f;  // atan2(a, +-inf) = 0 or pi (pi / 4 for a = inf): cos = 1 (0)
    if (isinf(a)) return -1.0f;                   // atan2(inf, d) = pi / 2
    const double den = d * d + a * a;
    return den == 0.0 ? 1.0f : (float)((d * d - a * a) / den);
}

// KeyFrame::UnprojectStereo(j, x3D)
__device__ __forceinline__ bool unproject_stereo(const NpKf& K, int j, float X[3]) {
    const float z = K.depth[j];
    if (!(z > 0)) return false;
    const float u = K.kps_raw[j].x, v = K.kps_raw[j].y;
    const float c[3] = {(u - K.cx) * z * K.invfx, (v - K.cy) * z * K.invfy, z};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float row[3] = {K.Tcw[r], K.Tcw[4 + r], K.Tcw[8 + r]};
        X[r] = dot3(row, c) + K.Ow[r];
    }
    return true;
}

__device__ __forceinline__ float cam_coord(const NpKf& K, int r, const float X[3]) {
    return dot3(&K.Tcw[4 * r], X) + K.Tcw[4 * r + 3];
}

// the reprojection test of one keyframe (:804-834 / :838-860); true = rejected
__device__ __forceinline__ bool chi2_rejects(const NpKf& K, const float X[3], float z, float kx, float ky, int octave,
                                             bool stereo, float kp_ur, float mbf1) {
    const float x = cam_coord(K, 0, X), y = cam_coord(K, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const double sigma2 = (double)K.sigma2[octave];
    if (!stereo) {
        const float ex = (K.fx * x / z + K.cx) - kx, ey = (K.fy * y / z + K.cy) - ky;
        return (double)fmaf(ex, ex, ey * ey) > 5.991 * sigma2;
    }
    const float u = fmaf(K.fx * x, invz, K.cx);
    const float u_r = fmaf(-mbf1, invz, u);
    const float v = fmaf(K.fy * y, invz, K.cy);
    const float ex = u - kx, ey = v - ky, er = u_r - kp_ur;
    return (double)fmaf(er, er, fmaf(ex, ex, ey * ey)) > 7.8 * sigma2;
}

__global__ __launch_bounds__(kNpThreads) void k_np_triangulate(const NpKf* __restrict__ kfs,
                                                               const int32_t* __restrict__ matches,
                                                               const int32_t* __restrict__ n_matches, int C,
                                                               orb_newpoints_params_t prm, int32_t* __restrict__ status,
                                                               float* __restrict__ x3d,
                                                               uint8_t* __restrict__ from_stereo) {
    const int i = blockIdx.x * kNpThreads + threadIdx.x, p = blockIdx.y;
    if (i >= C) return;
    const size_t job = (size_t)p * C + i;
    const NpKf& K1 = kfs[0];
    const NpKf& K2 = kfs[1 + p];
    int st = ORB_NP_NO_MATCH;
    float X[3] = {0.f, 0.f, 0.f};
    bool point_stereo = false;
    do {
        const int n1 = np_count(K1), n2 = np_count(K2);
        if (n1 < 0 || n2 < 0 || i >= n1) break;
        if (n_matches && n_matches[p] < 0) break;                       // a pair the search flagged
        const int idx2 = matches[job];
        if (idx2 < 0 || idx2 >= n2) break;
        const orb_keypoint_t kp1 = K1.kps[i], kp2 = K2.kps[idx2];       // :640, :653 (NLeft == -1: mvKeysUn)
        if (kp1.octave < 0 || kp1.octave >= K1.nlevels || kp2.octave < 0 || kp2.octave >= K2.nlevels) break;
        const float kp1_ur = K1.ur ? K1.ur[i] : -1.0f, kp2_ur = K2.ur ? K2.ur[idx2] : -1.0f;
        const bool stereo1 = kp1_ur >= 0, stereo2 = kp2_ur >= 0;        // :645, :659

        // the parallax between the rays (:720-748)
        const float xn1[3] = {(kp1.x - K1.cx) / K1.fx, (kp1.y - K1.cy) / K1.fy, 1.0f};
        const float xn2[3] = {(kp2.x - K2.cx) / K2.fx, (kp2.y - K2.cy) / K2.fy, 1.0f};
        float ray1[3], ray2[3];
        ray_of(K1, xn1, ray1);
        ray_of(K2, xn2, ray2);
        const float cosRays = dot3(ray1, ray2) / (sqrtf(dot3(ray1, ray1)) * sqrtf(dot3(ray2, ray2)));
        float cos1 = cosRays + 1, cos2 = cos1;
        if (stereo1) cos1 = cos_parallax_stereo(K1.mb, K1.depth[i]);
        else if (stereo2) cos2 = cos_parallax_stereo(K2.mb, K2.depth[idx2]);
        const float cosStereo = cos2 < cos1 ? cos2 : cos1;             // std::min(cos1, cos2)

        if (cosRays < cosStereo && cosRays > 0 &&
            (stereo1 || stereo2 || (double)cosRays < (prm.inertial ? 0.9996 : 0.9998))) {  // :758-765
            float A[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                A[0][c] = fmaf(xn1[0], K1.Tcw[8 + c], -K1.Tcw[c]);
                A[1][c] = fmaf(xn1[1], K1.Tcw[8 + c], -K1.Tcw[4 + c]);
                A[2][c] = fmaf(xn2[0], K2.Tcw[8 + c], -K2.Tcw[c]);
                A[3][c] = fmaf(xn2[1], K2.Tcw[8 + c], -K2.Tcw[4 + c]);
            }
            float xh[4];
            orbgpu::svd4_null_vector(A, xh);
            if (xh[3] == 0) { st = ORB_NP_TRI_W_ZERO; break; }
            X[0] = xh[0] / xh[3];
            X[1] = xh[1] / xh[3];
            X[2] = xh[2] / xh[3];
        } else if (stereo1 && cos1 < cos2) {                            // :766-772
            point_stereo = true;
            if (!unproject_stereo(K1, i, X)) { st = ORB_NP_STEREO_DEPTH; break; }
        } else if (stereo2 && cos2 < cos1) {                            // :773-779
            point_stereo = true;
            if (!unproject_stereo(K2, idx2, X)) { st = ORB_NP_STEREO_DEPTH; break; }
        } else {
            st = ORB_NP_LOW_PARALLAX;                                   // :780-783
            break;
        }

        const float z1 = cam_coord(K1, 2, X);                           // :794-800
        if (z1 <= 0) { st = ORB_NP_Z1; break; }
        const float z2 = cam_coord(K2, 2, X);
        if (z2 <= 0) { st = ORB_NP_Z2; break; }
        if (chi2_rejects(K1, X, z1, kp1.x, kp1.y, kp1.octave, stereo1, kp1_ur, K1.mbf)) { st = ORB_NP_CHI2_1; break; }
        if (chi2_rejects(K2, X, z2, kp2.x, kp2.y, kp2.octave, stereo2, kp2_ur, K1.mbf)) { st = ORB_NP_CHI2_2; break; }

        const float d1v[3] = {X[0] - K1.Ow[0], X[1] - K1.Ow[1], X[2] - K1.Ow[2]};   // :866-884
        const float d2v[3] = {X[0] - K2.Ow[0], X[1] - K2.Ow[1], X[2] - K2.Ow[2]};
        const float dist1 = sqrtf(dot3(d1v, d1v)), dist2 = sqrtf(dot3(d2v, d2v));
        if (dist1 == 0 || dist2 == 0) { st = ORB_NP_DIST_ZERO; break; }
        if (prm.far_points && (dist1 >= prm.th_far_points || dist2 >= prm.th_far_points)) { st = ORB_NP_FAR; break; }
        const float ratioDist = dist2 / dist1;
        const float ratioOctave = K1.scale[kp1.octave] / K2.scale[kp2.octave];
        if (ratioDist * prm.ratio_factor < ratioOctave || ratioDist > ratioOctave * prm.ratio_factor) {
            st = ORB_NP_SCALE;
            break;
        }
        st = ORB_NP_OK;
    } while (false);
    status[job] = st;
    x3d[3 * job] = X[0];
    x3d[3 * job + 1] = X[1];
    x3d[3 * job + 2] = X[2];
    from_stereo[job] = point_stereo ? 1 : 0;
}

// blk_cnt[p * gridDim.x + block]: the survivors of pair p among this block's idx1; rank[i]: idx1 i's place
// among them.  status: ORB_NP_OK past the first becomes ORB_NP_TAKEN.
__global__ __launch_bounds__(kNpThreads) void k_np_resolve(int32_t* __restrict__ status, int P, int C,
                                                           int32_t* __restrict__ taken_by, int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ blk_cnt) {
    __shared__ int s_w[kNpWaves][kNpMaxPairs];
    const int i = blockIdx.x * kNpThreads + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int taken = -1;
    if (i < C) {
        for (int p = 0; p < P; ++p) {
            const size_t job = (size_t)p * C + i;
            if (status[job] != ORB_NP_OK) continue;
            if (taken < 0) taken = p;
            else status[job] = ORB_NP_TAKEN;
        }
        taken_by[i] = taken;
    }
    int my = 0;
    for (int p = 0; p < P; ++p) {  // wave-uniform: every lane votes
        const unsigned long long b = __ballot(taken == p);
        if (taken == p) my = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w][p] = __popcll(b);
    }
    __syncthreads();
    if (taken >= 0) {
        for (int k = 0; k < w; ++k) my += s_w[k][taken];
        rank[i] = my;
    }
    for (int p = threadIdx.x; p < P; p += kNpThreads) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < kNpWaves; ++k) s += s_w[k][p];
        blk_cnt[(size_t)p * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kNpThreads) void k_np_emit(const NpKf* __restrict__ kfs, const int32_t* __restrict__ matches,
                                                        const float* __restrict__ x3d,
                                                        const uint8_t* __restrict__ from_stereo,
                                                        const int32_t* __restrict__ taken_by,
                                                        const int32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ blk_cnt, int P, int C,
                                                        orb_newpoint_t* __restrict__ records, int32_t* __restrict__ n_new) {
    __shared__ int s_off[kNpMaxPairs];
    __shared__ int s_wsum[kNpWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nblk = gridDim.x, total = P * nblk;
    // the exclusive scan of blk_cnt in (p, block) order; this block keeps the entries of its own column
    int carry = 0;
    for (int base = 0; base < total; base += kNpThreads) {
        const int q = base + threadIdx.x;
        const int v = q < total ? blk_cnt[q] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wsum[w] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < kNpWaves; ++k) {
            if (k < w) woff += s_wsum[k];
            tot += s_wsum[k];
        }
        if (q < total && q % nblk == blockIdx.x) s_off[q / nblk] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_new = carry;
    const int i = blockIdx.x * kNpThreads + threadIdx.x;
    if (i >= C) return;
    const int p = taken_by[i];
    if (p < 0) return;
    const NpKf& K1 = kfs[0];
    const NpKf& K2 = kfs[1 + p];
    const size_t job = (size_t)p * C + i;
    const float X[3] = {x3d[3 * job], x3d[3 * job + 1], x3d[3 * job + 2]};
    // MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:588-641) for the observations (KF1, idx1), (KF2, idx2):
    // the sum of two unit vectors does not depend on the std::map's order
    const float n1[3] = {X[0] - K1.Ow[0], X[1] - K1.Ow[1], X[2] - K1.Ow[2]};
    const float n2[3] = {X[0] - K2.Ow[0], X[1] - K2.Ow[1], X[2] - K2.Ow[2]};
    const float d1 = sqrtf(dot3(n1, n1)), d2 = sqrtf(dot3(n2, n2));
    orb_newpoint_t r;
    r.p = p;
    r.idx1 = i;
    r.idx2 = matches[job];
    r.from_stereo = from_stereo[job];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.x3d[k] = X[k];
        r.normal[k] = (n1[k] / d1 + n2[k] / d2) / 2.0f;
    }
    r.max_dist = d1 * K1.scale[K1.kps[i].octave];                       // :639-640, level = kp1.octave
    r.min_dist = r.max_dist / K1.scale[K1.nlevels - 1];
    records[s_off[p] + rank[i]] = r;
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

int np_blocks(int C) { return (C + kNpThreads - 1) / kNpThreads; }
size_t np_args_bytes(int P) { return align256(sizeof(NpKf) * (size_t)(P + 1)); }
// rank [C] | blk_cnt [P x blocks]
size_t np_scratch_bytes(int P, int C) { return align256(4 * (size_t)C) + align256(4 * (size_t)P * np_blocks(C)); }

bool out_ok(const orb_newpoints_out_t* o) {
    return o && o->status && o->x3d && o->from_stereo && o->taken_by && o->records && o->n_new;
}

bool extra_ok(const orb_newpoints_kf_extra_t& e, bool has_ur) { return !has_ur || e.depth; }

// the host-side fields of one keyframe; the device pointers are set by the caller
bool np_fill(NpKf& o, float fx, float fy, float cx, float cy, int nlevels, const float* scale, const float* sigma2,
             const orb_newpoints_kf_extra_t& e) {
    if (nlevels < 1 || nlevels > kNpMaxLevels || !scale || !sigma2) return false;
    memset(&o, 0, sizeof(o));
    o.nlevels = nlevels;
    memcpy(o.Tcw, e.Tcw, sizeof(o.Tcw));
    memcpy(o.Ow, e.Ow, sizeof(o.Ow));
    o.fx = fx; o.fy = fy; o.cx = cx; o.cy = cy;
    o.invfx = e.invfx; o.invfy = e.invfy; o.mb = e.mb; o.mbf = e.mbf;
    for (int l = 0; l < nlevels; ++l) {
        o.scale[l] = scale[l];
        o.sigma2[l] = sigma2[l];
    }
    return true;
}

// The launches of one call.  kfs: [0] keyframe 1, [1 + p] neighbour p, complete; h_args pinned staging of
// d_args (np_args_bytes); d_scratch np_scratch_bytes; every other pointer device memory.
int np_launch(const std::vector<NpKf>& kfs, char* h_args, char* d_args, char* d_scratch, const int32_t* d_matches,
              const int32_t* d_n_matches, int C, const orb_newpoints_params_t& prm, const orb_newpoints_out_t& out,
              hipStream_t s) {
    const int P = (int)kfs.size() - 1, nblk = np_blocks(C);
    memcpy(h_args, kfs.data(), sizeof(NpKf) * kfs.size());
    if (hipMemcpyAsync(d_args, h_args, sizeof(NpKf) * kfs.size(), hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "CreateNewMapPoints argument upload failed");
    const NpKf* dk = reinterpret_cast<const NpKf*>(d_args);
    int32_t* rank = reinterpret_cast<int32_t*>(d_scratch);
    int32_t* blk_cnt = reinterpret_cast<int32_t*>(d_scratch + align256(4 * (size_t)C));
    hipLaunchKernelGGL(k_np_triangulate, dim3(nblk, P), dim3(kNpThreads), 0, s, dk, d_matches, d_n_matches, C, prm,
                       out.status, out.x3d, out.from_stereo);
    hipLaunchKernelGGL(k_np_resolve, dim3(nblk), dim3(kNpThreads), 0, s, out.status, P, C, out.taken_by, rank, blk_cnt);
    hipLaunchKernelGGL(k_np_emit, dim3(nblk), dim3(kNpThreads), 0, s, dk, d_matches, out.x3d, out.from_stereo,
                       out.taken_by, rank, blk_cnt, P, C, out.records, out.n_new);
    return hipGetLastError() == hipSuccess ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "CreateNewMapPoints kernel launch failed");
}

}  // namespace

extern "C" {

int orb_create_new_map_points_device(orb_matcher_t m, const orb_newpoints_kf_device_t* kf1,
                                     const orb_newpoints_kf_device_t* kf2s, int n_pairs,
                                     const orb_newpoints_params_t* params, const int32_t* d_matches12,
                                     const int32_t* d_n_matches, const orb_newpoints_out_t* out, void* stream) {
    if (!m || !kf1 || !params || !out_ok(out) || n_pairs < 0 || n_pairs > kNpMaxPairs ||
        (n_pairs > 0 && (!kf2s || !d_matches12)))
        return orbgpu_fail(ORB_ERR_ARG, "bad CreateNewMapPoints arguments");
    std::vector<NpKf> recs(n_pairs + 1);
    for (int k = 0; k <= n_pairs; ++k) {
        const orb_newpoints_kf_device_t& v = k == 0 ? *kf1 : kf2s[k - 1];
        const orb_kf_device_t& f = v.view;
        if (f.cap <= 0 || f.cap > kNpMaxCap || !f.kps || !f.n || !extra_ok(v.extra, f.u_right != nullptr) ||
            !np_fill(recs[k], f.fx, f.fy, f.cx, f.cy, f.nlevels, f.scale_factors, f.level_sigma2, v.extra))
            return orbgpu_fail(ORB_ERR_ARG,
                               "CreateNewMapPoints: invalid keyframe device view (cap <= 2^20, nlevels <= 12, depth with u_right)");
        NpKf& o = recs[k];
        o.kps = f.kps;
        o.kps_raw = v.extra.kps_raw ? v.extra.kps_raw : f.kps;
        o.n_raw = f.n;
        o.ur = f.u_right;
        o.depth = v.extra.depth;
        o.cap = f.cap;
    }
    hipStream_t s = (hipStream_t)stream;
    const int C = kf1->view.cap;
    if ((size_t)n_pairs * np_blocks(C) > (size_t)kNpMaxScan)
        return orbgpu_fail(ORB_ERR_ARG, "CreateNewMapPoints: n_pairs x ceil(cap / 256) above 65536");
    if (n_pairs == 0) {
        const bool ok = hipMemsetAsync(out->taken_by, 0xFF, 4 * (size_t)C, s) == hipSuccess &&
                        hipMemsetAsync(out->n_new, 0, 4, s) == hipSuccess;
        return ok ? ORB_OK : orbgpu_fail(ORB_ERR_DEVICE, "CreateNewMapPoints memset failed");
    }
    const size_t abytes = np_args_bytes(n_pairs), sbytes = np_scratch_bytes(n_pairs, C);
    char* h = nullptr;
    if (int rc = orbgpu_matcher_upload_slot(m, abytes, &h)) return rc;
    char* d = nullptr;  // stream-ordered (calls on different streams do not share it)
    if (hipMallocAsync(reinterpret_cast<void**>(&d), abytes + sbytes, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "hipMallocAsync failed");
    int rc = np_launch(recs, h, d, d + abytes, d_matches12, d_n_matches, C, *params, *out, s);
    if (orbgpu_matcher_upload_mark(m, s) != ORB_OK && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "event record failed");
    if (hipFreeAsync(d, s) != hipSuccess && rc == ORB_OK) rc = orbgpu_fail(ORB_ERR_DEVICE, "hipFreeAsync failed");
    return rc;
}

int orb_create_new_map_points(orb_matcher_t m, const orb_newpoints_kf_t* kf1, const orb_newpoints_kf_t* kf2s, int n_pairs,
                              const orb_newpoints_params_t* params, const int32_t* matches12, const int32_t* n_matches,
                              const orb_newpoints_out_t* out) {
    if (!m || !kf1 || !params || !out_ok(out) || n_pairs < 0 || n_pairs > kNpMaxPairs ||
        (n_pairs > 0 && (!kf2s || !matches12)))
        return orbgpu_fail(ORB_ERR_ARG, "bad CreateNewMapPoints arguments");
    // every argument is checked before the handle's staging is touched
    std::vector<NpKf> recs(n_pairs + 1);
    for (int k = 0; k <= n_pairs; ++k) {
        const orb_newpoints_kf_t& v = k == 0 ? *kf1 : kf2s[k - 1];
        const orb_kf_view_t& f = v.view;
        if (f.n < 0 || f.n > kNpMaxCap || (f.n > 0 && !f.kps_un) || !extra_ok(v.extra, f.n > 0 && f.u_right != nullptr) ||
            !np_fill(recs[k], f.fx, f.fy, f.cx, f.cy, f.nlevels, f.scale_factors, f.level_sigma2, v.extra))
            return orbgpu_fail(ORB_ERR_ARG,
                               "CreateNewMapPoints: invalid keyframe view (N <= 2^20, nlevels <= 12, depth with u_right)");
        for (int i = 0; i < f.n; ++i)
            if (f.kps_un[i].octave < 0 || f.kps_un[i].octave >= f.nlevels)
                return orbgpu_fail(ORB_ERR_ARG, "CreateNewMapPoints: keypoint octave outside [0, nlevels)");
    }
    const int n1 = kf1->view.n, C = std::max(n1, 1);
    if ((size_t)n_pairs * np_blocks(C) > (size_t)kNpMaxScan)
        return orbgpu_fail(ORB_ERR_ARG, "CreateNewMapPoints: n_pairs x ceil(N1 / 256) above 65536");
    for (int p = 0; p < n_pairs; ++p) {
        if (n_matches && n_matches[p] < 0) continue;  // a flagged pair's row is not read
        for (int i = 0; i < n1; ++i)
            if (matches12[(size_t)p * C + i] >= kf2s[p].view.n)
                return orbgpu_fail(ORB_ERR_ARG, "CreateNewMapPoints: match index past the neighbour's N");
    }
    if (n_pairs == 0) {
        for (int i = 0; i < C; ++i) out->taken_by[i] = -1;
        *out->n_new = 0;
        return ORB_OK;
    }
    // packed layout, one upload: per keyframe count | kps_un | kps_raw | u_right | depth; matches; pair counts;
    // then the argument records, the outputs (one download) and the scratch
    struct Off { size_t cnt, kps, raw, ur, depth; };
    std::vector<Off> offs(n_pairs + 1);
    size_t off = 0;
    for (int k = 0; k <= n_pairs; ++k) {
        const orb_newpoints_kf_t& v = k == 0 ? *kf1 : kf2s[k - 1];
        const size_t cap = (size_t)std::max(v.view.n, 1);
        Off& o = offs[k];
        o.cnt = off; off = align256(off + 4);
        o.kps = off; off = align256(off + cap * sizeof(orb_keypoint_t));
        o.raw = off; if (v.extra.kps_raw) off = align256(off + cap * sizeof(orb_keypoint_t));
        o.ur = off; if (v.view.u_right) off = align256(off + cap * 4);
        o.depth = off; if (v.extra.depth) off = align256(off + cap * 4);
    }
    const size_t jobs = (size_t)n_pairs * C;
    const size_t o_match = off; off = align256(off + 4 * jobs);
    const size_t o_cnt = off; off = align256(off + 4 * (size_t)n_pairs);
    const size_t o_args = off; off += np_args_bytes(n_pairs);
    const size_t in_bytes = o_args;  // (the argument records are uploaded by np_launch)
    const size_t o_status = off; off = align256(off + 4 * jobs);
    const size_t o_x3d = off; off = align256(off + 12 * jobs);
    const size_t o_fs = off; off = align256(off + jobs);
    const size_t o_taken = off; off = align256(off + 4 * (size_t)C);
    const size_t o_rec = off; off = align256(off + sizeof(orb_newpoint_t) * (size_t)C);
    const size_t o_nnew = off; off = align256(off + 4);
    const size_t o_scratch = off; off += np_scratch_bytes(n_pairs, C);

    char *d = nullptr, *h = nullptr;
    hipStream_t s = nullptr;
    int check_ori = 0;
    if (int rc = orbgpu_matcher_reserve(m, off, &d, &h, &s, &check_ori)) return rc;
    for (int k = 0; k <= n_pairs; ++k) {
        const orb_newpoints_kf_t& v = k == 0 ? *kf1 : kf2s[k - 1];
        const orb_kf_view_t& f = v.view;
        const Off& o = offs[k];
        const size_t n = (size_t)f.n;
        *reinterpret_cast<int32_t*>(h + o.cnt) = f.n;
        if (n) {
            memcpy(h + o.kps, f.kps_un, n * sizeof(orb_keypoint_t));
            if (v.extra.kps_raw) memcpy(h + o.raw, v.extra.kps_raw, n * sizeof(orb_keypoint_t));
            if (f.u_right) memcpy(h + o.ur, f.u_right, n * 4);
            if (v.extra.depth) memcpy(h + o.depth, v.extra.depth, n * 4);
        }
        NpKf& r = recs[k];
        r.kps = reinterpret_cast<const orb_keypoint_t*>(d + o.kps);
        r.kps_raw = v.extra.kps_raw ? reinterpret_cast<const orb_keypoint_t*>(d + o.raw) : r.kps;
        r.n_raw = reinterpret_cast<const int32_t*>(d + o.cnt);
        r.ur = f.u_right ? reinterpret_cast<const float*>(d + o.ur) : nullptr;
        r.depth = v.extra.depth ? reinterpret_cast<const float*>(d + o.depth) : nullptr;
        r.cap = std::max(f.n, 1);
    }
    if (n1) memcpy(h + o_match, matches12, 4 * jobs);
    else memset(h + o_match, 0xFF, 4 * jobs);
    if (n_matches) memcpy(h + o_cnt, n_matches, 4 * (size_t)n_pairs);
    if (hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "CreateNewMapPoints upload failed");
    const orb_newpoints_out_t dout{reinterpret_cast<int32_t*>(d + o_status), reinterpret_cast<float*>(d + o_x3d),
                                   reinterpret_cast<uint8_t*>(d + o_fs), reinterpret_cast<int32_t*>(d + o_taken),
                                   reinterpret_cast<orb_newpoint_t*>(d + o_rec), reinterpret_cast<int32_t*>(d + o_nnew)};
    if (int rc = np_launch(recs, h + o_args, d + o_args, d + o_scratch, reinterpret_cast<const int32_t*>(d + o_match),
                           n_matches ? reinterpret_cast<const int32_t*>(d + o_cnt) : nullptr, C, *params, dout, s))
        return rc;
    if (hipMemcpyAsync(h + o_status, d + o_status, o_scratch - o_status, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return orbgpu_fail(ORB_ERR_DEVICE, "CreateNewMapPoints device error");
    const int n_new = *reinterpret_cast<const int32_t*>(h + o_nnew);
    if (n_new < 0 || n_new > C) return orbgpu_fail(ORB_ERR_INTERNAL, "CreateNewMapPoints: record count out of range");
    memcpy(out->status, h + o_status, 4 * jobs);
    memcpy(out->x3d, h + o_x3d, 12 * jobs);
    memcpy(out->from_stereo, h + o_fs, jobs);
    memcpy(out->taken_by, h + o_taken, 4 * (size_t)C);
    memcpy(out->records, h + o_rec, sizeof(orb_newpoint_t) * (size_t)n_new);
    *out->n_new = n_new;
    return ORB_OK;
}

}  // extern "C"
