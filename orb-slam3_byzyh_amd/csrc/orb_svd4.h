// The null vector of a 4x4 float matrix by one-sided (Hestenes) Jacobi, in float, in registers: the solve
// behind GeometricTools::Triangulate's `JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().col(3)` (reference
// src/GeometricTools.cc:79-81).  Shared by the device (orb_newpoints.hip) and the host (tests/native,
// tools): plain C++, no runtime-indexed array, every loop over columns unrolled by the template.
//
// The rotations act on the columns of A itself (never on A^T A, which would square the condition number):
// columns p < q are rotated until every pair is orthogonal to float precision, V accumulates the same
// rotations, and the answer is the column of V whose column of A V has the smallest norm.  Sums are plain
// float with explicit fmaf.  The result is not bit-identical to Eigen's two-sided solver; its accuracy is
// what tests/test_newpoints_gpu.py bounds against a float64 SVD of the same float32 A, with LAPACK's
// single-precision sgesdd as the yardstick.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ORB_SVD4_FN __host__ __device__ __forceinline__
#define ORB_SVD4_UNROLL _Pragma("unroll")
#else
#define ORB_SVD4_FN inline
#define ORB_SVD4_UNROLL
#endif

namespace orbgpu {

constexpr int kSvd4MaxSweeps = 12;  // 4x4 converges in 3-5; the cap only bounds a non-finite input

// one column pair (P, Q) of a sweep; returns whether it rotated
template <int P, int Q>
ORB_SVD4_FN bool svd4_rotate(float (&a)[4][4], float (&v)[4][4]) {
    const float alpha = fmaf(a[3][P], a[3][P], fmaf(a[2][P], a[2][P], fmaf(a[1][P], a[1][P], a[0][P] * a[0][P])));
    const float beta = fmaf(a[3][Q], a[3][Q], fmaf(a[2][Q], a[2][Q], fmaf(a[1][Q], a[1][Q], a[0][Q] * a[0][Q])));
    const float gamma = fmaf(a[3][P], a[3][Q], fmaf(a[2][P], a[2][Q], fmaf(a[1][P], a[1][Q], a[0][P] * a[0][Q])));
    // orthogonal to working precision (also false for a NaN, which ends the iteration)
    if (!(fabsf(gamma) > 5.9604645e-08f * sqrtf(alpha * beta))) return false;
    const float zeta = (beta - alpha) / (2.0f * gamma);
    const float t = copysignf(1.0f, zeta) / (fabsf(zeta) + sqrtf(fmaf(zeta, zeta, 1.0f)));
    const float c = 1.0f / sqrtf(fmaf(t, t, 1.0f)), s = c * t;
    ORB_SVD4_UNROLL
    for (int r = 0; r < 4; ++r) {
        const float ap = a[r][P], aq = a[r][Q];
        a[r][P] = fmaf(c, ap, -(s * aq));
        a[r][Q] = fmaf(s, ap, c * aq);
        const float vp = v[r][P], vq = v[r][Q];
        v[r][P] = fmaf(c, vp, -(s * vq));
        v[r][Q] = fmaf(s, vp, c * vq);
    }
    return true;
}

// x (4): the unit right singular vector of the smallest singular value of `a` (row-major, destroyed).
ORB_SVD4_FN void svd4_null_vector(float (&a)[4][4], float x[4]) {
    float v[4][4] = {{1.f, 0.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 1.f, 0.f}, {0.f, 0.f, 0.f, 1.f}};
    for (int sweep = 0; sweep < kSvd4MaxSweeps; ++sweep) {
        bool any = svd4_rotate<0, 1>(a, v);
        any |= svd4_rotate<0, 2>(a, v);
        any |= svd4_rotate<0, 3>(a, v);
        any |= svd4_rotate<1, 2>(a, v);
        any |= svd4_rotate<1, 3>(a, v);
        any |= svd4_rotate<2, 3>(a, v);
        if (!any) break;
    }
    float best = INFINITY;
    x[0] = v[0][0]; x[1] = v[1][0]; x[2] = v[2][0]; x[3] = v[3][0];
    ORB_SVD4_UNROLL
    for (int c = 0; c < 4; ++c) {
        const float n2 = fmaf(a[3][c], a[3][c], fmaf(a[2][c], a[2][c], fmaf(a[1][c], a[1][c], a[0][c] * a[0][c])));
        if (n2 < best) {
            best = n2;
            x[0] = v[0][c]; x[1] = v[1][c]; x[2] = v[2][c]; x[3] = v[3][c];
        }
    }
}

}  // namespace orbgpu
