// One Sim3Solver hypothesis (reference src/Sim3Solver.cc:311-439) in registers: Horn's closed form in FP64 on
// float32 points, rounded to float32 once, and the float32 reprojection test of one correspondence.  Shared by
// the device (orb_sim3.hip) and the host (tests/native/sim3_host.cpp): plain C++, no runtime-indexed array,
// every loop over rows and columns unrolled.
//
// The reference solves the 4x4 eigenproblem with a float general solver and carries float through the rest;
// here everything up to T12 / T21 is double, so the result does not depend on the solver: with a relative gap
// g between the two largest eigenvalues the eigenvector is good to ~1e-16 / g, and the one rounding to float
// (6e-8 relative) is the whole error.  The eigenvector's sign does not matter: (w, v) -> (-w, -v) turns the
// angle 2 atan2(|v|, w) about v / |v| into 2 pi - that angle about -v / |v|, the same rotation.
//
// Nothing is special-cased: |v| = 0 (the two triples equal up to a translation) divides 0 by 0, the transform
// is NaN and every comparison of sim3_inlier is false, as in the reference.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ORB_SIM3_FN __host__ __device__ __forceinline__
#define ORB_SIM3_UNROLL _Pragma("unroll")
#else
#define ORB_SIM3_FN inline
#define ORB_SIM3_UNROLL
#endif

namespace orbgpu {

constexpr int kSim3MaxSweeps = 12;  // a symmetric 4x4 converges in 4-6; the cap only bounds a non-finite input

// One two-sided Jacobi rotation of the symmetric a (full storage) in the (P, Q) plane; v's columns follow.
// An exactly zero a[P][Q] is left alone, so a block-diagonal N keeps its exact zeros.
template <int P, int Q>
ORB_SIM3_FN bool sym4_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (!(fabs(apq) > 0.0)) return false;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
    if (s == 0.0) return false;  // a[P][Q] below the diagonal's last bit
    ORB_SIM3_UNROLL
    for (int k = 0; k < 4; ++k) {  // columns P, Q of every row
        const double kp = a[k][P], kq = a[k][Q];
        a[k][P] = c * kp - s * kq;
        a[k][Q] = s * kp + c * kq;
    }
    ORB_SIM3_UNROLL
    for (int k = 0; k < 4; ++k) {  // rows P, Q of every column
        const double pk = a[P][k], qk = a[Q][k];
        a[P][k] = c * pk - s * qk;
        a[Q][k] = s * pk + c * qk;
    }
    a[P][Q] = a[Q][P] = 0.0;
    ORB_SIM3_UNROLL
    for (int k = 0; k < 4; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
    return true;
}

// ComputeSim3 (:311-412).  p1, p2: the three sampled points of each set, [point][xyz].  T12 = [s R | t] and
// T21 = [(1/s) R^T | -(1/s) R^T t], both 3x4 row-major; *scale = s (1 when fix_scale).
ORB_SIM3_FN void sim3_closed_form(const float p1[3][3], const float p2[3][3], bool fix_scale, float T12[12],
                                  float T21[12], float* scale) {
    // step 1: centroids and relative coordinates
    double O1[3], O2[3], r1[3][3], r2[3][3];
    ORB_SIM3_UNROLL
    for (int k = 0; k < 3; ++k) {
        O1[k] = ((double)p1[0][k] + (double)p1[1][k] + (double)p1[2][k]) / 3.0;
        O2[k] = ((double)p2[0][k] + (double)p2[1][k] + (double)p2[2][k]) / 3.0;
    }
    ORB_SIM3_UNROLL
    for (int i = 0; i < 3; ++i) {
        ORB_SIM3_UNROLL
        for (int k = 0; k < 3; ++k) {
            r1[i][k] = (double)p1[i][k] - O1[k];
            r2[i][k] = (double)p2[i][k] - O2[k];
        }
    }
    // step 2: M = Pr2 Pr1^T (the points are the columns of Pr)
    double M[3][3];
    ORB_SIM3_UNROLL
    for (int a = 0; a < 3; ++a) {
        ORB_SIM3_UNROLL
        for (int b = 0; b < 3; ++b) M[a][b] = r2[0][a] * r1[0][b] + r2[1][a] * r1[1][b] + r2[2][a] * r1[2][b];
    }
    // step 3: Horn's N
    double N[4][4];
    N[0][0] = M[0][0] + M[1][1] + M[2][2];
    N[0][1] = N[1][0] = M[1][2] - M[2][1];
    N[0][2] = N[2][0] = M[2][0] - M[0][2];
    N[0][3] = N[3][0] = M[0][1] - M[1][0];
    N[1][1] = M[0][0] - M[1][1] - M[2][2];
    N[1][2] = N[2][1] = M[0][1] + M[1][0];
    N[1][3] = N[3][1] = M[2][0] + M[0][2];
    N[2][2] = -M[0][0] + M[1][1] - M[2][2];
    N[2][3] = N[3][2] = M[1][2] + M[2][1];
    N[3][3] = -M[0][0] - M[1][1] + M[2][2];
    // step 4: the eigenvector of the largest eigenvalue (the first one on a tie)
    double V[4][4] = {{1., 0., 0., 0.}, {0., 1., 0., 0.}, {0., 0., 1., 0.}, {0., 0., 0., 1.}};
    for (int sweep = 0; sweep < kSim3MaxSweeps; ++sweep) {
        bool any = sym4_rotate<0, 1>(N, V);
        any |= sym4_rotate<0, 2>(N, V);
        any |= sym4_rotate<0, 3>(N, V);
        any |= sym4_rotate<1, 2>(N, V);
        any |= sym4_rotate<1, 3>(N, V);
        any |= sym4_rotate<2, 3>(N, V);
        if (!any) break;
    }
    double lmax = N[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
    ORB_SIM3_UNROLL
    for (int c = 1; c < 4; ++c) {
        if (N[c][c] > lmax) {
            lmax = N[c][c];
            qw = V[0][c]; qx = V[1][c]; qy = V[2][c]; qz = V[3][c];
        }
    }
    // the rotation vector 2 atan2(|v|, w) v / |v| and its exponential (Rodrigues)
    const double vn = sqrt(qx * qx + qy * qy + qz * qz);
    const double ang = 2.0 * atan2(vn, qw);
    const double ax = qx / vn, ay = qy / vn, az = qz / vn;
    const double sn = sin(ang), cs = cos(ang), oc = 1.0 - cs;
    double R[3][3];
    R[0][0] = cs + oc * ax * ax;      R[0][1] = oc * ax * ay - sn * az; R[0][2] = oc * ax * az + sn * ay;
    R[1][0] = oc * ax * ay + sn * az; R[1][1] = cs + oc * ay * ay;      R[1][2] = oc * ay * az - sn * ax;
    R[2][0] = oc * ax * az - sn * ay; R[2][1] = oc * ay * az + sn * ax; R[2][2] = cs + oc * az * az;
    // steps 5, 6: rotate set 2; s = <Pr1, P3> / <P3, P3>
    double s = 1.0;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
        ORB_SIM3_UNROLL
        for (int i = 0; i < 3; ++i) {
            ORB_SIM3_UNROLL
            for (int a = 0; a < 3; ++a) {
                const double p3 = R[a][0] * r2[i][0] + R[a][1] * r2[i][1] + R[a][2] * r2[i][2];
                nom += r1[i][a] * p3;
                den += p3 * p3;
            }
        }
        s = nom / den;
    }
    // steps 7, 8: t = O1 - s R O2; T12 = [s R | t]; T21 = [(1/s) R^T | -(1/s) R^T t]
    double t[3];
    ORB_SIM3_UNROLL
    for (int a = 0; a < 3; ++a) t[a] = O1[a] - s * (R[a][0] * O2[0] + R[a][1] * O2[1] + R[a][2] * O2[2]);
    const double is = 1.0 / s;
    ORB_SIM3_UNROLL
    for (int a = 0; a < 3; ++a) {
        ORB_SIM3_UNROLL
        for (int b = 0; b < 3; ++b) {
            T12[4 * a + b] = (float)(s * R[a][b]);
            T21[4 * a + b] = (float)(is * R[b][a]);
        }
        T12[4 * a + 3] = (float)t[a];
        T21[4 * a + 3] = (float)(-is * (R[0][a] * t[0] + R[1][a] * t[1] + R[2][a] * t[2]));
    }
    *scale = (float)s;
}

// Pinhole::project of T X in float, no contraction: ((r0 x + r1 y) + r2 z) + t, then fx * x / z + cx.
ORB_SIM3_FN void sim3_project(const float T[12], const float X[3], const float cam[4], float* u, float* v) {
    const float x = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[3];
    const float y = ((T[4] * X[0] + T[5] * X[1]) + T[6] * X[2]) + T[7];
    const float z = ((T[8] * X[0] + T[9] * X[1]) + T[10] * X[2]) + T[11];
    *u = cam[0] * x / z + cam[2];
    *v = cam[1] * y / z + cam[3];
}

// CheckInliers (:415-439) for one correspondence: im1 / im2 are the points' own projections (mvP1im1, mvP2im2).
ORB_SIM3_FN bool sim3_inlier(const float T12[12], const float T21[12], const float X1[3], const float X2[3],
                             const float im1[2], const float im2[2], const float cam1[4], const float cam2[4],
                             float max_err1, float max_err2) {
    float u, v;
    sim3_project(T12, X2, cam1, &u, &v);
    const float ax = im1[0] - u, ay = im1[1] - v;
    const float err1 = ax * ax + ay * ay;
    sim3_project(T21, X1, cam2, &u, &v);
    const float bx = u - im2[0], by = v - im2[1];
    const float err2 = bx * bx + by * by;
    return err1 < max_err1 && err2 < max_err2;
}

}  // namespace orbgpu
