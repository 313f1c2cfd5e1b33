// The arithmetic of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494) in FP64: g2o::Sim3
// (Thirdparty/g2o/g2o/types/sim3.h), the two reprojection edges of include/OptimizableTypes.h:194-235, their
// numeric linearisation (core/base_binary_edge.hpp:131-205: central differences, delta 1e-9), the dense 7x7
// LDL^T and the Levenberg-Marquardt controller of core/optimization_algorithm_levenberg.cpp:61-194.  Shared by
// the device (orb_optsim3.hip) and the host (tests/native/optsim3_host.cpp): plain C++, no runtime-indexed
// local array, every loop over rows and columns unrolled, no contraction.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define ORB_OS3_FN __host__ __device__ __forceinline__
#define ORB_OS3_UNROLL _Pragma("unroll")
#else
#define ORB_OS3_FN inline
#define ORB_OS3_UNROLL
#endif
// On the device the 15 estimates and their inverses (240 doubles) are read from LDS where they are used: without
// this compiler barrier the loads are hoisted out of the loop over a thread's pairs and the kernel spills.
#if defined(__HIP_DEVICE_COMPILE__)
#define ORB_OS3_REREAD()              \
    asm volatile("" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#else
#define ORB_OS3_REREAD()
#endif

namespace orbgpu {

constexpr double kOptSim3Delta = 1e-9;                        // base_binary_edge.hpp:147
constexpr double kOptSim3Scalar = 1.0 / (2 * kOptSim3Delta);  // :148
constexpr int kOptSim3Acc = 36;  // H's upper triangle row by row (28), b (7), the robust chi2

struct Sim3d {  // g2o::Sim3: r (x y z w, as Eigen stores it), t, s
    double q[4], t[3], s;
};

// One gathered pair: 88 bytes
struct OptSim3Pair {
    double p1[3], p2[3];  // P3D1c, P3D2c
    double o1[2], o2[2];  // obs1, obs2
    float is1, is2;       // the edges' information
};

// Eigen's Quaternion * Vector3 (_transformVector): uv = 2 q.vec x v; v + w uv + q.vec x uv
ORB_OS3_FN void os3_qrotate(const double q[4], const double v[3], double o[3]) {
    const double uv0 = 2 * (q[1] * v[2] - q[2] * v[1]);
    const double uv1 = 2 * (q[2] * v[0] - q[0] * v[2]);
    const double uv2 = 2 * (q[0] * v[1] - q[1] * v[0]);
    o[0] = v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
    o[1] = v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
    o[2] = v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}

// Eigen's quaternion product, not re-normalised
ORB_OS3_FN void os3_qmul(const double a[4], const double b[4], double o[4]) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaterniond(Matrix3d), m row-major
ORB_OS3_FN void os3_qfrom_matrix(const double m[9], double q[4]) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else if (m[4] <= m[0] && m[8] <= m[0]) {
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t;
        q[1] = (m[3] + m[1]) * t;
        q[2] = (m[6] + m[2]) * t;
    } else if (m[8] <= m[4]) {
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t;
        q[2] = (m[7] + m[5]) * t;
        q[0] = (m[1] + m[3]) * t;
    } else {
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t;
        q[0] = (m[2] + m[6]) * t;
        q[1] = (m[5] + m[7]) * t;
    }
}

// Sim3(const Vector7d& update) (sim3.h:70-142): omega, upsilon, sigma; all four eps branches
ORB_OS3_FN Sim3d sim3_exp(const double u[7]) {
    Sim3d S;
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double O2[9];
    ORB_OS3_UNROLL
    for (int i = 0; i < 3; ++i) {
        ORB_OS3_UNROLL
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    }
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, ra = 1.0, rb = 1.0;  // R = I + ra Omega + rb Omega2
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            ra = sin(theta) / theta;
            rb = (1 - cos(theta)) / (theta * theta);
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    double R[9], W[9];
    ORB_OS3_UNROLL
    for (int k = 0; k < 9; ++k) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        R[k] = I + ra * O[k] + rb * O2[k];
        W[k] = A * O[k] + B * O2[k] + C * I;
    }
    os3_qfrom_matrix(R, S.q);
    ORB_OS3_UNROLL
    for (int i = 0; i < 3; ++i) S.t[i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    return S;
}

// map (:144): s (r xyz) + t
ORB_OS3_FN void sim3_map(const Sim3d& S, const double x[3], double o[3]) {
    double r[3];
    os3_qrotate(S.q, x, r);
    ORB_OS3_UNROLL
    for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}

// inverse (:233): Sim3(r.conjugate(), r.conjugate() * ((-1 / s) t), 1 / s)
ORB_OS3_FN Sim3d sim3_inverse(const Sim3d& S) {
    Sim3d I;
    I.q[0] = -S.q[0]; I.q[1] = -S.q[1]; I.q[2] = -S.q[2]; I.q[3] = S.q[3];
    const double f = -1. / S.s;
    const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    os3_qrotate(I.q, v, I.t);
    I.s = 1. / S.s;
    return I;
}

// operator* (:266)
ORB_OS3_FN Sim3d sim3_mul(const Sim3d& a, const Sim3d& b) {
    Sim3d r;
    os3_qmul(a.q, b.q, r.q);
    double rt[3];
    os3_qrotate(a.q, b.t, rt);
    ORB_OS3_UNROLL
    for (int i = 0; i < 3; ++i) r.t[i] = a.s * rt[i] + a.t[i];
    r.s = a.s * b.s;
    return r;
}

// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:177-186): _fix_scale zeroes update[6]
ORB_OS3_FN Sim3d optsim3_oplus(const Sim3d& S, const double u[7], bool fix_scale) {
    const double v[7] = {u[0], u[1], u[2], u[3], u[4], u[5], fix_scale ? 0.0 : u[6]};
    return sim3_mul(sim3_exp(v), S);
}

// The estimate perturbed for central difference k: dimension k >> 1, +delta for even k, -delta for odd k
ORB_OS3_FN Sim3d optsim3_perturbed(const Sim3d& S, int k, bool fix_scale) {
    double u[7];
    ORB_OS3_UNROLL
    for (int d = 0; d < 7; ++d) u[d] = (k >> 1) == d ? ((k & 1) ? -kOptSim3Delta : kOptSim3Delta) : 0.0;
    return optsim3_oplus(S, u, fix_scale);
}

// Pinhole::project(Vector3d): float parameters promoted
ORB_OS3_FN void os3_project(const float cam[4], const double X[3], double uv[2]) {
    uv[0] = (double)cam[0] * X[0] / X[2] + (double)cam[2];
    uv[1] = (double)cam[1] * X[1] / X[2] + (double)cam[3];
}

// obs - project(T.map(X)): EdgeSim3ProjectXYZ::computeError with T = S, X = P3D2c, camera 1 (e12), and
// EdgeInverseSim3ProjectXYZ::computeError with T = S.inverse(), X = P3D1c, camera 2 (e21)
ORB_OS3_FN void os3_edge_error(const Sim3d& T, const double X[3], const float cam[4], const double obs[2], double e[2]) {
    double Y[3], uv[2];
    sim3_map(T, X, Y);
    os3_project(cam, Y, uv);
    e[0] = obs[0] - uv[0];
    e[1] = obs[1] - uv[1];
}
ORB_OS3_FN void optsim3_errors(const Sim3d& S, const Sim3d& Si, const OptSim3Pair& p, const float cam1[4],
                               const float cam2[4], double e12[2], double e21[2]) {
    os3_edge_error(S, p.p2, cam1, p.o1, e12);
    os3_edge_error(Si, p.p1, cam2, p.o2, e21);
}

ORB_OS3_FN double os3_chi2(const double e[2], float info) {
    const double w = (double)info;
    return e[0] * w * e[0] + e[1] * w * e[1];
}

// RobustKernelHuber with its float dsqr member (robust_kernel_impl.cpp:78-91)
struct OptSim3Huber {
    double delta;
    float dsqr;
};
ORB_OS3_FN OptSim3Huber optsim3_huber(float th2) {
    OptSim3Huber h;
    const float d = sqrtf(th2);  // const float deltaHuber = sqrt(th2)
    h.delta = d;
    h.dsqr = (float)((double)d * (double)d);
    return h;
}
ORB_OS3_FN void os3_robustify(const OptSim3Huber& h, bool robust, double e, double& rho0, double& rho1) {
    if (!robust || e <= (double)h.dsqr) {
        rho0 = e;
        rho1 = 1.0;
    } else {
        const double sqrte = sqrt(e);
        rho0 = 2 * sqrte * h.delta - (double)h.dsqr;
        rho1 = h.delta / sqrte;
    }
}

// One edge's share of J^T W J, -J^T W e and the robust chi2 (constructQuadraticForm, base_binary_edge.hpp:91-113)
ORB_OS3_FN void os3_accumulate(const double (&J0)[7], const double (&J1)[7], const double e[2], float info,
                               const OptSim3Huber& h, bool robust, double (&acc)[kOptSim3Acc]) {
    double rho0, rho1;
    os3_robustify(h, robust, os3_chi2(e, info), rho0, rho1);
    acc[35] += rho0;
    const double w = rho1 * (double)info;
    int k = 0;
    ORB_OS3_UNROLL
    for (int i = 0; i < 7; ++i) {
        const double a0 = J0[i] * w, a1 = J1[i] * w;
        ORB_OS3_UNROLL
        for (int j = i; j < 7; ++j, ++k) acc[k] += a0 * J0[j] + a1 * J1[j];
        acc[28 + i] -= a0 * e[0] + a1 * e[1];
    }
}

// One edge's linearisation: T[14] the transform at the estimate (S for e12, S.inverse() for e21), T[k] at the
// 14 perturbed estimates of optsim3_perturbed; the error at the estimate, the 14 evaluations, the edge's share.
// nd: 6 when the scale is fixed (column 6 is exactly zero: both evaluations see the same estimate), else 7.
ORB_OS3_FN double os3_linearize_edge(const Sim3d* T, const double X[3], const float cam[4], const double obs[2],
                                     float info, const OptSim3Huber& h, bool robust, int nd,
                                     double (&acc)[kOptSim3Acc]) {
    double e[2];
    os3_edge_error(T[14], X, cam, obs, e);
    double J0[7], J1[7];
    ORB_OS3_UNROLL
    for (int d = 0; d < 7; ++d) {
        J0[d] = J1[d] = 0.0;
        if (d < nd) {
            ORB_OS3_REREAD();
            double ep[2], em[2];
            os3_edge_error(T[2 * d], X, cam, obs, ep);
            os3_edge_error(T[2 * d + 1], X, cam, obs, em);
            J0[d] = kOptSim3Scalar * (ep[0] - em[0]);
            J1[d] = kOptSim3Scalar * (ep[1] - em[1]);
        }
    }
    ORB_OS3_REREAD();
    os3_accumulate(J0, J1, e, info, h, robust, acc);
    return os3_chi2(e, info);
}

// A pair's linearisation with the estimates Pm[15] and their inverses Pi[15]: e12, then e21
ORB_OS3_FN void optsim3_linearize_pair(const Sim3d* Pm, const Sim3d* Pi, const OptSim3Pair& p, const float cam1[4],
                                       const float cam2[4], const OptSim3Huber& h, bool robust, int nd,
                                       double (&acc)[kOptSim3Acc], double& chi12, double& chi21) {
    chi12 = os3_linearize_edge(Pm, p.p2, cam1, p.o1, p.is1, h, robust, nd, acc);
    chi21 = os3_linearize_edge(Pi, p.p1, cam2, p.o2, p.is2, h, robust, nd, acc);
}

// A pair's errors at the estimate S (inverse Si): both chi2 and the robust chi2 they add
ORB_OS3_FN double optsim3_error_pair(const Sim3d& S, const Sim3d& Si, const OptSim3Pair& p, const float cam1[4],
                                     const float cam2[4], const OptSim3Huber& h, bool robust, double& chi12,
                                     double& chi21) {
    double e12[2], e21[2], r0, r1, s0;
    optsim3_errors(S, Si, p, cam1, cam2, e12, e21);
    chi12 = os3_chi2(e12, p.is1);
    chi21 = os3_chi2(e21, p.is2);
    os3_robustify(h, robust, chi12, r0, r1);
    os3_robustify(h, robust, chi21, s0, r1);
    return r0 + s0;
}

// (H + lambda I) x = b by LDL^T without pivoting (LinearSolverDense's Eigen::LDLT up to rounding); sys: H's upper
// triangle row by row, then b.  Returns LDLT::isPositive's answer: no negative pivot (and none zero, which the
// division needs).
ORB_OS3_FN bool optsim3_solve7(const double* sys, double lambda, double (&x)[7]) {
    double M[7][7], Lm[7][7], d[7];
    {
        int k = 0;
        ORB_OS3_UNROLL
        for (int i = 0; i < 7; ++i) {
            ORB_OS3_UNROLL
            for (int j = i; j < 7; ++j, ++k) M[i][j] = sys[k] + (i == j ? lambda : 0.0);
        }
    }
    bool ok = true;
    ORB_OS3_UNROLL
    for (int j = 0; j < 7; ++j) {
        double dj = M[j][j];
        ORB_OS3_UNROLL
        for (int k = 0; k < j; ++k) dj -= Lm[j][k] * Lm[j][k] * d[k];
        ok = ok && dj > 0;
        d[j] = dj;
        ORB_OS3_UNROLL
        for (int i = j + 1; i < 7; ++i) {
            double v = M[j][i];
            ORB_OS3_UNROLL
            for (int k = 0; k < j; ++k) v -= Lm[i][k] * Lm[j][k] * d[k];
            Lm[i][j] = v / dj;
        }
    }
    ORB_OS3_UNROLL
    for (int i = 0; i < 7; ++i) {
        x[i] = sys[28 + i];
        ORB_OS3_UNROLL
        for (int k = 0; k < i; ++k) x[i] -= Lm[i][k] * x[k];
    }
    ORB_OS3_UNROLL
    for (int i = 0; i < 7; ++i) x[i] /= d[i];
    ORB_OS3_UNROLL
    for (int i = 6; i >= 0; --i) {
        ORB_OS3_UNROLL
        for (int k = i + 1; k < 7; ++k) x[i] -= Lm[k][i] * x[k];
    }
    if (!ok) {
        ORB_OS3_UNROLL
        for (int i = 0; i < 7; ++i) x[i] = 0.0;
    }
    return ok;
}

// OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize(iters), as oracle/orb_pose_oracle.cpp
// restates it: lambda0 = 1e-5 max |diag H| at the first iteration of every optimize(), rho against
// x . (lambda x + b) + 1e-3, lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)) on an acceptance, lambda *= ni,
// ni *= 2 on a rejection, at most 10 trials, stop on 10 trials, rho == 0, three iterations in a row with a
// relative decrease below 1e-3, or `iters` iterations.
struct OptSim3Lm {
    double lambda, ni, current, ini;
    int nbad, qmax, it, iters;
};
enum { kOptSim3Trial = 1, kOptSim3NextIteration = 2, kOptSim3Done = 3 };

ORB_OS3_FN void optsim3_lm_begin(OptSim3Lm& L, int iters) {
    L.lambda = 0;
    L.ni = 2;
    L.current = L.ini = 0;
    L.nbad = L.qmax = L.it = 0;
    L.iters = iters;
}
// after the linearisation at the estimate (sys: 28 H, 7 b, the robust chi2)
ORB_OS3_FN void optsim3_lm_iteration(OptSim3Lm& L, const double* sys) {
    L.current = L.ini = sys[35];
    if (L.it == 0) {  // computeLambdaInit: tau * max |diag H|
        double m = 0;
        int k = 0;
        ORB_OS3_UNROLL
        for (int i = 0; i < 7; ++i) {
            m = fmax(fabs(sys[k]), m);
            k += 7 - i;
        }
        L.lambda = 1e-5 * m;
        L.ni = 2;
        L.nbad = 0;
    }
    L.qmax = 0;
}
// after the trial's error pass; b = sys + 28.  accept: the trial estimate becomes the estimate.
ORB_OS3_FN int optsim3_lm_decide(OptSim3Lm& L, double tempChi, bool ok, const double (&x)[7], const double* b,
                                 bool& accept) {
    if (!ok) tempChi = DBL_MAX;
    double rho = L.current - tempChi;
    double scale = 0;
    ORB_OS3_UNROLL
    for (int i = 0; i < 7; ++i) scale += x[i] * (L.lambda * x[i] + b[i]);
    scale += 1e-3;
    rho /= scale;
    accept = rho > 0 && std::isfinite(tempChi);
    if (accept) {
        const double c = 2 * rho - 1;
        double alpha = 1. - c * c * c;
        alpha = fmin(alpha, 2. / 3.);
        L.lambda *= fmax(1. / 3., alpha);
        L.ni = 2;
        L.current = tempChi;
    } else {
        L.lambda *= L.ni;
        L.ni *= 2;
    }
    L.qmax++;
    if (rho < 0 && L.qmax < 10) return kOptSim3Trial;
    if (L.qmax == 10 || rho == 0) return kOptSim3Done;
    if ((L.ini - L.current) * 1e3 < L.ini) L.nbad++;
    else L.nbad = 0;
    if (L.nbad >= 3) return kOptSim3Done;
    if (++L.it >= L.iters) return kOptSim3Done;
    return kOptSim3NextIteration;
}

}  // namespace orbgpu
