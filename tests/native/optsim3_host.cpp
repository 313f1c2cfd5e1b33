// csrc/orb_optsim3_math.h compiled for the host as a small shared library (tests/optsim3_ref.py loads it with
// ctypes): Sim3(update), one error pair, one 14-evaluation Jacobian, and the whole schedule of k_optsim3 in plain
// serial loops over one problem (the same functions, the pairs summed in index order instead of the kernel's
// butterfly).
#include <cstdint>
#include <vector>

#include "../../orb-slam3_byzyh_amd/csrc/orb_optsim3_math.h"

using namespace orbgpu;

namespace {

Sim3d from_vector(const double* v) {
    Sim3d S;
    for (int k = 0; k < 4; ++k) S.q[k] = v[k];
    for (int k = 0; k < 3; ++k) S.t[k] = v[4 + k];
    S.s = v[7];
    return S;
}
void to_vector(const Sim3d& S, double* v) {
    for (int k = 0; k < 4; ++k) v[k] = S.q[k];
    for (int k = 0; k < 3; ++k) v[4 + k] = S.t[k];
    v[7] = S.s;
}
OptSim3Pair pair_of(int i, const double* p1, const double* p2, const double* o1, const double* o2, const float* is1,
                    const float* is2) {
    OptSim3Pair p;
    for (int k = 0; k < 3; ++k) {
        p.p1[k] = p1[3 * i + k];
        p.p2[k] = p2[3 * i + k];
    }
    for (int k = 0; k < 2; ++k) {
        p.o1[k] = o1[2 * i + k];
        p.o2[k] = o2[2 * i + k];
    }
    p.is1 = is1[i];
    p.is2 = is2[i];
    return p;
}

}  // namespace

extern "C" {

void optsim3_host_exp(const double* update, double* out8) { to_vector(sim3_exp(update), out8); }

// pair88: one OptSim3Pair; cams: cam1 then cam2; e: e12 then e21
void optsim3_host_errors(const double* s12, const void* pair88, const float* cam1, const float* cam2, double* e) {
    const Sim3d S = from_vector(s12);
    optsim3_errors(S, sim3_inverse(S), *static_cast<const OptSim3Pair*>(pair88), cam1, cam2, e, e + 2);
}

// J12, J21: 2 x 7 row-major each
void optsim3_host_jacobian(const double* s12, int fix_scale, const void* pair88, const float* cam1, const float* cam2,
                           double* J12, double* J21) {
    const Sim3d S = from_vector(s12);
    const OptSim3Pair& p = *static_cast<const OptSim3Pair*>(pair88);
    for (int d = 0; d < 7; ++d) {
        const Sim3d Sp = optsim3_perturbed(S, 2 * d, fix_scale != 0), Sm = optsim3_perturbed(S, 2 * d + 1, fix_scale != 0);
        double ap[2], bp[2], am[2], bm[2];
        optsim3_errors(Sp, sim3_inverse(Sp), p, cam1, cam2, ap, bp);
        optsim3_errors(Sm, sim3_inverse(Sm), p, cam1, cam2, am, bm);
        for (int r = 0; r < 2; ++r) {
            J12[7 * r + d] = kOptSim3Scalar * (ap[r] - am[r]);
            J21[7 * r + d] = kOptSim3Scalar * (bp[r] - bm[r]);
        }
    }
}

void optsim3_host_solve(int n, const double* p1, const double* p2, const double* o1, const double* o2, const float* is1,
                        const float* is2, const float* cam1, const float* cam2, const double* s12, float th2f,
                        int fix_scale, double* s12_out, int32_t* n_in_bad, uint8_t* inlier, double* chi12, double* chi21,
                        int32_t* trials) {
    const bool fix = fix_scale != 0;
    const int nd = fix ? 6 : 7;
    const OptSim3Huber hub = optsim3_huber(th2f);
    const double th2 = (double)th2f;
    for (int k = 0; k < 8; ++k) s12_out[k] = s12[k];
    n_in_bad[0] = n_in_bad[1] = 0;
    trials[0] = trials[1] = 0;
    if (n == 0) return;
    std::vector<uint8_t> bad(n, 0);
    Sim3d cur = from_vector(s12);
    auto errors = [&](const Sim3d& S, bool robust) {
        const Sim3d Si = sim3_inverse(S);
        double sum = 0;
        for (int i = 0; i < n; ++i)
            if (!bad[i]) sum += optsim3_error_pair(S, Si, pair_of(i, p1, p2, o1, o2, is1, is2), cam1, cam2, hub, robust, chi12[i], chi21[i]);
        return sum;
    };
    auto optimize = [&](int iters, bool robust, int32_t& ntrials) {
        OptSim3Lm lm;
        optsim3_lm_begin(lm, iters);
        for (;;) {
            Sim3d P[15], Pi[15];
            for (int k = 0; k < 14; ++k) P[k] = optsim3_perturbed(cur, k, fix);
            P[14] = cur;
            for (int k = 0; k < 15; ++k) Pi[k] = sim3_inverse(P[k]);
            double sys[kOptSim3Acc] = {};
            for (int i = 0; i < n; ++i)
                if (!bad[i])
                    optsim3_linearize_pair(P, Pi, pair_of(i, p1, p2, o1, o2, is1, is2), cam1, cam2, hub, robust, nd, sys, chi12[i], chi21[i]);
            optsim3_lm_iteration(lm, sys);
            int cmd;
            for (;;) {
                double x[7];
                const bool ok = optsim3_solve7(sys, lm.lambda, x);
                const Sim3d T = optsim3_oplus(cur, x, fix);
                const double temp = errors(T, robust);
                ++ntrials;
                bool accept;
                cmd = optsim3_lm_decide(lm, temp, ok, x, sys + 28, accept);
                if (accept) cur = T;
                if (cmd != kOptSim3Trial) break;
            }
            if (cmd == kOptSim3Done) break;
        }
    };
    optimize(5, true, trials[0]);
    int nBad = 0;
    for (int i = 0; i < n; ++i) {
        bad[i] = chi12[i] > th2 || chi21[i] > th2;
        nBad += bad[i];
        inlier[i] = !bad[i];
    }
    n_in_bad[1] = nBad;
    if (n - nBad < 10) return;
    optimize(nBad > 0 ? 10 : 5, false, trials[1]);
    (void)errors(cur, false);
    int nIn = 0;
    for (int i = 0; i < n; ++i) {
        inlier[i] = !bad[i] && !(chi12[i] > th2 || chi21[i] > th2);
        nIn += inlier[i];
    }
    n_in_bad[0] = nIn;
    to_vector(cur, s12_out);
}

}  // extern "C"
