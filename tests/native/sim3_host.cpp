// csrc/orb_sim3_math.h compiled for the host as a small shared library (tests/test_sim3_ref_cpu.py loads it with
// ctypes): the closed form and the inlier test k_sim3_hypotheses runs per lane, here in two plain loops over one
// problem.  bits: n_hyp x n bytes.
#include <cstdint>

#include "../../orb-slam3_byzyh_amd/csrc/orb_sim3_math.h"

extern "C" void sim3_host_evaluate(int n, const float* x1, const float* x2, const float* e1, const float* e2,
                                   const float* cam1, const float* cam2, int fix_scale, int n_hyp,
                                   const int32_t* samples, float* t12, float* scale, uint8_t* bits) {
    for (int h = 0; h < n_hyp; ++h) {
        float p1[3][3], p2[3][3], T12[12], T21[12];
        for (int k = 0; k < 3; ++k) {
            for (int c = 0; c < 3; ++c) {
                p1[k][c] = x1[3 * samples[3 * h + k] + c];
                p2[k][c] = x2[3 * samples[3 * h + k] + c];
            }
        }
        orbgpu::sim3_closed_form(p1, p2, fix_scale != 0, T12, T21, &scale[h]);
        for (int k = 0; k < 12; ++k) t12[12 * h + k] = T12[k];
        for (int i = 0; i < n; ++i) {
            const float* X1 = &x1[3 * i];
            const float* X2 = &x2[3 * i];
            const float im1[2] = {cam1[0] * X1[0] / X1[2] + cam1[2], cam1[1] * X1[1] / X1[2] + cam1[3]};
            const float im2[2] = {cam2[0] * X2[0] / X2[2] + cam2[2], cam2[1] * X2[1] / X2[2] + cam2[3]};
            bits[(long)h * n + i] = orbgpu::sim3_inlier(T12, T21, X1, X2, im1, im2, cam1, cam2, e1[i], e2[i]) ? 1 : 0;
        }
    }
}
