// csrc/orb_svd4.h compiled for the host as a small shared library (tests/test_newpoints_ref_cpu.py loads it
// with ctypes): the routine k_np_triangulate runs per thread, here over an array of 4x4 float matrices.
#include "../../orb-slam3_byzyh_amd/csrc/orb_svd4.h"

extern "C" void svd4_null_vectors(const float* a, int n, float* x) {
    for (int k = 0; k < n; ++k) {
        float m[4][4];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) m[r][c] = a[16 * k + 4 * r + c];
        orbgpu::svd4_null_vector(m, x + 4 * k);
    }
}
