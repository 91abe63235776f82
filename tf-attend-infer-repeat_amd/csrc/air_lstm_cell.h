// BasicLSTMCell forward (TF 1.3, air_model.py:286), the ONE definition: the fused GEMM epilogues (air_gemm_common.h)
// and the unfused kernels (air_pointwise.hip) are pinned bit for bit against each other, so they share the arithmetic.
#pragma once
#include "air_common.h"

// g = the pre-activations i, j, f, o of unit u (split(gates, 4, 1)); forget bias 1.0:
// c' = c*sigmoid(f + 1) + sigmoid(i)*tanh(j); h' = tanh(c')*sigmoid(o).
// acts = this row's [4R] activations, idx = row * R + u in c / h / h16 (h16: bf16 twin of h, may be null)
__device__ __forceinline__ void air_lstm_cell_fwd(const float (&g)[4], float c_prev, float* acts, float* c, float* h,
                                                  unsigned short* h16, int R, int u, size_t idx) {
    const float si = air_sigmoid(g[0]), tj = tanhf(g[1]);
    const float sf = air_sigmoid(g[2] + 1.0f), so = air_sigmoid(g[3]);
    const float cn = c_prev * sf + si * tj;
    acts[u] = si; acts[R + u] = tj; acts[2 * R + u] = sf; acts[3 * R + u] = so;
    c[idx] = cn;
    const float hn = tanhf(cn) * so;
    h[idx] = hn;
    if (h16) h16[idx] = air_bf16_of(hn);
}
