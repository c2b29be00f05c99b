// fp64 building blocks shared by ops_f64.hip and layer_f64.hip (the --double path). Plain VALU fp64, one fixed
// summation order per output element: bitwise reproducible, no floating-point atomics.
#pragma once
#include "common.h"

// Y[r, c] (row stride ldy) = (accumulate ? Y[r, c] : 0) + (b ? b[c] : 0) + sum_k X[r*ldx + k] * W[c*wsc + k*wsk]
// for r < R, c < C, k < K (k ascending).
int pvs64_gemm(hipStream_t s, double* Y, int ldy, const double* X, int ldx, const double* W, int wsc, int wsk,
               const double* b, int R, int K, int C, bool accumulate);

// G[c*ldg + k] = (accumulate ? G : 0) + sum_r A[r*lda + c] * (B ? B[r*ldb + k] : 1), c < C, k < K.
// Rows are summed in fixed slabs (their number depends on R only), the slabs in ascending order.
// slabs: pvs64_atb_slab_doubles(R, C, K) doubles of scratch.
size_t pvs64_atb_slab_doubles(int R, int C, int K);
int pvs64_atb(hipStream_t s, double* G, int ldg, const double* A, int lda, const double* B, int ldb, int R, int C,
              int K, double* slabs, bool accumulate);

// out[c] = sum_r A[r*lda + c], c < C: the column sums (bias gradients and the like) as pvs64_atb without a right operand.
inline int pvs64_colsum(hipStream_t s, double* out, const double* A, int lda, int R, int C, double* slabs) {
    return pvs64_atb(s, out, 1, A, lda, nullptr, 0, R, C, 1, slabs, false);
}

// Largest C*K the layer hands to pvs64_atb (the slab scratch it reserves).
#define PVS64_MAX_ATB_OUT (64 * 64)

__device__ __forceinline__ double pvs64_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }
__device__ __forceinline__ double pvs64_silu(double v) { return v * pvs64_sigmoid(v); }
// d/dv SiLU(v)
__device__ __forceinline__ double pvs64_silu_grad(double v) {
    const double s = pvs64_sigmoid(v);
    return s * (1.0 + v * (1.0 - s));
}
__device__ __forceinline__ double pvs64_att_act(int act, double l) {
    switch (act) {
        case PVS_ACT_SIGMOID: return pvs64_sigmoid(l);
        case PVS_ACT_TANH: return tanh(l);
        case PVS_ACT_RELU: return l > 0.0 ? l : 0.0;
        case PVS_ACT_SILU: return pvs64_silu(l);
        default: return l;
    }
}
// derivative wrt the logit l, a = act(l)
__device__ __forceinline__ double pvs64_att_act_grad(int act, double l, double a) {
    switch (act) {
        case PVS_ACT_SIGMOID: return a * (1.0 - a);
        case PVS_ACT_TANH: return 1.0 - a * a;
        case PVS_ACT_RELU: return l > 0.0 ? 1.0 : 0.0;
        case PVS_ACT_SILU: return pvs64_silu_grad(l);
        default: return 1.0;
    }
}
