// The arithmetic of a head (PvsHead: one nn.Linear followed by nothing, ReLU or a default Softplus), said once for the
// kernels that evaluate heads: on a pooled row (dense_ops.hip: k_pool_head_fwd, k_pool_heads_fwd) and on every node row
// (node_heads.hip: k_node_heads_fwd). The contract: the bias first, then one fmaf per channel, channels ascending.
#pragma once
#include "common.h"

// The head descriptors as kernel arguments (no device table: the launch captures as it stands); the loops over them are
// unrolled so that they stay in scalar registers.
struct PvsHeadArgs {
    PvsHead head[PVS_MAX_POOL_HEADS];
    int n;
};

// `heads` (a HOST array) checked and copied into *args: weights present, a known activation, column ranges inside
// ld_y and disjoint. `who` begins the error text.
inline int pvs_head_args(const char* who, const PvsHead* heads, int n_heads, int ld_y, PvsHeadArgs* args) {
    PVS_REQUIRE(heads && n_heads >= 1 && n_heads <= PVS_MAX_POOL_HEADS, "%s: %d heads (1..%d in one launch)", who,
                n_heads, PVS_MAX_POOL_HEADS);
    *args = PvsHeadArgs{};
    args->n = n_heads;
    for (int i = 0; i < n_heads; ++i) {
        const PvsHead& hd = heads[i];
        PVS_REQUIRE(hd.w && hd.n_out >= 1 && hd.act >= PVS_HEAD_NONE && hd.act <= PVS_HEAD_SOFTPLUS,
                    "%s: head %d: weights missing, n_out %d or activation %d unsupported", who, i, hd.n_out, hd.act);
        PVS_REQUIRE(hd.col >= 0 && hd.col <= ld_y - hd.n_out, "%s: head %d: columns [%d, %d + %d) outside the %d of y",
                    who, i, hd.col, hd.col, hd.n_out, ld_y);
        for (int j = 0; j < i; ++j)
            PVS_REQUIRE(hd.col >= heads[j].col + heads[j].n_out || heads[j].col >= hd.col + hd.n_out,
                        "%s: heads %d and %d write overlapping columns", who, j, i);
        args->head[i] = hd;
    }
    return 0;
}

// b[o] + sum_k W[o, k] pl[k], k ascending (the order of k_linear), one fmaf per term
__device__ __forceinline__ float head_dot(const float* pl, const float* __restrict__ W, const float* __restrict__ b,
                                          int o, int width) {
    float acc = b ? b[o] : 0.f;
    const float* wr = W + (size_t)o * width;
    for (int k = 0; k < width; ++k) acc = fmaf(pl[k], wr[k], acc);
    return acc;
}

// head_dot for the outputs o0 .. o0 + J - 1 of one head at once on a row whose channels are read four at a time
// (width % 4 == 0, pl 16-byte aligned): every output keeps its own chain - bias first, one fmaf per channel, channels
// ascending - so acc[j] is bit for bit head_dot(pl, W, b, o0 + j, width); the J chains share the reads of the row.
// Outputs past n_out repeat the last one (their weights are read, nothing past the matrix) and are the caller's to drop.
template <int J>
__device__ __forceinline__ void head_dot_x4(const float* pl, const float* __restrict__ W, const float* __restrict__ b,
                                            int o0, int n_out, int width, float (&acc)[J]) {
    const float* wr[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int o = min(o0 + j, n_out - 1);
        acc[j] = b ? b[o] : 0.f;
        wr[j] = W + (size_t)o * width;
    }
    for (int k = 0; k < width; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(pl + k);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            acc[j] = fmaf(v.x, wr[j][k], acc[j]);
            acc[j] = fmaf(v.y, wr[j][k + 1], acc[j]);
            acc[j] = fmaf(v.z, wr[j][k + 2], acc[j]);
            acc[j] = fmaf(v.w, wr[j][k + 3], acc[j]);
        }
    }
}

// nn.Softplus() with its defaults (beta 1, threshold 20): the input itself above the threshold
__device__ __forceinline__ float head_act(int act, float v) {
    if (act == PVS_HEAD_RELU) return v > 0.f ? v : 0.f;
    if (act == PVS_HEAD_SOFTPLUS) return v > 20.f ? v : log1pf(expf(v));
    return v;
}
