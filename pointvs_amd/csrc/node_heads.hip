// Heads on every node row (pvs_node_heads_fwd): y[n, col + o] = act(b[o] + sum_k h[n, k] W[o, k]) for up to
// PVS_MAX_POOL_HEADS heads, the arithmetic of the pooled heads (head_ops.h) applied per node - the class-activation map
// of a screening step (screening.py: LibraryScreen(cam=...)). Memory bound: a row is read once, 16 bytes per lane and
// load, into an LDS tile; one lane then owns one row of the tile and runs its channel-ascending chains from LDS, the
// weights (wave-uniform) in scalar registers.
#include "common.h"
#include "head_ops.h"
#include "node_heads.h"

namespace {
// U 16-byte loads of one lane, kPvsNodeHeadThreads float4 apart from i0 on, all in flight before the first is written
// to the tile; every one of them lies inside the tile (the caller's count), so nothing here is conditional - behind a
// condition the compiler moves each load next to its write and waits for it there.
template <int U>
__device__ __forceinline__ void stage_loads(const float4* __restrict__ src4, float* tile, int i0, int w4, int stride) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src4[i0 + u * kPvsNodeHeadThreads];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = i0 + u * kPvsNodeHeadThreads, r = i / w4, q = i - r * w4;
        *reinterpret_cast<float4*>(tile + r * stride + 4 * q) = v[u];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kPvsNodeHeadThreads)
k_node_heads_fwd(const float* __restrict__ h, const PvsHeadArgs heads, float* __restrict__ y, int n_rows, int width,
                 int ld_y, int stride, int tile_rows) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const long long r0 = (long long)blockIdx.x * tile_rows;
    const int nr = (int)min((long long)tile_rows, (long long)n_rows - r0);      // (>= 1: the grid ends with the rows)
    const float* __restrict__ src = h + (size_t)r0 * width;                     // the tile's rows are one contiguous range
    if (VEC) {
        const int w4 = width >> 2, n4 = nr * w4;
        const float4* __restrict__ src4 = reinterpret_cast<const float4*>(src);
        // rounds every lane takes part in: 16 loads at a time (a full tile of 128 rows x 64 channels is one such round),
        // then 8, 4, 1; what is left is less than one float4 per lane
        int i = threadIdx.x;
        int rounds = n4 / kPvsNodeHeadThreads;      // (workgroup-uniform)
        for (; rounds >= 16; rounds -= 16, i += 16 * kPvsNodeHeadThreads) stage_loads<16>(src4, tile, i, w4, stride);
        if (rounds >= 8) { stage_loads<8>(src4, tile, i, w4, stride); rounds -= 8; i += 8 * kPvsNodeHeadThreads; }
        if (rounds >= 4) { stage_loads<4>(src4, tile, i, w4, stride); rounds -= 4; i += 4 * kPvsNodeHeadThreads; }
        for (; rounds > 0; --rounds, i += kPvsNodeHeadThreads) stage_loads<1>(src4, tile, i, w4, stride);
        if (i < n4) stage_loads<1>(src4, tile, i, w4, stride);
    } else {
        const int n1 = nr * width;
        for (int i = threadIdx.x; i < n1; i += kPvsNodeHeadThreads) {
            const int r = i / width, k = i - r * width;
            tile[r * stride + k] = src[i];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x >= nr) return;
    const float* pl = tile + threadIdx.x * stride;
    float* yr = y + (size_t)(r0 + threadIdx.x) * ld_y;
#pragma nounroll
    for (int i = 0; i < heads.n; ++i) {      // (one body for all heads: their weights fill the scalar registers)
        const PvsHead hd = heads.head[i];
        if (!VEC) {
            for (int o = 0; o < hd.n_out; ++o) yr[hd.col + o] = head_act(hd.act, head_dot(pl, hd.w, hd.b, o, width));
        } else if (hd.n_out == 1) {
            float acc[1];
            head_dot_x4<1>(pl, hd.w, hd.b, 0, 1, width, acc);
            yr[hd.col] = head_act(hd.act, acc[0]);
        } else {
            for (int o0 = 0; o0 < hd.n_out; o0 += 4) {
                float acc[4];
                head_dot_x4<4>(pl, hd.w, hd.b, o0, hd.n_out, width, acc);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (o0 + j < hd.n_out) yr[hd.col + o0 + j] = head_act(hd.act, acc[j]);
            }
        }
    }
}
}  // namespace

extern "C" int pvs_node_heads_fwd(const float* h, const PvsHead* heads, int32_t n_heads, float* y, int32_t n_rows,
                                  int32_t width, int32_t ld_y, pvs_stream_t stream) {
    PVS_REQUIRE(width >= 1 && width <= kPvsNodeHeadMaxWidth, "node_heads: width %d unsupported (1..%d)", width,
                kPvsNodeHeadMaxWidth);
    PVS_REQUIRE(n_rows >= 0, "node_heads: %d rows", n_rows);
    PvsHeadArgs args;
    PVS_TRY(pvs_head_args("node_heads", heads, n_heads, ld_y, &args));
    if (n_rows == 0) return 0;
    PVS_REQUIRE(h && y, "node_heads: NULL argument");
    // (16-byte loads need rows that start on 16 bytes: a width that is a multiple of four on an aligned base)
    const bool vec = (width & 3) == 0 && ((uintptr_t)h & 15) == 0;
    const int stride = pvs_node_heads_stride(width, vec), tile_rows = pvs_node_heads_tile_rows(stride);
    const unsigned blocks = (unsigned)(((long long)n_rows + tile_rows - 1) / tile_rows);
    const size_t lds = (size_t)tile_rows * stride * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        k_node_heads_fwd<true><<<blocks, kPvsNodeHeadThreads, lds, s>>>(h, args, y, n_rows, width, ld_y, stride, tile_rows);
    else
        k_node_heads_fwd<false><<<blocks, kPvsNodeHeadThreads, lds, s>>>(h, args, y, n_rows, width, ld_y, stride, tile_rows);
    PVS_CHECK_LAUNCH();
    return 0;
}
