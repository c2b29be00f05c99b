// fp64 dense building blocks and the small model-level ops of the --double path: linear, global mean pool and
// unsorted segment sum / mean (include/pvs_egnn.h, the *_f64 entries). Plain VALU fp64; every output element is
// summed by one thread in a fixed order, so results are bitwise reproducible.
#include <hipcub/hipcub.hpp>

#include "f64_ops.h"

// ---- Y = X W^T (+ b) (+ Y) ----
__global__ void __launch_bounds__(256) k64_gemm(double* __restrict__ Y, int ldy, const double* __restrict__ X, int ldx,
                                                const double* __restrict__ W, int wsc, int wsk,
                                                const double* __restrict__ b, int R, int K, int C, int accumulate) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)R * C) return;
    const int r = (int)(idx / C), c = (int)(idx % C);
    const double* x = X + (size_t)r * ldx;
    const double* w = W + (size_t)c * wsc;
    double acc = b ? b[c] : 0.0;
    for (int k = 0; k < K; ++k) acc = fma(x[k], w[(size_t)k * wsk], acc);
    double* y = Y + (size_t)r * ldy + c;
    *y = accumulate ? *y + acc : acc;
}

int pvs64_gemm(hipStream_t s, double* Y, int ldy, const double* X, int ldx, const double* W, int wsc, int wsk,
               const double* b, int R, int K, int C, bool accumulate) {
    const long long total = (long long)R * C;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(k64_gemm, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Y, ldy, X, ldx, W, wsc, wsk,
                       b, R, K, C, accumulate ? 1 : 0);
    PVS_CHECK_LAUNCH();
    return 0;
}

// ---- G = A^T B over rows, by slabs ----
static int atb_slabs(int R) {
    int n = (R + 1023) / 1024;
    return n < 1 ? 1 : (n > 512 ? 512 : n);
}

size_t pvs64_atb_slab_doubles(int R, int C, int K) { return (size_t)atb_slabs(R) * C * K; }

__global__ void __launch_bounds__(256) k64_atb_slab(double* __restrict__ slabs, const double* __restrict__ A, int lda,
                                                    const double* __restrict__ B, int ldb, int R, int C, int K,
                                                    int n_slabs) {
    const int o = blockIdx.y * blockDim.x + threadIdx.x;
    if (o >= C * K) return;
    const int c = o / K, k = o % K;
    const int sl = blockIdx.x;
    const int per = (R + n_slabs - 1) / n_slabs;
    const int r0 = sl * per, r1 = min(R, r0 + per);
    double acc = 0.0;
    if (B) {
        for (int r = r0; r < r1; ++r) acc = fma(A[(size_t)r * lda + c], B[(size_t)r * ldb + k], acc);
    } else {
        for (int r = r0; r < r1; ++r) acc += A[(size_t)r * lda + c];
    }
    slabs[(size_t)sl * C * K + o] = acc;
}

__global__ void __launch_bounds__(256) k64_atb_sum(double* __restrict__ G, int ldg, const double* __restrict__ slabs,
                                                   int C, int K, int n_slabs, int accumulate) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= C * K) return;
    double acc = 0.0;
    for (int sl = 0; sl < n_slabs; ++sl) acc += slabs[(size_t)sl * C * K + o];
    double* g = G + (size_t)(o / K) * ldg + (o % K);
    *g = accumulate ? *g + acc : acc;
}

int pvs64_atb(hipStream_t s, double* G, int ldg, const double* A, int lda, const double* B, int ldb, int R, int C,
              int K, double* slabs, bool accumulate) {
    if (C * K <= 0) return 0;
    const int ns = atb_slabs(R);
    const unsigned nb = (unsigned)((C * K + 255) / 256);
    hipLaunchKernelGGL(k64_atb_slab, dim3(ns, nb), dim3(256), 0, s, slabs, A, lda, B, ldb, R, C, K, ns);
    PVS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k64_atb_sum, dim3(nb), dim3(256), 0, s, G, ldg, slabs, C, K, ns, accumulate ? 1 : 0);
    PVS_CHECK_LAUNCH();
    return 0;
}

// ---- linear ----
extern "C" int pvs_linear_fwd_f64(const double* x, const double* w, const double* b, double* y, int32_t N, int32_t K,
                                  int32_t C, pvs_stream_t stream) {
    PVS_REQUIRE(N >= 0 && K >= 0 && C >= 0, "pvs_linear_fwd_f64: negative size");
    PVS_REQUIRE(N == 0 || C == 0 || (x && w && y) || K == 0, "pvs_linear_fwd_f64: NULL tensor");
    return pvs64_gemm((hipStream_t)stream, y, C, x, K, w, K, 1, b, N, K, C, false);
}

extern "C" size_t pvs_linear_bwd_workspace_bytes_f64(int32_t N, int32_t K, int32_t C) {
    const size_t a = pvs64_atb_slab_doubles(N, C, K), b = pvs64_atb_slab_doubles(N, C, 1);
    return (a > b ? a : b) * sizeof(double) + 256;
}

extern "C" int pvs_linear_bwd_f64(const double* x, const double* w, const double* g_y, double* g_x, double* g_w,
                                  double* g_b, int32_t N, int32_t K, int32_t C, void* workspace,
                                  size_t workspace_bytes, pvs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    PVS_REQUIRE(N >= 0 && K >= 0 && C >= 0, "pvs_linear_bwd_f64: negative size");
    PVS_REQUIRE(workspace_bytes >= pvs_linear_bwd_workspace_bytes_f64(N, K, C), "pvs_linear_bwd_f64: workspace too small");
    double* slabs = (double*)workspace;
    if (g_x) {   // g_x[n, k] = sum_c g_y[n, c] w[c, k]
        int rc = pvs64_gemm(s, g_x, K, g_y, C, w, 1, K, nullptr, N, C, K, false);
        if (rc) return rc;
    }
    if (g_w) {
        int rc = pvs64_atb(s, g_w, K, g_y, C, x, K, N, C, K, slabs, false);
        if (rc) return rc;
    }
    if (g_b) {
        int rc = pvs64_colsum(s, g_b, g_y, C, N, C, slabs);
        if (rc) return rc;
    }
    return 0;
}

// ---- global mean pool over contiguous node ranges ----
__global__ void k64_mean_pool_fwd(const double* __restrict__ h, const int32_t* __restrict__ gptr,
                                  double* __restrict__ pooled, int B, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * W) return;
    const int g = (int)(idx / W), c = (int)(idx % W);
    const int n0 = gptr[g], n1 = gptr[g + 1];
    double acc = 0.0;
    for (int n = n0; n < n1; ++n) acc += h[(size_t)n * W + c];
    const int cnt = n1 - n0;
    pooled[idx] = acc / (double)(cnt > 1 ? cnt : 1);
}

__global__ void k64_mean_pool_bwd(const double* __restrict__ gp, const int32_t* __restrict__ gptr,
                                  double* __restrict__ g_h, int B, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * W) return;
    const int g = (int)(idx / W), c = (int)(idx % W);
    const int n0 = gptr[g], n1 = gptr[g + 1];
    const int cnt = n1 - n0;
    const double v = gp[idx] / (double)(cnt > 1 ? cnt : 1);
    for (int n = n0; n < n1; ++n) g_h[(size_t)n * W + c] = v;
}

extern "C" int pvs_mean_pool_fwd_f64(const double* h, const int32_t* graph_ptr, double* pooled, int32_t n_graphs,
                                     int32_t width, pvs_stream_t stream) {
    PVS_REQUIRE(n_graphs >= 0 && width >= 0, "pvs_mean_pool_fwd_f64: negative size");
    const long long total = (long long)n_graphs * width;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k64_mean_pool_fwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       h, graph_ptr, pooled, n_graphs, width);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_mean_pool_bwd_f64(const double* g_pooled, const int32_t* graph_ptr, double* g_h, int32_t n_graphs,
                                     int32_t n_nodes, int32_t width, pvs_stream_t stream) {
    PVS_REQUIRE(n_graphs >= 0 && width >= 0 && n_nodes >= 0, "pvs_mean_pool_bwd_f64: negative size");
    hipStream_t s = (hipStream_t)stream;
    // nodes outside every graph's range get a zero gradient (as in the fp32 op)
    if ((size_t)n_nodes * width) PVS_CHECK_HIP(hipMemsetAsync(g_h, 0, (size_t)n_nodes * width * sizeof(double), s));
    const long long total = (long long)n_graphs * width;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k64_mean_pool_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g_pooled, graph_ptr,
                       g_h, n_graphs, width);
    PVS_CHECK_LAUNCH();
    return 0;
}

// ---- unsorted segment sum / mean ----
// The rows are ordered by segment with a stable radix sort (row order kept inside a segment), each output element
// sums its segment's rows in that order.
struct Seg64Ws {
    int32_t *keys, *keys_sorted, *iota, *order;
    void* sort_tmp;
    size_t sort_bytes;
};

static size_t seg64_plan(int E, Seg64Ws* w, void* base, size_t* total) {
    size_t sort_bytes = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const int32_t*)nullptr, (int32_t*)nullptr,
                                       (const int32_t*)nullptr, (int32_t*)nullptr, E > 0 ? E : 1, 0, 32, 0);
    PvsArena a(base, (size_t)-1);
    w->keys = a.take<int32_t>(E);
    w->keys_sorted = a.take<int32_t>(E);
    w->iota = a.take<int32_t>(E);
    w->order = a.take<int32_t>(E);
    w->sort_tmp = a.take<char>(sort_bytes);
    w->sort_bytes = sort_bytes;
    *total = a.off + 256;
    return *total;
}

extern "C" size_t pvs_segment_workspace_bytes_f64(int32_t n_rows, int32_t n_segments) {
    (void)n_segments;
    Seg64Ws w;
    size_t total;
    return seg64_plan(n_rows, &w, nullptr, &total);
}

__global__ void k64_seg_keys(const int64_t* __restrict__ ids, int E, int S, int32_t* __restrict__ keys,
                             int32_t* __restrict__ iota, int32_t* __restrict__ status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t v = ids[e];
    int k = (int)v;
    if (v < 0 || v >= S) {
        atomicOr(status, 1);
        k = 0;
    }
    keys[e] = k;
    iota[e] = e;
}

__global__ void k64_seg_ptr(const int32_t* __restrict__ keys_sorted, int E, int S, int32_t* __restrict__ ptr) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    int lo = 0, hi = E;        // first position with key >= s
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys_sorted[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    ptr[s] = lo;
}

__global__ void k64_seg_sum(const double* __restrict__ data, const int32_t* __restrict__ order,
                            const int32_t* __restrict__ ptr, int S, int C, int mean, double* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)S * C) return;
    const int s = (int)(idx / C), c = (int)(idx % C);
    const int p0 = ptr[s], p1 = ptr[s + 1];
    double acc = 0.0;
    for (int p = p0; p < p1; ++p) acc += data[(size_t)order[p] * C + c];
    if (mean) acc /= (double)(p1 - p0 > 1 ? p1 - p0 : 1);
    out[idx] = acc;
}

extern "C" int pvs_segment_reduce_fwd_f64(const double* data, const int64_t* ids, int32_t n_rows, int32_t width,
                                          int32_t n_segments, int32_t mean, double* out, int32_t* ptr_out,
                                          int32_t* status, void* workspace, size_t workspace_bytes,
                                          pvs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const int E = n_rows, C = width, S = n_segments;
    PVS_REQUIRE(E >= 0 && C >= 0 && S >= 0, "pvs_segment_reduce_fwd_f64: negative size");
    PVS_REQUIRE(ptr_out && status, "pvs_segment_reduce_fwd_f64: ptr_out / status are required");
    Seg64Ws w;
    size_t need;
    seg64_plan(E, &w, workspace, &need);
    PVS_REQUIRE(workspace_bytes >= need, "pvs_segment_reduce_fwd_f64: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    PVS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (E == 0) {
        PVS_CHECK_HIP(hipMemsetAsync(ptr_out, 0, (size_t)(S + 1) * sizeof(int32_t), s));
        if ((size_t)S * C) PVS_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)S * C * sizeof(double), s));
        return 0;
    }
    hipLaunchKernelGGL(k64_seg_keys, dim3((E + 255) / 256), dim3(256), 0, s, ids, E, S, w.keys, w.iota, status);
    PVS_CHECK_LAUNCH();
    size_t tb = w.sort_bytes;
    PVS_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.sort_tmp, tb, w.keys, w.keys_sorted, w.iota, w.order, E, 0, 32,
                                                     s));
    hipLaunchKernelGGL(k64_seg_ptr, dim3((S + 1 + 255) / 256), dim3(256), 0, s, w.keys_sorted, E, S, ptr_out);
    PVS_CHECK_LAUNCH();
    const long long total = (long long)S * C;
    if (total) {
        hipLaunchKernelGGL(k64_seg_sum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, data, w.order, ptr_out,
                           S, C, mean, out);
        PVS_CHECK_LAUNCH();
    }
    return 0;
}

__global__ void k64_seg_bwd(const double* __restrict__ g_out, const int64_t* __restrict__ ids,
                            const int32_t* __restrict__ ptr, int E, int C, int S, int mean, double* __restrict__ g) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)E * C) return;
    const int e = (int)(idx / C), c = (int)(idx % C);
    const int64_t v = ids[e];
    const int sid = (v < 0 || v >= S) ? 0 : (int)v;
    double val = g_out[(size_t)sid * C + c];
    if (mean) {
        const int cnt = ptr[sid + 1] - ptr[sid];
        val /= (double)(cnt > 1 ? cnt : 1);
    }
    g[idx] = val;
}

extern "C" int pvs_segment_reduce_bwd_f64(const double* g_out, const int64_t* ids, const int32_t* ptr, int32_t n_rows,
                                          int32_t width, int32_t n_segments, int32_t mean, double* g_data,
                                          pvs_stream_t stream) {
    PVS_REQUIRE(n_rows >= 0 && width >= 0 && n_segments >= 0, "pvs_segment_reduce_bwd_f64: negative size");
    const long long total = (long long)n_rows * width;
    if (total == 0) return 0;
    PVS_REQUIRE(n_segments > 0, "pvs_segment_reduce_bwd_f64: rows but no segments");
    hipLaunchKernelGGL(k64_seg_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_out,
                       ids, ptr, n_rows, width, n_segments, mean, g_data);
    PVS_CHECK_LAUNCH();
    return 0;
}
