// One EGNNLayer forward and backward in fp64 (pvs_egnn_layer_*_f64, include/pvs_egnn.h): the --double path.
//
// Design ("fp64 layer"):
//   - node level: the P/Q split of edge_mlp.0 (P = h W_row^T + b, Q = h W_col^T), node_mlp, GraphNorm and the
//     gates as plain fp64 GEMMs / element-wise kernels over N rows (f64_ops.h);
//   - edge level: one wavefront per CSR destination row, one lane per channel (H <= 64). edge_mlp.2 and coord_mlp.0
//     sit in LDS as fp64 (input-major, row stride H + 1: the forward reads them lane-contiguous, the backward's
//     transposed product with a 2-way bank conflict at most). Activations travel between lanes by v_readlane; dot
//     products are xor-butterfly sums (every lane gets the same bits). Row sums stay in lanes: no atomics;
//   - backward: the row kernel recomputes the edge forward, keeps the row-side sums in lanes and writes the per-edge
//     gradients the column side and the weight gradients need; a CSC gather (colptr / cedge) sums the column side;
//     weight gradients are A^T B over edges or nodes in fixed slabs (pvs64_atb).
// Every output is summed in one fixed order: bitwise reproducible from run to run.
#include "f64_ops.h"

namespace {

constexpr int kWaves = 4;      // wavefronts per block
constexpr int kMaxBlocks = 1024;

struct E64Args {
    int N, A, ld1, base1;      // base1: column of edge_mlp.0 that holds the radial weight
    int coords, eatt, softmax, norm, tanh_, eres, rezero, gated, act;
    const int32_t *rowptr, *col;
    const uint8_t* etype;
    const double *x, *P, *Q, *w1, *b2, *W2, *bc1, *Wc1, *wc2, *aw, *ab, *mp, *egate;
    // forward outputs
    double *magg, *x_out, *m_out, *att_out;
    // backward
    const double *att, *g_agg, *g_xout, *g_mout;
    double *gz1, *gd, *g_mp, *a1s, *gz2s, *ms, *gc1s, *gP, *gxrow, *rp;
};

__device__ __forceinline__ double rl64(double v, int k) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), k);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__device__ __forceinline__ double wsum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct EdgeV {
    double z1, a1, z2, m0, mp, m, c1, s1, s, l;
    double d0, d1, d2, r, den;
    int t;
};

// per-lane constants of one layer
struct LaneC {
    double wr, wa0, wa1, wa2, b2, bc1, wc2, aw, ab, gate;
};

// The forward of edge e of row i up to m, s and the attention logit (lane = channel; lanes >= H hold zeros).
template <int H>
__device__ __forceinline__ void eval_edge(const E64Args& a, const double* S2, const double* SC, int e, int lane,
                                          bool on, int cc, double xi0, double xi1, double xi2, double Pi,
                                          const LaneC& k, EdgeV& v) {
    const int j = a.col[e];
    v.t = a.A ? (int)a.etype[e] : 0;
    v.d0 = xi0 - a.x[3 * j + 0];
    v.d1 = xi1 - a.x[3 * j + 1];
    v.d2 = xi2 - a.x[3 * j + 2];
    v.r = v.d0 * v.d0 + v.d1 * v.d1 + v.d2 * v.d2;
    v.den = a.norm ? sqrt(v.r) + 1e-8 : 1.0;
    double z1 = Pi + a.Q[(size_t)j * H + cc] + k.wr * v.r;
    if (a.A) z1 += v.t == 0 ? k.wa0 : (v.t == 1 ? k.wa1 : k.wa2);
    v.z1 = z1;
    v.a1 = on ? pvs64_silu(z1) : 0.0;
    double z2 = k.b2;
#pragma unroll 8
    for (int q = 0; q < H; ++q) z2 = fma(S2[q * (H + 1) + cc], rl64(v.a1, q), z2);
    v.z2 = z2;
    v.m0 = on ? pvs64_silu(z2) : 0.0;
    v.mp = 0.0;
    v.m = v.m0;
    if (a.eres) {
        v.mp = on ? a.mp[(size_t)e * H + cc] : 0.0;
        if (a.rezero) v.m = v.mp + k.gate * v.m0;
        else if (a.gated) v.m = k.gate * v.m0 + (1.0 - k.gate) * v.mp;
        else v.m = v.m0 + v.mp;
    }
    if (a.coords) {
        double c1 = k.bc1;
#pragma unroll 8
        for (int q = 0; q < H; ++q) c1 = fma(SC[q * (H + 1) + cc], rl64(v.m, q), c1);
        v.c1 = c1;
        v.s1 = on ? pvs64_silu(c1) : 0.0;
        const double sp = wsum64(k.wc2 * v.s1);
        v.s = a.tanh_ ? tanh(sp) : sp;
    }
    if (a.eatt) v.l = wsum64(k.aw * v.m) + k.ab;
}

template <int H>
__device__ __forceinline__ void load_weights(const E64Args& a, double* S2, double* SC) {
    for (int idx = threadIdx.x; idx < H * H; idx += blockDim.x) {
        const int o = idx / H, i = idx % H;
        S2[i * (H + 1) + o] = a.W2[idx];
        SC[i * (H + 1) + o] = a.coords ? a.Wc1[idx] : 0.0;
    }
    __syncthreads();
}

template <int H>
__device__ __forceinline__ LaneC lane_consts(const E64Args& a, int cc, bool on) {
    LaneC k;
    const double* w = a.w1 + (size_t)cc * a.ld1 + a.base1;
    k.wr = on ? w[0] : 0.0;
    k.wa0 = (on && a.A > 0) ? w[1] : 0.0;
    k.wa1 = (on && a.A > 1) ? w[2] : 0.0;
    k.wa2 = (on && a.A > 2) ? w[3] : 0.0;
    k.b2 = on ? a.b2[cc] : 0.0;
    k.bc1 = (on && a.coords) ? a.bc1[cc] : 0.0;
    k.wc2 = (on && a.coords) ? a.wc2[cc] : 0.0;
    k.aw = (on && a.eatt) ? a.aw[cc] : 0.0;
    k.ab = a.eatt ? a.ab[0] : 0.0;
    k.gate = 0.0;
    if (a.eres && (a.rezero || a.gated)) {
        const double g = a.egate[0];
        k.gate = a.rezero ? g : (g > 0.0 ? g : 0.0);
    }
    return k;
}

template <int H>
__global__ void __launch_bounds__(256) k64_edge_fwd(E64Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    double* S2 = lds64;
    double* SC = lds64 + H * (H + 1);
    load_weights<H>(a, S2, SC);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < H;
    const int cc = on ? lane : 0;
    const LaneC k = lane_consts<H>(a, cc, on);
    for (int i = blockIdx.x * kWaves + wave; i < a.N; i += gridDim.x * kWaves) {
        const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
        const double xi0 = a.x[3 * i], xi1 = a.x[3 * i + 1], xi2 = a.x[3 * i + 2];
        const double Pi = a.P[(size_t)i * H + cc];
        EdgeV v;
        double mx = -INFINITY, ssum = 0.0;
        if (a.eatt && a.softmax) {      // running max / sum over the row (online softmax)
            for (int e = r0; e < r1; ++e) {
                eval_edge<H>(a, S2, SC, e, lane, on, cc, xi0, xi1, xi2, Pi, k, v);
                if (v.l > mx) {
                    ssum = ssum * exp(mx - v.l) + 1.0;
                    mx = v.l;
                } else {
                    ssum += exp(v.l - mx);
                }
            }
        }
        double agg = 0.0, xs0 = 0.0, xs1 = 0.0, xs2 = 0.0;
        for (int e = r0; e < r1; ++e) {
            eval_edge<H>(a, S2, SC, e, lane, on, cc, xi0, xi1, xi2, Pi, k, v);
            if (a.coords) {
                xs0 += (v.d0 / v.den) * v.s;
                xs1 += (v.d1 / v.den) * v.s;
                xs2 += (v.d2 / v.den) * v.s;
            }
            double att = 1.0;
            if (a.eatt) {
                att = a.softmax ? exp(v.l - mx) / ssum : pvs64_att_act(a.act, v.l);
                if (lane == 0) a.att_out[e] = att;
            }
            agg += att * v.m;
            if (a.m_out && on) a.m_out[(size_t)e * H + lane] = v.m;
        }
        if (on) a.magg[(size_t)i * H + lane] = agg;
        if (lane < 3) {
            const double xv = a.x[3 * i + lane];
            const double xs = lane == 0 ? xs0 : (lane == 1 ? xs1 : xs2);
            const int cnt = r1 - r0 > 1 ? r1 - r0 : 1;
            a.x_out[3 * i + lane] = a.coords ? xv + xs / (double)cnt : xv;
        }
    }
}

template <int H>
__global__ void __launch_bounds__(256) k64_edge_bwd(E64Args a) {
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    double* S2 = lds64;
    double* SC = lds64 + H * (H + 1);
    load_weights<H>(a, S2, SC);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < H;
    const int cc = on ? lane : 0;
    const LaneC k = lane_consts<H>(a, cc, on);
    const int KP = 6 * H + 2;
    const bool coord_live = a.coords && a.g_xout;
    for (int i = blockIdx.x * kWaves + wave; i < a.N; i += gridDim.x * kWaves) {
        const int r0 = a.rowptr[i], r1 = a.rowptr[i + 1];
        const double xi0 = a.x[3 * i], xi1 = a.x[3 * i + 1], xi2 = a.x[3 * i + 2];
        const double Pi = a.P[(size_t)i * H + cc];
        const double gagg = on ? a.g_agg[(size_t)i * H + cc] : 0.0;
        const int cnt = r1 - r0 > 1 ? r1 - r0 : 1;
        double gx0 = 0.0, gx1 = 0.0, gx2 = 0.0;
        if (coord_live) {
            gx0 = a.g_xout[3 * i] / (double)cnt;
            gx1 = a.g_xout[3 * i + 1] / (double)cnt;
            gx2 = a.g_xout[3 * i + 2] / (double)cnt;
        }
        EdgeV v;
        double dsum = 0.0;      // softmax: sum_e att_e * dL/datt_e over the row
        if (a.eatt && a.softmax) {
            for (int e = r0; e < r1; ++e) {
                eval_edge<H>(a, S2, SC, e, lane, on, cc, xi0, xi1, xi2, Pi, k, v);
                dsum += a.att[e] * wsum64(gagg * v.m);
            }
        }
        double accP = 0.0, acc_wc2 = 0.0, acc_aw = 0.0, acc_wr = 0.0, acc_wa0 = 0.0, acc_wa1 = 0.0, acc_wa2 = 0.0;
        double acc_ab = 0.0, acc_eg = 0.0, gxr0 = 0.0, gxr1 = 0.0, gxr2 = 0.0;
        for (int e = r0; e < r1; ++e) {
            eval_edge<H>(a, S2, SC, e, lane, on, cc, xi0, xi1, xi2, Pi, k, v);
            double gm = a.g_mout && on ? a.g_mout[(size_t)e * H + cc] : 0.0;
            if (a.eatt) {
                const double att = a.softmax ? a.att[e] : pvs64_att_act(a.act, v.l);
                gm += att * gagg;
                const double ga = wsum64(gagg * v.m);
                const double gl = a.softmax ? att * (ga - dsum) : ga * pvs64_att_act_grad(a.act, v.l, att);
                acc_aw += gl * v.m;
                acc_ab += gl;
                gm += gl * k.aw;
            } else {
                gm += gagg;
            }
            double gdc0 = 0.0, gdc1 = 0.0, gdc2 = 0.0;
            if (coord_live) {
                const double dn0 = v.d0 / v.den, dn1 = v.d1 / v.den, dn2 = v.d2 / v.den;
                const double gs = gx0 * dn0 + gx1 * dn1 + gx2 * dn2;
                const double gsp = a.tanh_ ? gs * (1.0 - v.s * v.s) : gs;
                acc_wc2 += gsp * v.s1;
                const double gc1 = on ? gsp * k.wc2 * pvs64_silu_grad(v.c1) : 0.0;
                double t = 0.0;
#pragma unroll 8
                for (int q = 0; q < H; ++q) t = fma(SC[cc * (H + 1) + q], rl64(gc1, q), t);
                if (on) {
                    gm += t;
                    a.ms[(size_t)e * H + lane] = v.m;
                    a.gc1s[(size_t)e * H + lane] = gc1;
                }
                gdc0 = gx0 * v.s / v.den;
                gdc1 = gx1 * v.s / v.den;
                gdc2 = gx2 * v.s / v.den;
            }
            if (!on) gm = 0.0;
            double gm0 = gm;
            if (a.eres) {
                double gmp = gm;
                if (a.rezero) {
                    gm0 = gm * k.gate;
                    acc_eg += wsum64(gm * v.m0);
                } else if (a.gated) {
                    gm0 = gm * k.gate;
                    gmp = gm * (1.0 - k.gate);
                    if (a.egate[0] > 0.0) acc_eg += wsum64(gm * (v.m0 - v.mp));
                }
                if (on) a.g_mp[(size_t)e * H + lane] = gmp;
            }
            const double gz2 = on ? gm0 * pvs64_silu_grad(v.z2) : 0.0;
            if (on) {
                a.a1s[(size_t)e * H + lane] = v.a1;
                a.gz2s[(size_t)e * H + lane] = gz2;
            }
            double ga1 = 0.0;
#pragma unroll 8
            for (int q = 0; q < H; ++q) ga1 = fma(S2[cc * (H + 1) + q], rl64(gz2, q), ga1);
            const double gz1 = on ? ga1 * pvs64_silu_grad(v.z1) : 0.0;
            if (on) a.gz1[(size_t)e * H + lane] = gz1;
            accP += gz1;
            acc_wr += gz1 * v.r;
            if (a.A) {
                if (v.t == 0) acc_wa0 += gz1;
                else if (v.t == 1) acc_wa1 += gz1;
                else acc_wa2 += gz1;
            }
            const double gr = wsum64(gz1 * k.wr);
            const double gd0 = 2.0 * v.d0 * gr + gdc0, gd1 = 2.0 * v.d1 * gr + gdc1, gd2 = 2.0 * v.d2 * gr + gdc2;
            if (lane < 3) a.gd[3 * (size_t)e + lane] = lane == 0 ? gd0 : (lane == 1 ? gd1 : gd2);
            gxr0 += gd0;
            gxr1 += gd1;
            gxr2 += gd2;
        }
        double* rp = a.rp + (size_t)i * KP;
        if (on) {
            a.gP[(size_t)i * H + lane] = accP;
            rp[lane] = acc_wc2;
            rp[H + lane] = acc_aw;
            rp[2 * H + lane] = acc_wr;
            rp[3 * H + lane] = acc_wa0;
            rp[4 * H + lane] = acc_wa1;
            rp[5 * H + lane] = acc_wa2;
        }
        if (lane == 0) {
            rp[6 * H] = acc_ab;
            rp[6 * H + 1] = acc_eg;
        }
        if (lane < 3) a.gxrow[3 * i + lane] = lane == 0 ? gxr0 : (lane == 1 ? gxr1 : gxr2);
    }
}

// Column side of the backward: gQ[j] = sum over the edges with col j of gz1 (CSC order); g_x[j] = g_x_out[j] + the
// row-side sum - the column-side sum of the per-edge coordinate gradients.
__global__ void k64_col_gather(const int32_t* __restrict__ colptr, const int32_t* __restrict__ cedge, int N, int H,
                               const double* __restrict__ gz1, const double* __restrict__ gd,
                               const double* __restrict__ gxrow, const double* __restrict__ g_xout,
                               double* __restrict__ gQ, double* __restrict__ g_x) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = H + 3;
    if (idx >= (long long)N * W) return;
    const int j = (int)(idx / W), q = (int)(idx % W);
    const int p0 = colptr[j], p1 = colptr[j + 1];
    if (q < H) {
        double acc = 0.0;
        for (int p = p0; p < p1; ++p) acc += gz1[(size_t)cedge[p] * H + q];
        gQ[(size_t)j * H + q] = acc;
    } else if (g_x) {
        const int d = q - H;
        double acc = 0.0;
        for (int p = p0; p < p1; ++p) acc += gd[3 * (size_t)cedge[p] + d];
        g_x[3 * j + d] = (g_xout ? g_xout[3 * j + d] : 0.0) + gxrow[3 * j + d] - acc;
    }
}

// ---- node level ----
__global__ void k64_silu_fwd(const double* __restrict__ u, double* __restrict__ a, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = pvs64_silu(u[i]);
}

__global__ void k64_silu_bwd(const double* __restrict__ u, const double* __restrict__ g_a, double* __restrict__ g_u,
                             long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g_u[i] = g_a[i] * pvs64_silu_grad(u[i]);
}

// mu[c] = su[c] / N
__global__ void k64_scale_vec(const double* __restrict__ src, double* __restrict__ dst, int n, double div) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] / div;
}

// o = u - mu * ms, o2 = o * o
__global__ void k64_gn_center(const double* __restrict__ u, const double* __restrict__ mu,
                              const double* __restrict__ ms, double* __restrict__ o, double* __restrict__ o2, int N,
                              int H) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * H) return;
    const int c = (int)(i % H);
    const double v = u[i] - mu[c] * ms[c];
    o[i] = v;
    o2[i] = v * v;
}

// sq[c] = sqrt(so2[c] / N + eps)
__global__ void k64_gn_sq(const double* __restrict__ so2, double* __restrict__ sq, int H, double n) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < H) sq[c] = sqrt(so2[c] / n + 1e-5);
}

// a = SiLU(gw * o / sq + gb)
__global__ void k64_gn_apply(const double* __restrict__ o, const double* __restrict__ sq,
                             const double* __restrict__ gw, const double* __restrict__ gb, double* __restrict__ a,
                             int N, int H) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * H) return;
    const int c = (int)(i % H);
    a[i] = pvs64_silu(gw[c] * o[i] / sq[c] + gb[c]);
}

// gv = g_a * SiLU'(v), t1 = gv * o / sq, t2 = gv * gw * o
__global__ void k64_gn_bwd1(const double* __restrict__ u, const double* __restrict__ mu,
                            const double* __restrict__ ms, const double* __restrict__ sq,
                            const double* __restrict__ gw, const double* __restrict__ gb,
                            const double* __restrict__ g_a, double* __restrict__ gv, double* __restrict__ t1,
                            double* __restrict__ t2, int N, int H) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * H) return;
    const int c = (int)(i % H);
    const double o = u[i] - mu[c] * ms[c];
    const double v = gw[c] * o / sq[c] + gb[c];
    const double g = g_a[i] * pvs64_silu_grad(v);
    gv[i] = g;
    t1[i] = g * o / sq[c];
    t2[i] = g * gw[c] * o;
}

// g_o = gv * gw / sq + 2 o g_var / N, g_var = -st2 / (2 sq^3)
__global__ void k64_gn_bwd2(const double* __restrict__ u, const double* __restrict__ mu,
                            const double* __restrict__ ms, const double* __restrict__ sq,
                            const double* __restrict__ gw, const double* __restrict__ gv,
                            const double* __restrict__ st2, double* __restrict__ g_o, int N, int H) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * H) return;
    const int c = (int)(i % H);
    const double o = u[i] - mu[c] * ms[c];
    const double s = sq[c];
    const double g_var = -st2[c] / (2.0 * s * s * s);
    g_o[i] = gv[i] * gw[c] / s + 2.0 * o * g_var / (double)N;
}

// g_u = g_o - ms * s3 / N
__global__ void k64_gn_bwd3(const double* __restrict__ g_o, const double* __restrict__ ms,
                            const double* __restrict__ s3, double* __restrict__ g_u, int N, int H) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * H) return;
    const int c = (int)(i % H);
    g_u[i] = g_o[i] - ms[c] * s3[c] / (double)N;
}

// g_ms = -mu * s3
__global__ void k64_gn_gms(const double* __restrict__ mu, const double* __restrict__ s3, double* __restrict__ g_ms,
                           int H) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < H) g_ms[c] = -mu[c] * s3[c];
}

struct NodeArgs {
    int N, H, natt, act, residual, rezero, gated;
    const double *h, *out, *naw, *nab, *ngate;
    double *nl, *node_att_out, *h_out;
    const double* g_hout;
    double *g_out, *g_h, *np;      // np [N, H + 2]: g_nl * out, g_nl, gate term
};

// h_out from out = node_mlp(...): node attention, then the residual variant
__global__ void k64_node_tail_fwd(NodeArgs a) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const int H = a.H;
    const double* out = a.out + (size_t)n * H;
    const double* h = a.h + (size_t)n * H;
    double na = 1.0;
    if (a.natt) {
        double l = a.nab[0];
        for (int c = 0; c < H; ++c) l = fma(a.naw[c], out[c], l);
        a.nl[n] = l;
        na = pvs64_att_act(a.act, l);
        if (a.node_att_out) a.node_att_out[n] = na;
    }
    double gate = 0.0;
    if (a.residual && (a.rezero || a.gated)) gate = a.rezero ? a.ngate[0] : (a.ngate[0] > 0.0 ? a.ngate[0] : 0.0);
    for (int c = 0; c < H; ++c) {
        const double o2 = out[c] * na;
        double r;
        if (!a.residual) r = o2;
        else if (a.rezero) r = h[c] + gate * o2;
        else if (a.gated) r = gate * o2 + (1.0 - gate) * h[c];
        else r = h[c] + o2;
        a.h_out[(size_t)n * H + c] = r;
    }
}

__global__ void k64_node_tail_bwd(NodeArgs a) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const int H = a.H;
    const double* out = a.out + (size_t)n * H;
    const double* h = a.h + (size_t)n * H;
    const double* gh = a.g_hout + (size_t)n * H;
    double* np = a.np + (size_t)n * (H + 2);
    double na = 1.0, l = 0.0;
    if (a.natt) {
        l = a.nl[n];
        na = pvs64_att_act(a.act, l);
    }
    double gate = 1.0, hgate = 1.0, gterm = 0.0;
    if (!a.residual) hgate = 0.0;
    else if (a.rezero) {
        gate = a.ngate[0];
        for (int c = 0; c < H; ++c) gterm += gh[c] * (out[c] * na);
    } else if (a.gated) {
        const double g = a.ngate[0];
        gate = g > 0.0 ? g : 0.0;
        hgate = 1.0 - gate;
        if (g > 0.0)
            for (int c = 0; c < H; ++c) gterm += gh[c] * (out[c] * na - h[c]);
    }
    double gnatt = 0.0;
    for (int c = 0; c < H; ++c) gnatt += gh[c] * gate * out[c];
    const double gl = a.natt ? gnatt * pvs64_att_act_grad(a.act, l, na) : 0.0;
    for (int c = 0; c < H; ++c) {
        const double go2 = gh[c] * gate;
        a.g_out[(size_t)n * H + c] = go2 * na + (a.natt ? gl * a.naw[c] : 0.0);
        a.g_h[(size_t)n * H + c] = gh[c] * hgate;
        np[c] = gl * out[c];
    }
    np[H] = gl;
    np[H + 1] = gterm;
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

int edge_blocks(int N) {
    int b = (N + kWaves - 1) / kWaves;
    return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}

template <int H>
int launch_edge(hipStream_t s, bool backward, const E64Args& a) {
    const size_t lds = 2 * (size_t)H * (H + 1) * sizeof(double);
    auto kernel = backward ? k64_edge_bwd<H> : k64_edge_fwd<H>;
    PVS_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(edge_blocks(a.N)), dim3(256), lds, s, a);
    PVS_CHECK_LAUNCH();
    return 0;
}

int launch_edge_any(int H, hipStream_t s, bool backward, const E64Args& a) {
    switch (H) {
        case 16: return launch_edge<16>(s, backward, a);
        case 32: return launch_edge<32>(s, backward, a);
        default: return launch_edge<64>(s, backward, a);
    }
}

// Workspace of one call (the same walk sizes it and hands it out).
struct Ws64 {
    double *P, *Q, *o, *o2, *vec0, *vec1, *vec2, *vec3, *slabs;
    // backward only
    double *g_out, *g_a, *t1, *t2, *g_o, *g_u, *g_agg, *gP, *gQ, *gxrow, *np, *rp;
    double *gz1, *gd, *a1s, *gz2s, *ms, *gc1s;
};

size_t plan_ws(int H, int N, int E, bool backward, void* base, Ws64* w) {
    PvsArena a(base, (size_t)-1);
    const size_t NH = (size_t)N * H, EH = (size_t)E * H;
    w->P = a.take<double>(NH);
    w->Q = a.take<double>(NH);
    w->vec0 = a.take<double>(H);
    w->vec1 = a.take<double>(H);
    w->vec2 = a.take<double>(H);
    w->vec3 = a.take<double>(H);
    const int rmax = N > E ? N : E;
    w->slabs = a.take<double>(pvs64_atb_slab_doubles(rmax, H, H));
    if (!backward) {
        w->o = a.take<double>(NH);
        w->o2 = a.take<double>(NH);
        return a.off + 256;
    }
    w->o = w->o2 = nullptr;
    w->g_out = a.take<double>(NH);
    w->g_a = a.take<double>(NH);
    w->t1 = a.take<double>(NH);
    w->t2 = a.take<double>(NH);
    w->g_o = a.take<double>(NH);
    w->g_u = a.take<double>(NH);
    w->g_agg = a.take<double>(NH);
    w->gP = a.take<double>(NH);
    w->gQ = a.take<double>(NH);
    w->gxrow = a.take<double>((size_t)N * 3);
    w->np = a.take<double>((size_t)N * (H + 2));
    w->rp = a.take<double>((size_t)N * (6 * H + 2));
    w->gz1 = a.take<double>(EH);
    w->gd = a.take<double>((size_t)E * 3);
    w->a1s = a.take<double>(EH);
    w->gz2s = a.take<double>(EH);
    w->ms = a.take<double>(EH);
    w->gc1s = a.take<double>(EH);
    return a.off + 256;
}

// saved: agg [N,H] | u [N,H] | a [N,H] | out [N,H] | nl [N] | mu [H] | sq [H]
struct Saved64 {
    double *agg, *u, *a, *out, *nl, *mu, *sq;
};
Saved64 saved_layout(double* base, int N, int H) {
    Saved64 s;
    const size_t NH = (size_t)N * H;
    s.agg = base;
    s.u = base + NH;
    s.a = base + 2 * NH;
    s.out = base + 3 * NH;
    s.nl = base + 4 * NH;
    s.mu = s.nl + N;
    s.sq = s.mu + H;
    return s;
}

int check_desc(const PvsLayerDesc* d, const PvsGraph* g, const char* who) {
    PVS_REQUIRE(d && g, "%s: NULL descriptor or graph", who);
    PVS_REQUIRE(d->hidden == 16 || d->hidden == 32 || d->hidden == 64,
                "%s: hidden=%d is not built in fp64 (16, 32, 64; the caller pads other widths up to 64)", who,
                d->hidden);
    PVS_REQUIRE(d->n_edge_attr >= 0 && d->n_edge_attr <= 3, "%s: n_edge_attr=%d (0..3 built)", who, d->n_edge_attr);
    PVS_REQUIRE(g->n_nodes > 0 && g->n_edges >= 0, "%s: graph with %d nodes / %d edges", who, g->n_nodes, g->n_edges);
    PVS_REQUIRE(!g->n_edges_dev, "%s: a graph with a device-side edge count is forward-only fp32", who);
    PVS_REQUIRE(!(d->flags & PVS_GRAPHNORM_SEGMENTS), "%s: PVS_GRAPHNORM_SEGMENTS (GraphNorm per node segment) is fp32 only", who);
    PVS_REQUIRE(!g->n_norm_rows_dev, "%s: a graph with a device-side GraphNorm row count (n_norm_rows_dev) is fp32 only",
                who);
    PVS_REQUIRE(g->rowptr && (g->n_edges == 0 || g->col), "%s: graph without CSR arrays", who);
    PVS_REQUIRE(d->n_edge_attr == 0 || g->n_edges == 0 || g->etype, "%s: edge classes without etype", who);
    PVS_REQUIRE(!((d->flags & PVS_GATED_RESIDUAL) && (d->flags & PVS_REZERO)), "%s: gated_residual with rezero", who);
    return 0;
}

E64Args edge_args(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParamsF64* p, const double* x,
                  const double* m_prev, const double* P, const double* Q) {
    E64Args a = {};
    const int H = d->hidden;
    const uint32_t f = d->flags;
    a.N = g->n_nodes;
    a.A = d->n_edge_attr;
    a.base1 = (f & PVS_PERM_INVARIANT) ? H : 2 * H;
    a.ld1 = a.base1 + 1 + a.A;
    a.coords = (f & PVS_UPDATE_COORDS) ? 1 : 0;
    a.eatt = (f & PVS_EDGE_ATTENTION) ? 1 : 0;
    a.softmax = (f & PVS_SOFTMAX_ATT) ? 1 : 0;
    a.norm = (f & PVS_NORMALIZE) ? 1 : 0;
    a.tanh_ = (f & PVS_TANH) ? 1 : 0;
    a.eres = ((f & PVS_EDGE_RESIDUAL) && m_prev) ? 1 : 0;
    a.rezero = (f & PVS_REZERO) ? 1 : 0;
    a.gated = (f & PVS_GATED_RESIDUAL) ? 1 : 0;
    a.act = d->att_act;
    a.rowptr = g->rowptr;
    a.col = g->col;
    a.etype = g->etype;
    a.x = x;
    a.P = P;
    a.Q = Q;
    a.w1 = p->edge_w1;
    a.b2 = p->edge_b2;
    a.W2 = p->edge_w2;
    a.bc1 = p->coord_b1;
    a.Wc1 = p->coord_w1;
    a.wc2 = p->coord_w2;
    a.aw = p->att_w;
    a.ab = p->att_b;
    a.mp = m_prev;
    a.egate = p->edge_gate;
    return a;
}

// the node tail's arguments both directions share; the caller adds its outputs (forward) or gradients (backward)
NodeArgs node_args(const PvsLayerDesc* d, const PvsLayerParamsF64* p, int N, const double* h, const Saved64& sv) {
    NodeArgs na = {};
    const uint32_t f = d->flags;
    na.N = N;
    na.H = d->hidden;
    na.natt = (f & PVS_NODE_ATTENTION) ? 1 : 0;
    na.act = d->att_act;
    na.residual = (f & PVS_RESIDUAL) ? 1 : 0;
    na.rezero = (f & PVS_REZERO) ? 1 : 0;
    na.gated = (f & PVS_GATED_RESIDUAL) ? 1 : 0;
    na.h = h;
    na.out = sv.out;
    na.naw = p->node_att_w;
    na.nab = p->node_att_b;
    na.ngate = p->node_gate;
    na.nl = sv.nl;
    return na;
}

int check_params(const PvsLayerDesc* d, const PvsLayerParamsF64* p, const char* who) {
    const uint32_t f = d->flags;
    PVS_REQUIRE(p && p->edge_w1 && p->edge_b1 && p->edge_w2 && p->edge_b2 && p->node_w1 && p->node_b1 &&
                    p->node_w2 && p->node_b2,
                "%s: missing edge_mlp / node_mlp parameters", who);
    PVS_REQUIRE(!(f & PVS_UPDATE_COORDS) || (p->coord_w1 && p->coord_b1 && p->coord_w2), "%s: missing coord_mlp",
                who);
    PVS_REQUIRE(!(f & PVS_EDGE_ATTENTION) || (p->att_w && p->att_b), "%s: missing att_mlp", who);
    PVS_REQUIRE(!(f & PVS_NODE_ATTENTION) || (p->node_att_w && p->node_att_b), "%s: missing node_att_mlp", who);
    PVS_REQUIRE(!(f & PVS_GRAPHNORM) || (p->gn_weight && p->gn_bias && p->gn_mean_scale), "%s: missing GraphNorm",
                who);
    return 0;
}

// P = h W_row^T + b1, Q = h W_col^T (permutation invariance: the same block)
int node_pre(hipStream_t s, const PvsLayerDesc* d, const PvsLayerParamsF64* p, const double* h, int N, double* P,
             double* Q) {
    const int H = d->hidden;
    const bool perm = d->flags & PVS_PERM_INVARIANT;
    const int ld1 = (perm ? H : 2 * H) + 1 + d->n_edge_attr;
    int rc = pvs64_gemm(s, P, H, h, H, p->edge_w1, ld1, 1, p->edge_b1, N, H, H, false);
    if (rc) return rc;
    return pvs64_gemm(s, Q, H, h, H, p->edge_w1 + (perm ? 0 : H), ld1, 1, nullptr, N, H, H, false);
}

}  // namespace

extern "C" size_t pvs_egnn_layer_saved_doubles_f64(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges) {
    (void)n_edges;
    if (!desc) return 0;
    const size_t H = desc->hidden, N = n_nodes > 0 ? n_nodes : 0;
    return 4 * N * H + N + 2 * H;
}

extern "C" size_t pvs_egnn_layer_workspace_bytes_f64(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges,
                                                     int32_t backward) {
    if (!desc) return 0;
    Ws64 w;
    return plan_ws(desc->hidden, n_nodes > 0 ? n_nodes : 0, n_edges > 0 ? n_edges : 0, backward != 0, nullptr, &w);
}

extern "C" int pvs_egnn_layer_fwd_f64(const PvsLayerDesc* desc, const PvsGraph* graph,
                                      const PvsLayerParamsF64* params, const double* h, const double* x,
                                      const double* m_prev, double* h_out, double* x_out, double* m_out,
                                      double* att_out, double* node_att_out, double* saved, void* workspace,
                                      size_t workspace_bytes, pvs_stream_t stream) {
    const char* who = "pvs_egnn_layer_fwd_f64";
    if (int rc = check_desc(desc, graph, who)) return rc;
    if (int rc = check_params(desc, params, who)) return rc;
    PVS_REQUIRE(h && x && h_out && x_out && saved, "%s: NULL tensor", who);
    PVS_REQUIRE(!(desc->flags & PVS_EDGE_ATTENTION) || att_out, "%s: att_out is required with edge attention", who);
    const int H = desc->hidden, N = graph->n_nodes, E = graph->n_edges;
    const uint32_t f = desc->flags;
    Ws64 w;
    const size_t need = plan_ws(H, N, E, false, workspace, &w);
    PVS_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes,
                need);
    hipStream_t s = (hipStream_t)stream;
    Saved64 sv = saved_layout(saved, N, H);
    int rc = node_pre(s, desc, params, h, N, w.P, w.Q);
    if (rc) return rc;
    E64Args a = edge_args(desc, graph, params, x, m_prev, w.P, w.Q);
    a.magg = sv.agg;
    a.x_out = x_out;
    a.m_out = E ? m_out : nullptr;
    a.att_out = att_out;
    if ((rc = launch_edge_any(H, s, false, a))) return rc;
    // node_mlp.0 on [h, agg]
    if ((rc = pvs64_gemm(s, sv.u, H, h, H, params->node_w1, 2 * H, 1, params->node_b1, N, H, H, false))) return rc;
    if ((rc = pvs64_gemm(s, sv.u, H, sv.agg, H, params->node_w1 + H, 2 * H, 1, nullptr, N, H, H, true))) return rc;
    const long long NH = (long long)N * H;
    if (f & PVS_GRAPHNORM) {
        if ((rc = pvs64_colsum(s, w.vec0, sv.u, H, N, H, w.slabs))) return rc;
        hipLaunchKernelGGL(k64_scale_vec, dim3(1), dim3(64), 0, s, w.vec0, sv.mu, H, (double)N);
        PVS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k64_gn_center, dim3(blocks_for(NH)), dim3(256), 0, s, sv.u, sv.mu, params->gn_mean_scale,
                           w.o, w.o2, N, H);
        PVS_CHECK_LAUNCH();
        if ((rc = pvs64_colsum(s, w.vec1, w.o2, H, N, H, w.slabs))) return rc;
        hipLaunchKernelGGL(k64_gn_sq, dim3(1), dim3(64), 0, s, w.vec1, sv.sq, H, (double)N);
        PVS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k64_gn_apply, dim3(blocks_for(NH)), dim3(256), 0, s, w.o, sv.sq, params->gn_weight,
                           params->gn_bias, sv.a, N, H);
        PVS_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(k64_silu_fwd, dim3(blocks_for(NH)), dim3(256), 0, s, sv.u, sv.a, NH);
        PVS_CHECK_LAUNCH();
    }
    if ((rc = pvs64_gemm(s, sv.out, H, sv.a, H, params->node_w2, H, 1, params->node_b2, N, H, H, false))) return rc;
    NodeArgs na = node_args(desc, params, N, h, sv);
    na.node_att_out = node_att_out;
    na.h_out = h_out;
    PVS_REQUIRE(!(na.residual && (na.rezero || na.gated)) || na.ngate, "%s: missing node_gate_parameter", who);
    PVS_REQUIRE(!a.eres || !(a.rezero || a.gated) || a.egate, "%s: missing edge_gate_parameter", who);
    hipLaunchKernelGGL(k64_node_tail_fwd, dim3(blocks_for(N)), dim3(256), 0, s, na);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_egnn_layer_bwd_f64(const PvsLayerDesc* desc, const PvsGraph* graph,
                                      const PvsLayerParamsF64* params, const double* h, const double* x,
                                      const double* m_prev, const double* att, const double* saved,
                                      const double* g_h_out, const double* g_x_out, const double* g_m_out,
                                      double* g_h, double* g_x, double* g_m_prev, const PvsLayerGradsF64* grads,
                                      void* workspace, size_t workspace_bytes, pvs_stream_t stream) {
    const char* who = "pvs_egnn_layer_bwd_f64";
    if (int rc = check_desc(desc, graph, who)) return rc;
    if (int rc = check_params(desc, params, who)) return rc;
    PVS_REQUIRE(h && x && saved && g_h_out && g_h && grads, "%s: NULL tensor", who);
    PVS_REQUIRE(graph->n_edges == 0 || (graph->colptr && graph->cedge),
                "%s: the backward needs the by-column lists (colptr / cedge)", who);
    const uint32_t f = desc->flags;
    const int H = desc->hidden, N = graph->n_nodes, E = graph->n_edges;
    const bool eres = (f & PVS_EDGE_RESIDUAL) && m_prev;
    PVS_REQUIRE(!eres || g_m_prev, "%s: g_m_prev is required when the edge residual applies", who);
    PVS_REQUIRE(!(f & PVS_EDGE_ATTENTION) || att || E == 0, "%s: att is required with edge attention", who);
    Ws64 w;
    const size_t need = plan_ws(H, N, E, true, workspace, &w);
    PVS_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes,
                need);
    hipStream_t s = (hipStream_t)stream;
    Saved64 sv = saved_layout(const_cast<double*>(saved), N, H);
    const long long NH = (long long)N * H;
    int rc;

    // node tail: residual and node attention
    NodeArgs na = node_args(desc, params, N, h, sv);
    na.g_hout = g_h_out;
    na.g_out = w.g_out;
    na.g_h = g_h;
    na.np = w.np;
    PVS_REQUIRE(!(na.residual && (na.rezero || na.gated)) || na.ngate, "%s: missing node_gate_parameter", who);
    hipLaunchKernelGGL(k64_node_tail_bwd, dim3(blocks_for(N)), dim3(256), 0, s, na);
    PVS_CHECK_LAUNCH();
    if (na.natt && grads->node_att_w)
        if ((rc = pvs64_colsum(s, grads->node_att_w, w.np, H + 2, N, H, w.slabs))) return rc;
    if (na.natt && grads->node_att_b)
        if ((rc = pvs64_colsum(s, grads->node_att_b, w.np + H, H + 2, N, 1, w.slabs))) return rc;
    if (na.residual && (na.rezero || na.gated) && grads->node_gate)
        if ((rc = pvs64_colsum(s, grads->node_gate, w.np + H + 1, H + 2, N, 1, w.slabs))) return rc;

    // node_mlp.3
    if (grads->node_w2 && (rc = pvs64_atb(s, grads->node_w2, H, w.g_out, H, sv.a, H, N, H, H, w.slabs, false)))
        return rc;
    if (grads->node_b2 && (rc = pvs64_colsum(s, grads->node_b2, w.g_out, H, N, H, w.slabs))) return rc;
    if ((rc = pvs64_gemm(s, w.g_a, H, w.g_out, H, params->node_w2, 1, H, nullptr, N, H, H, false))) return rc;

    // SiLU and GraphNorm
    if (f & PVS_GRAPHNORM) {
        hipLaunchKernelGGL(k64_gn_bwd1, dim3(blocks_for(NH)), dim3(256), 0, s, sv.u, sv.mu, params->gn_mean_scale,
                           sv.sq, params->gn_weight, params->gn_bias, w.g_a, w.g_o, w.t1, w.t2, N, H);
        PVS_CHECK_LAUNCH();
        if (grads->gn_bias && (rc = pvs64_colsum(s, grads->gn_bias, w.g_o, H, N, H, w.slabs))) return rc;
        if (grads->gn_weight && (rc = pvs64_colsum(s, grads->gn_weight, w.t1, H, N, H, w.slabs))) return rc;
        if ((rc = pvs64_colsum(s, w.vec0, w.t2, H, N, H, w.slabs))) return rc;
        // g_o (into t1, free now)
        hipLaunchKernelGGL(k64_gn_bwd2, dim3(blocks_for(NH)), dim3(256), 0, s, sv.u, sv.mu, params->gn_mean_scale,
                           sv.sq, params->gn_weight, w.g_o, w.vec0, w.t1, N, H);
        PVS_CHECK_LAUNCH();
        if ((rc = pvs64_colsum(s, w.vec1, w.t1, H, N, H, w.slabs))) return rc;
        hipLaunchKernelGGL(k64_gn_bwd3, dim3(blocks_for(NH)), dim3(256), 0, s, w.t1, params->gn_mean_scale, w.vec1,
                           w.g_u, N, H);
        PVS_CHECK_LAUNCH();
        if (grads->gn_mean_scale) {
            hipLaunchKernelGGL(k64_gn_gms, dim3(1), dim3(64), 0, s, sv.mu, w.vec1, grads->gn_mean_scale, H);
            PVS_CHECK_LAUNCH();
        }
    } else {
        hipLaunchKernelGGL(k64_silu_bwd, dim3(blocks_for(NH)), dim3(256), 0, s, sv.u, w.g_a, w.g_u, NH);
        PVS_CHECK_LAUNCH();
    }

    // node_mlp.0 on [h, agg]
    if (grads->node_w1) {
        if ((rc = pvs64_atb(s, grads->node_w1, 2 * H, w.g_u, H, h, H, N, H, H, w.slabs, false))) return rc;
        if ((rc = pvs64_atb(s, grads->node_w1 + H, 2 * H, w.g_u, H, sv.agg, H, N, H, H, w.slabs, false))) return rc;
    }
    if (grads->node_b1 && (rc = pvs64_colsum(s, grads->node_b1, w.g_u, H, N, H, w.slabs))) return rc;
    if ((rc = pvs64_gemm(s, g_h, H, w.g_u, H, params->node_w1, 1, 2 * H, nullptr, N, H, H, true))) return rc;
    if ((rc = pvs64_gemm(s, w.g_agg, H, w.g_u, H, params->node_w1 + H, 1, 2 * H, nullptr, N, H, H, false))) return rc;

    // edges: row side
    if ((rc = node_pre(s, desc, params, h, N, w.P, w.Q))) return rc;
    E64Args a = edge_args(desc, graph, params, x, eres ? m_prev : nullptr, w.P, w.Q);
    a.att = att;
    a.g_agg = w.g_agg;
    a.g_xout = g_x_out;
    a.g_mout = E ? g_m_out : nullptr;
    a.gz1 = w.gz1;
    a.gd = w.gd;
    a.g_mp = g_m_prev;
    a.a1s = w.a1s;
    a.gz2s = w.gz2s;
    a.ms = w.ms;
    a.gc1s = w.gc1s;
    a.gP = w.gP;
    a.gxrow = w.gxrow;
    a.rp = w.rp;
    PVS_REQUIRE(!a.eres || !(a.rezero || a.gated) || a.egate, "%s: missing edge_gate_parameter", who);
    if ((rc = launch_edge_any(H, s, true, a))) return rc;
    // column side
    if (E > 0) {
        hipLaunchKernelGGL(k64_col_gather, dim3(blocks_for((long long)N * (H + 3))), dim3(256), 0, s, graph->colptr,
                           graph->cedge, N, H, w.gz1, w.gd, w.gxrow, g_x_out, w.gQ, g_x);
        PVS_CHECK_LAUNCH();
    } else {
        PVS_CHECK_HIP(hipMemsetAsync(w.gQ, 0, NH * sizeof(double), s));
        if (g_x) {
            if (g_x_out) PVS_CHECK_HIP(hipMemcpyAsync(g_x, g_x_out, (size_t)N * 3 * sizeof(double),
                                                      hipMemcpyDeviceToDevice, s));
            else PVS_CHECK_HIP(hipMemsetAsync(g_x, 0, (size_t)N * 3 * sizeof(double), s));
        }
    }

    // edge_mlp.0: h rows / cols, radial and class columns, bias
    const bool perm = f & PVS_PERM_INVARIANT;
    const int ld1 = a.ld1, KP = 6 * H + 2;
    if ((rc = pvs64_gemm(s, g_h, H, w.gP, H, params->edge_w1, 1, ld1, nullptr, N, H, H, true))) return rc;
    if ((rc = pvs64_gemm(s, g_h, H, w.gQ, H, params->edge_w1 + (perm ? 0 : H), 1, ld1, nullptr, N, H, H, true)))
        return rc;
    if (grads->edge_w1) {
        if ((rc = pvs64_atb(s, grads->edge_w1, ld1, w.gP, H, h, H, N, H, H, w.slabs, false))) return rc;
        if ((rc = pvs64_atb(s, grads->edge_w1 + (perm ? 0 : H), ld1, w.gQ, H, h, H, N, H, H, w.slabs, perm)))
            return rc;
        if ((rc = pvs64_atb(s, grads->edge_w1 + a.base1, ld1, w.rp + 2 * H, KP, nullptr, 0, N, H, 1, w.slabs, false)))
            return rc;
        for (int t = 0; t < desc->n_edge_attr; ++t)
            if ((rc = pvs64_atb(s, grads->edge_w1 + a.base1 + 1 + t, ld1, w.rp + (3 + t) * H, KP, nullptr, 0, N, H, 1,
                                w.slabs, false)))
                return rc;
    }
    if (grads->edge_b1 && (rc = pvs64_colsum(s, grads->edge_b1, w.gP, H, N, H, w.slabs))) return rc;
    // edge_mlp.2
    if (grads->edge_w2 && (rc = pvs64_atb(s, grads->edge_w2, H, w.gz2s, H, w.a1s, H, E, H, H, w.slabs, false)))
        return rc;
    if (grads->edge_b2 && (rc = pvs64_colsum(s, grads->edge_b2, w.gz2s, H, E, H, w.slabs))) return rc;
    // coord_mlp (live when the coordinates were updated and a gradient arrived for them)
    if ((f & PVS_UPDATE_COORDS) && g_x_out) {
        if (grads->coord_w1 && (rc = pvs64_atb(s, grads->coord_w1, H, w.gc1s, H, w.ms, H, E, H, H, w.slabs, false)))
            return rc;
        if (grads->coord_b1 && (rc = pvs64_colsum(s, grads->coord_b1, w.gc1s, H, E, H, w.slabs))) return rc;
        if (grads->coord_w2 && (rc = pvs64_colsum(s, grads->coord_w2, w.rp, KP, N, H, w.slabs))) return rc;
    }
    // attention and the edge gate
    if (f & PVS_EDGE_ATTENTION) {
        if (grads->att_w && (rc = pvs64_colsum(s, grads->att_w, w.rp + H, KP, N, H, w.slabs))) return rc;
        if (grads->att_b && (rc = pvs64_colsum(s, grads->att_b, w.rp + 6 * H, KP, N, 1, w.slabs))) return rc;
    }
    if (a.eres && (a.rezero || a.gated) && grads->edge_gate)
        if ((rc = pvs64_colsum(s, grads->edge_gate, w.rp + 6 * H + 1, KP, N, 1, w.slabs))) return rc;
    // (a graph without edges: the caller's [0, H] m_prev has no device pointer; the gate's gradient is the sum over no edges)
    if (E == 0 && !a.eres && (f & PVS_EDGE_RESIDUAL) && (a.rezero || a.gated) && grads->edge_gate)
        PVS_CHECK_HIP(hipMemsetAsync(grads->edge_gate, 0, sizeof(double), s));
    return 0;
}
