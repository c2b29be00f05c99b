// MFMA edge kernels for H = 32*HB (HB = 1, 2): the fast path of EGNNLayer's per-edge work.
//
// Tile = 32 consecutive CSR-sorted edges per wavefront. Activations live in the "X layout" of
// v_mfma_f32_32x32x2_f32 accumulators: lane l = (edge slot j = l&31, half hh = l>>5), register t
// of channel block b holds channel 32b + (t&3) + 8(t>>2) + 4hh. An accumulator in that layout is
// directly the B operand of the next product over channels (k pairs {ch(t,0), ch(t,1)}), so the
// edge-MLP chain  z1 -> SiLU -> W2 -> SiLU -> Wc1 -> SiLU  needs no lane movement; the weights
// are staged once per workgroup in LDS in A-operand order (one ds_read_b32 per MFMA).
// The first edge-MLP layer is algebraically split per node (P_i + Q_j + w_rho*rho + W_a[type]),
// so the per-edge MFMA work is the HxH products only.
// Per-row sums (the reference's scatter-sum / scatter-mean, egnn_satorras.py:332-347): each wave
// owns a row-aligned, edge-balanced chunk of the CSR; a tile's weighted messages go through a
// per-wave LDS tile and are re-read channel-per-lane, where segment boundaries are wave-uniform
// scalars: no atomics, fixed summation order, bitwise reproducible.
//
// Layout maps validated lane-by-lane in tools/mfma_layout_check.py.
#include "edge_mfma_common.h"
// Node gathers and index loads with a scalar base + 32-bit lane offset (pvs_off, edge_mfma_common.h): 1-2 registers
// fewer at both widths, the H = 32 forward -2.6 %, cfg5 +1.7 % poses/s. Withdrawn earlier in round 5 because one register
// allocation of the H = 64 instantiation returned NaN rows; that was the unprotected inline-asm -> MFMA hazard of the
// operand split (pvs_f16_split2 has the story, tools/asm_mfma_hazard_scan.py finds such places), which any change of
// schedule could expose - with the conversions back in the compiler's hands the same build is green.

namespace {

// F16X2 (round 3): the two chain products as three-term fp16 products with power-of-two operand scales - per EDGE
// since round 4 (pvs_edge_scale_blocks, edge_mfma_common.h)
// instead of six-term bf16 products: half the MFMAs, 2 instead of 5.5 VALU instructions per split value.
// MODE (H = 128, where two split weight matrices do not fit in LDS beside the waves' tiles: the layer's edge forward runs
// as two launches): 0 everything; 1 everything but the coordinate branch, with only W2 staged - the messages go to
// io.m_out; 2 the coordinate branch alone, with only Wc1 staged - it reads the messages back from io.m_out.
// SA32: node rows and index arrays addressed as a scalar base + a 32-bit lane offset (pvs_off: -2.6 % at H = 32); the
// launcher takes the 64-bit instantiation when a table outgrows 32-bit byte offsets (N * 8H >= 2^32 or E >= 2^30)
template <int HB, int NT = kThreads, bool SOFT = false, bool F16X2 = false, int MODE = 0, bool SA32 = true>
__global__ void __launch_bounds__(NT, (F16X2 && HB == 1) ? 4 : (F16X2 && NT == 768) ? 3 : 1)
k_edge_fwd_mfma(PvsGraph g, PvsEdgeW w, uint32_t flags, int att_act, PvsEdgeFwdIO io, int n_chunks,
                int e_lo, int e_hi, PvsEdgePlan plan) {
    constexpr int H = 32 * HB;
    static_assert(MODE == 0 || F16X2, "the two-launch form exists for the f16x2 kernels");
    constexpr int TS = H + 4;   // tile row stride (floats): conflict-free b128 writes / b32 reads
    if (g.n_edges_dev) {        // edge count only known on the device: e_hi is the room of the edge arrays
        e_hi = min(e_hi, *g.n_edges_dev);
        // the chunks the host would have planned for this count: the room decides the grid, never a row's sums
        n_chunks = __builtin_amdgcn_readfirstlane(pvs_edge_replan(plan, e_hi - e_lo));      // (uniform: keep it scalar)
    }
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NW = NT / 64;
    constexpr int kBlkWords = 4 * 64 * 4;      // one 32x32 block as f16x2: 4 KB
    constexpr int kMats = MODE == 0 ? 2 : 1;
    constexpr int kWeightWords = F16X2 ? kMats * HB * HB * kBlkWords + 4 : 2 * H * H;
    float* W2s = smem;
    float* Wc1s = W2s + H * H;
    float* b2t = smem + kWeightWords;
    float* bc1t = b2t + H;
    float* wc2t = bc1t + H;
    float* wat = wc2t + H;
    float* wrhot = wat + H;
    float* attrt = wrhot + H;                            // [max(n_attr, 1)][H]
    const int attr_rows = w.n_attr > 1 ? w.n_attr : 1;
    float* wave_base = attrt + attr_rows * H;            // per wave: tile[32][TS], tx[32][4], rowbuf[32]
    constexpr int kWaveFloats = kTile * TS + kTile * 4 + kTile;

    const bool upd = MODE != 1 && (flags & PVS_UPDATE_COORDS);
    const bool eatt = MODE != 2 && (flags & PVS_EDGE_ATTENTION);
    constexpr bool soft = SOFT;      // softmax attention: its own instantiation (keeps the others' registers)
    const bool eres = (flags & PVS_EDGE_RESIDUAL) && io.m_prev != nullptr;

    // F16X2: each 32x32 block takes 2 parts x 2 k-steps x 64 lanes x 16 B = 4 KB
    unsigned* W2b = reinterpret_cast<unsigned*>(W2s);
    unsigned* Wc1b = MODE == 0 ? W2b + HB * HB * kBlkWords : W2b;      // (one matrix per launch: the same slot)
    float inv_sw2 = 1.f, inv_swc1 = 1.f;
    if constexpr (F16X2) {
        unsigned* wmax = W2b + kMats * HB * HB * kBlkWords;     // [0]: max |W2|, [1]: max |Wc1| (fp32 bits)
        if (threadIdx.x < 4) wmax[threadIdx.x] = 0u;
        __syncthreads();
        if (MODE != 2) pvs_block_absmax(w.w2, H * H, wmax);
        if (upd) pvs_block_absmax(w.wc1, H * H, wmax + 1);
        __syncthreads();
        const float sw2 = pvs_f16_scale(wmax[0], &inv_sw2);
        const float swc1 = pvs_f16_scale(wmax[1], &inv_swc1);
        if (MODE != 2) stage_weights_f16x2_blocks<HB>(W2b, w.w2, sw2);
        if (upd) stage_weights_f16x2_blocks<HB>(Wc1b, w.wc1, swc1);
    } else {
        stage_weights<HB>(W2s, w.w2, false);
        if (upd) stage_weights<HB>(Wc1s, w.wc1, false);
    }
    for (int c = threadIdx.x; c < H; c += NT) {
        b2t[c] = w.b2[c];
        bc1t[c] = upd ? w.bc1[c] : 0.f;
        wc2t[c] = upd ? w.wc2[c] : 0.f;
        wat[c] = eatt ? w.wa[c] : 0.f;
        wrhot[c] = w.w1[c * w.ld1 + w.off_rho];
        for (int t = 0; t < attr_rows; ++t)
            attrt[t * H + c] = t < w.n_attr ? w.w1[c * w.ld1 + w.off_rho + 1 + t] : 0.f;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = lane & 31, hh = lane >> 5;
    float* tile = wave_base + wv * kWaveFloats;
    float* tx = tile + kTile * TS;
    int* rowbuf = reinterpret_cast<int*>(tx + kTile * 4);
    const float bac = eatt ? w.ba[0] : 0.f;
    float gate = 1.f;
    if (eres && (flags & (PVS_REZERO | PVS_GATED_RESIDUAL))) {
        gate = w.edge_gate[0];
        if (flags & PVS_GATED_RESIDUAL) gate = fmaxf(gate, 0.f);
    }
    // edge residual without per-element branches: m = res_a * m_new + res_b * m_prev
    const float res_a = (flags & (PVS_REZERO | PVS_GATED_RESIDUAL)) ? gate : 1.f;
    const float res_b = (flags & PVS_GATED_RESIDUAL) ? 1.f - gate : 1.f;

    const int total_waves = gridDim.x * NW;
    for (int chunk = pvs_xcd_block(blockIdx.x, gridDim.x) * NW + wv; chunk < n_chunks; chunk += total_waves) {
        // (never past e_hi: the per-edge outputs are stored unclamped. A chunk end is rowptr[row[t]], which exceeds t only
        // where rowptr and row are not of one graph - a builder that overflowed keeps the true counts in rowptr and an
        // earlier call's rows; such a launch may compute nonsense, inside its buffers)
        const int e_begin = min(chunk_begin(g, chunk, n_chunks, e_lo, e_hi), e_hi);
        const int e_end = min(chunk_begin(g, chunk + 1, n_chunks, e_lo, e_hi), e_hi);
        int cur_row = -1;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), accx = acc;   // open row: lane = (row slot, quad)
        constexpr int QPR = H / 4;
        const int quad = lane % QPR, rsub = lane / QPR;

        // softmax attention: running maximum of the open row's logits (online softmax: the open row's
        // sums are rescaled when the maximum grows; tx[.].w carries the weights' sum)
        float mu_open = -INFINITY;
        auto flush = [&](int row_id) {
            if (row_id >= 0) {
                float4 tot = sum_row_slots<HB>(acc);
                float4 tx4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (upd || soft) tx4 = sum_row_slots<HB>(accx);
                if constexpr (soft) {
                    const float inv = tx4.w > 0.f ? 1.f / tx4.w : 0.f;
                    tot.x *= inv; tot.y *= inv; tot.z *= inv; tot.w *= inv;
                    if (lane == 0) io.ssum[row_id] = tx4.w;
                }
                if (MODE != 2 && rsub == 0) *reinterpret_cast<float4*>(io.Magg + (size_t)row_id * H + 4 * quad) = tot;
                if (upd) {
                    if (lane == 0) {
                        if (flags & kFwdRawXsum) {
                            io.x_out[3 * row_id] = tx4.x;
                            io.x_out[3 * row_id + 1] = tx4.y;
                            io.x_out[3 * row_id + 2] = tx4.z;
                        } else {
                            const float inv = g.inv_deg[row_id];
                            io.x_out[3 * row_id] = io.x[3 * row_id] + tx4.x * inv;
                            io.x_out[3 * row_id + 1] = io.x[3 * row_id + 1] + tx4.y * inv;
                            io.x_out[3 * row_id + 2] = io.x[3 * row_id + 2] + tx4.z * inv;
                        }
                    }
                }
            }
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            accx = acc;
        };

        // tile t+1's indices are loaded at the top of tile t (its node rows at its own start)
        TileIdx I = SA32 ? load_tile_idx32(g, w.n_attr | ((flags & kAblNoGather) ? 0x100 : 0), e_begin, e_begin, e_end, j)
                                  : load_tile_idx(g, w.n_attr | ((flags & kAblNoGather) ? 0x100 : 0), e_begin, e_begin, e_end, j);
        TileGather<HB> G;
        for (int e0 = e_begin; e0 < e_end; e0 += kTile) {
            const int e_next = (e0 + kTile < e_end) ? e0 + kTile : e0;
            const TileIdx In = SA32 ? load_tile_idx32(g, w.n_attr | ((flags & kAblNoGather) ? 0x100 : 0), e_next, e_begin, e_end, j)
                                             : load_tile_idx(g, w.n_attr | ((flags & kAblNoGather) ? 0x100 : 0), e_next, e_begin, e_end, j);
            const int e = I.e, ee = I.ee, i = I.i;
            const bool valid = I.valid;
            const unsigned long long ball = __ballot(valid && hh == 0 && i != I.prev_row);
            const unsigned bmask = (unsigned)ball;
            float d0, d1, d2;
            if constexpr (MODE == 2) {
                d0 = io.x[3 * I.i] - io.x[3 * I.jn];
                d1 = io.x[3 * I.i + 1] - io.x[3 * I.jn + 1];
                d2 = io.x[3 * I.i + 2] - io.x[3 * I.jn + 2];
            } else {
                if (SA32) gather_tile32<HB>(io.PQ, io.x, I, hh, G); else gather_tile<HB>(io.PQ, io.x, I, hh, G);
                d0 = G.d0; d1 = G.d1; d2 = G.d2;
            }
            const float rho = d0 * d0 + d1 * d1 + d2 * d2;

            float m[HB][16];
            if constexpr (MODE == 2) {      // the messages of the first launch (final: edge residual applied)
                load_x<HB>(io.m_out + (size_t)ee * H, hh, m);
            } else {
            // ---- first layer: z1 = P_i + Q_j + w_rho*rho + W_a[type]; a1 = SiLU(z1) ----
            float a1[HB][16];
            assemble_z1<HB>(G, attrt, wrhot, I.ty, hh, rho, a1);
#pragma unroll
            for (int b = 0; b < HB; ++b)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    if constexpr (pvs_pair_math<HB>) {
                        const pvs_f2 av = pvs_silu2(pvs_f2{a1[b][r], a1[b][r + 1]});
                        a1[b][r] = av.x; a1[b][r + 1] = av.y;
                    } else {
                        a1[b][r] = pvs_silu(a1[b][r]); a1[b][r + 1] = pvs_silu(a1[b][r + 1]);
                    }
                }
            // ---- second layer on the matrix cores: m = SiLU(W2 a1 + b2) ----
            {
                f32x16 acc2[HB];
                float bias[HB][16];
                if constexpr (!F16X2) load_tab<HB>(b2t, hh, bias);
                if constexpr (F16X2) {
                    float inv_s;
                    const float s_a = pvs_edge_scale_blocks<HB>(a1, &inv_s);      // (per edge: one column of the product)
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc2[b][r] = 0.f;
                    mfma_chain_f16x2_blocks<HB>(W2b, lane, a1, s_a, acc2);
                    load_tab<HB>(b2t, hh, bias);      // (after the chain: not live across it)
                    const float k2 = inv_s * inv_sw2;
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            if constexpr (pvs_pair_math<HB>) {
                                const pvs_f2 mv = pvs_silu2(pvs_fma2(pvs_f2{acc2[b][r], acc2[b][r + 1]}, pvs_f2{k2, k2}, pvs_f2{bias[b][r], bias[b][r + 1]}));
                                m[b][r] = mv.x; m[b][r + 1] = mv.y;
                            } else {
                                m[b][r] = pvs_silu(fmaf(acc2[b][r], k2, bias[b][r]));
                                m[b][r + 1] = pvs_silu(fmaf(acc2[b][r + 1], k2, bias[b][r + 1]));
                            }
                        }
                } else {
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc2[b][r] = bias[b][r];
                    mfma_chain<HB>(W2s, lane, a1, acc2, flags & kAblNoMfma);
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) m[b][r] = pvs_silu(acc2[b][r]);
                }
            }
            if (eres) {
#pragma unroll
                for (int b = 0; b < HB; ++b)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const float4 mp = *reinterpret_cast<const float4*>(
                            io.m_prev + (size_t)ee * H + 32 * b + 8 * gq + 4 * hh);
                        const float mpv[4] = {mp.x, mp.y, mp.z, mp.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float& mv = m[b][4 * gq + q];
                            mv = fmaf(res_a, mv, res_b * mpv[q]);
                        }
                    }
            }
            if (io.m_out && valid) {
#pragma unroll
                for (int b = 0; b < HB; ++b)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        *reinterpret_cast<float4*>(io.m_out + (size_t)e * H + 32 * b + 8 * gq + 4 * hh) =
                            make_float4(m[b][4 * gq], m[b][4 * gq + 1], m[b][4 * gq + 2], m[b][4 * gq + 3]);
            }
            }   // MODE != 2
            // ---- coordinate branch: s = wc2 . SiLU(Wc1 m + bc1) ----
            float s = 0.f;
            if (upd) {
                f32x16 accc[HB];
                float bias[HB][16];
                if constexpr (!F16X2) load_tab<HB>(bc1t, hh, bias);
                float q[HB][16];
                if constexpr (F16X2) {
                    float inv_s;
                    const float s_m = pvs_edge_scale_blocks<HB>(m, &inv_s);
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accc[b][r] = 0.f;
                    mfma_chain_f16x2_blocks<HB>(Wc1b, lane, m, s_m, accc);
                    load_tab<HB>(bc1t, hh, bias);
                    const float kc = inv_s * inv_swc1;
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            if constexpr (pvs_pair_math<HB>) {
                                const pvs_f2 qv = pvs_silu2(pvs_fma2(pvs_f2{accc[b][r], accc[b][r + 1]}, pvs_f2{kc, kc}, pvs_f2{bias[b][r], bias[b][r + 1]}));
                                q[b][r] = qv.x; q[b][r + 1] = qv.y;
                            } else {
                                q[b][r] = pvs_silu(fmaf(accc[b][r], kc, bias[b][r]));
                                q[b][r + 1] = pvs_silu(fmaf(accc[b][r + 1], kc, bias[b][r + 1]));
                            }
                        }
                } else {
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) accc[b][r] = bias[b][r];
                    mfma_chain<HB>(Wc1s, lane, m, accc, flags & kAblNoMfma);
#pragma unroll
                    for (int b = 0; b < HB; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) q[b][r] = pvs_silu(accc[b][r]);
                }
                s = dot_tab<HB>(wc2t, hh, q);
                if (flags & PVS_TANH) s = pvs_tanh(s);
                if (flags & PVS_NORMALIZE) s = s / (sqrtf(rho) + 1e-8f);
            }
            // ---- attention gate ----
            float a = 1.f;
            if (eatt) {
                const float logit = dot_tab<HB>(wat, hh, m) + bac;
                if constexpr (soft) {
                    // segment = row within the tile (0: the row left open by the previous tile)
                    const int sg = __popc(bmask & (j == 31 ? 0xffffffffu : ((2u << j) - 1u)));
                    const int nseg = __popc(bmask);
                    float shift = 0.f, last = mu_open;
                    for (int sgi = 0; sgi <= nseg; ++sgi) {
                        float mx = (valid && sg == sgi) ? logit : -INFINITY;
#pragma unroll
                        for (int o = 1; o < 32; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                        if (sgi == 0) {
                            const float nm = fmaxf(mu_open, mx);
                            const float f = (mu_open == -INFINITY) ? 0.f : __expf(mu_open - nm);
                            acc.x *= f; acc.y *= f; acc.z *= f; acc.w *= f;
                            accx.w *= f;
                            mx = nm;
                        }
                        if (sg == sgi) shift = mx;
                        last = mx;
                    }
                    mu_open = last;
                    a = valid ? __expf(logit - shift) : 0.f;
                    if (valid && hh == 0) { io.att_out[e] = logit; io.smax[i] = shift; }   // finalised after the kernel
                } else {
                    a = pvs_att_act(att_act, logit);
                    if (valid && hh == 0) io.att_out[e] = a;
                }
            }
            // ---- hand the weighted messages to the channel-per-lane reduction ----
            const float wgt = valid ? a : 0.f;
            if constexpr (MODE != 2) {
#pragma unroll
            for (int b = 0; b < HB; ++b)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                {
                    if constexpr (pvs_pair_math<HB>) {
                        const pvs_f2 lo = pvs_f2{m[b][4 * gq], m[b][4 * gq + 1]} * wgt, hi = pvs_f2{m[b][4 * gq + 2], m[b][4 * gq + 3]} * wgt;
                        *reinterpret_cast<float4*>(tile + j * TS + 32 * b + 8 * gq + 4 * hh) = make_float4(lo.x, lo.y, hi.x, hi.y);
                    } else {
                        *reinterpret_cast<float4*>(tile + j * TS + 32 * b + 8 * gq + 4 * hh) =
                            make_float4(wgt * m[b][4 * gq], wgt * m[b][4 * gq + 1], wgt * m[b][4 * gq + 2],
                                        wgt * m[b][4 * gq + 3]);
                    }
                }
            }
            if (hh == 0) {
                const float sv = valid ? s : 0.f;
                *reinterpret_cast<float4*>(tx + j * 4) = make_float4(d0 * sv, d1 * sv, d2 * sv, soft ? wgt : 0.f);
                rowbuf[j] = i;
            }
            I = In;
            pvs_wave_lds_sync();
            if (!(flags & kAblNoReduce))
                reduce_rows_tile<HB, soft, MODE != 2>(tile, tx, rowbuf, bmask, lane, acc, accx, cur_row, flush,
                                     [](int, int, const float4&) {});
            pvs_wave_lds_sync();
        }
        flush(cur_row);
    }
}



}  // namespace

namespace {
__global__ void k_init_fwd(float* __restrict__ Magg, const float* __restrict__ x, float* __restrict__ x_out,
                           int N, int H, int raw_xsum) {
    const int qpr = H / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t / qpr, q = t - n * qpr;
    if (n >= N) return;
    *reinterpret_cast<float4*>(Magg + (size_t)n * H + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q == 0 && raw_xsum) { x_out[3 * n] = 0.f; x_out[3 * n + 1] = 0.f; x_out[3 * n + 2] = 0.f; }
    else if (q == 0 && x) { x_out[3 * n] = x[3 * n]; x_out[3 * n + 1] = x[3 * n + 1]; x_out[3 * n + 2] = x[3 * n + 2]; }
}

// One launch of k_edge_fwd_mfma<HB, NT, SOFT, F16X2, MODE, SA32>: the softmax form and the offset width picked at run time
// (MODE 2, the coordinate branch alone, has no attention: only its SOFT = false form exists)
template <int HB, int NT, bool F16X2, int MODE>
int launch_fwd(hipStream_t s, bool soft, bool sa32, PvsEdgeGrid grid, PvsEdgePlan plan, size_t lds, const PvsGraph& g,
               const PvsEdgeW& w, uint32_t flags, int att_act, const PvsEdgeFwdIO& io) {
    return pvs_dispatch<MODE == 2 ? 1 : 2>(soft, sa32, [&](auto SF, auto SA) {
        auto kernel = k_edge_fwd_mfma<HB, NT, decltype(SF)::value != 0, F16X2, MODE, decltype(SA)::value>;
        if (set_lds(kernel, lds)) return -2;
        kernel<<<grid.blocks, NT, lds, s>>>(g, w, flags, att_act, io, grid.n_chunks, 0, g.n_edges, plan);
        PVS_CHECK_LAUNCH();
        return 0;
    });
}
}  // namespace

int pvs_launch_edge_fwd_mfma(hipStream_t s, int H, PvsEdgeFamily fam, const PvsGraph& g, const PvsEdgeW& w, uint32_t flags,
                             int att_act, const PvsEdgeFwdIO& io) {
    PVS_REQUIRE(w.n_attr <= PVS_MAX_EDGE_ATTR, "edge_attr classes %d > %d", w.n_attr,
                PVS_MAX_EDGE_ATTR);
    PVS_REQUIRE(fam == PVS_EDGE_WIDE ? H == 128 : ((fam == PVS_EDGE_SPLIT || fam == PVS_EDGE_EXACT) && (H == 32 || H == 64)),
                "MFMA edge forward: no kernel of family %d for H = %d", (int)fam, H);
    // (32-bit byte offsets into the node tables [N, 2H] fp32 and the edge index arrays: pvs_off; beyond them the 64-bit
    // instantiation of the same kernel runs: PVS_FWD_SADDR=0 at run time forces it for the test)
    const char* sa_env = getenv("PVS_FWD_SADDR");
    const bool force64 = sa_env && sa_env[0] == '0';
    const bool sa32 = !force64 && (long long)g.n_nodes * 8 * H < (1ll << 32) && g.n_edges < (1 << 30);
    // rows without edges are never flushed: M = 0, x_out = x
    if (!io.init_done) {
        const long long threads = (long long)g.n_nodes * (H / 4);
        k_init_fwd<<<(int)((threads + 255) / 256), 256, 0, s>>>(io.Magg, (flags & PVS_UPDATE_COORDS) ? io.x : nullptr,
                                                                io.x_out, g.n_nodes, H, (flags & kFwdRawXsum) ? 1 : 0);
        PVS_CHECK_LAUNCH();
    }
    if (g.n_edges == 0) return 0;
    PvsProfScope prof(s, pvs_prof_fwd_tag());
    const int HB = H / 32;
    const int attr_rows = w.n_attr > 1 ? w.n_attr : 1;
    const bool soft = (flags & PVS_EDGE_ATTENTION) && (flags & PVS_SOFTMAX_ATT);
    if (fam == PVS_EDGE_WIDE) {
        // The wide layer (64 < hidden <= 128, padded to 128): two launches of the f16x2 kernel, one split weight matrix
        // (64 KB) in LDS each - everything but the coordinate branch, messages to m_out (or the scratch); then the
        // coordinate branch alone, reading the messages back. 256 threads, one workgroup per CU (138 KB of LDS).
        float* mbuf = io.m_out ? io.m_out : io.m_scratch;
        const bool upd = flags & PVS_UPDATE_COORDS;
        PVS_REQUIRE(mbuf || !upd, "H = 128 edge forward needs m_out or the message scratch");
        const PvsEdgeGrid grid = pvs_edge_grid(g.n_edges, kWaves, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges());
        const PvsEdgePlan plan = pvs_edge_plan(kWaves, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges());
        const size_t words = (size_t)16 * 4 * 64 * 4 + 4 + (5 + attr_rows) * H +
                             (size_t)kWaves * (kTile * (H + 4) + kTile * 4 + kTile);
        const size_t lds = words * sizeof(float);
        PvsEdgeFwdIO io1 = io;
        io1.m_out = upd ? mbuf : io.m_out;
        PVS_TRY(launch_fwd<4, kThreads, true, 1>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io1));
        if (upd) PVS_TRY(launch_fwd<4, kThreads, true, 2>(s, false, sa32, grid, plan, lds, g, w, flags, att_act, io1));
    } else {
        // split (default): the two chain products as three-term fp16 products with tile scales ("f16x2", round 3);
        // exact: fp32 MFMAs - the cross-check family of the tests. (The six-term bf16 form of rounds 1-2 is gone from
        // the library: same accuracy, twice the MFMAs, a dearer split.)
        const bool f16x2 = fam == PVS_EDGE_SPLIT;
        // H = 64: 32 KB of weight operands, one workgroup per CU: 768 threads = three waves per SIMD where the edge-class
        // table leaves room in the 160 KB of LDS (up to 3 classes), 512 threads otherwise
        const int nw = (HB == 2 && f16x2) ? (attr_rows <= 3 ? 12 : 8) : kWaves;
        const PvsEdgeGrid grid = pvs_edge_grid(g.n_edges, nw, nw >= 8 ? kPvsFwdLargeMaxBlocks : kPvsFwdMaxBlocks,
                                               pvs_edges_per_wave(), pvs_chunk_edges());
        const PvsEdgePlan plan = pvs_edge_plan(nw, nw >= 8 ? kPvsFwdLargeMaxBlocks : kPvsFwdMaxBlocks, pvs_edges_per_wave(),
                                               pvs_chunk_edges());
        const size_t words = (f16x2 ? (size_t)2 * HB * HB * 4 * 64 * 4 + 4 : (size_t)2 * H * H) +
                             (5 + attr_rows) * H +
                             (size_t)nw * (kTile * (H + 4) + kTile * 4 + kTile);
        const size_t lds = words * sizeof(float);
        if (HB == 2 && f16x2 && nw == 12) PVS_TRY(launch_fwd<2, 768, true, 0>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io));
        else if (HB == 2 && f16x2) PVS_TRY(launch_fwd<2, 512, true, 0>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io));
        else if (HB == 1 && f16x2) PVS_TRY(launch_fwd<1, kThreads, true, 0>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io));
        else if (HB == 1) PVS_TRY(launch_fwd<1, kThreads, false, 0>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io));
        else PVS_TRY(launch_fwd<2, kThreads, false, 0>(s, soft, sa32, grid, plan, lds, g, w, flags, att_act, io));
    }
    // softmax attention: att_out holds the logits, the rows' maxima and sums are complete now
    if (soft) return pvs_launch_softmax_finalize(s, g, io.smax, io.ssum, io.att_out);
    return 0;
}
