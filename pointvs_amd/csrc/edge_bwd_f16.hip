// Edge backward for H = 32 with every product as a THREE-term fp16 product on the matrix cores ("f16x2",
// edge_mfma_common.h), one wave per 32-edge tile, two waves per SIMD (round 3; its bf16x3 predecessor needed six terms per
// product and three parts per operand).
//
// Per 32-edge tile:
//   * an operand is split into two fp16 parts by conversions (pvs_f16_split2: scale, v_cvt_pk, two v_fma_mix, v_cvt_pk:
//     2.5 vector instructions per value since the scale multiply runs on register pairs); the power-of-two tile scale
//     rides in the split;
//   * a chain product (W2 a1, Wc1 m, Wc1^T g_zc, W2^T g_z2) is 6 MFMAs;
//   * activations AND gradients (g_zc, g_z2) go to LDS as row-major [edge][channel] fp16 images (two parts = 4 KB per
//     tensor and wave), and BOTH operands of the two weight-gradient products over the edge index come back through the
//     transposing read (ds_read_b64_tr_b16);
//   * a weight-gradient product is 6 MFMAs (+ 4 for the bias column, a product with a ones column).
// 44 MFMAs per tile. Scales: one per operand and tile; in the instantiations without edge attention they move LAZILY and
// the weight gradients accumulate in the MFMA accumulators at the images' scale (below: wgrad_tile_f16_acc); with edge
// attention every tile takes its own scale from the wave-wide maximum and the products go through a temporary
// accumulator (wgrad_tile_f16). Elementwise work (SiLU and SiLU', descales, the split's scale) is written on register
// pairs (common.h pvs_f2). What bounds the kernel, measured phase by phase: DESIGN.md §5 / §8 item 1.
//
// Reference semantics: autograd of EGNNLayer.edge_model / coord_model / node_model's aggregation,
// /root/reference/point_vs/models/geometric/egnn_satorras.py:123-206 (SURVEY.md §8a "Backward spec").
#include "edge_mfma_common.h"

namespace {

constexpr int kH = 32;
constexpr int kPartShorts = 32 * kH;              // one fp16 part image of a [32 edges][32 channels] tensor
constexpr int kImg2 = 2 * kPartShorts;            // hi + lo

template <bool TRANSPOSE>
__device__ __forceinline__ f16x8 frag_f16(const unsigned short* __restrict__ part, int lane, int s) {
    return __builtin_bit_cast(f16x8, img_fragment_bits<1, TRANSPOSE>(part, lane, 0, 0, s));
}

// acc += (W s_w) (v s_v)  (TRANSPOSE: W^T), v given as its two fp16 parts (B operand, X layout); three terms,
// the smallest first
template <bool TRANSPOSE>
__device__ __forceinline__ void chain_f16(const unsigned short* __restrict__ img, int lane, const F16Parts& b,
                                          f32x16& acc) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f16x8 ah = frag_f16<TRANSPOSE>(img, lane, s);
        const f16x8 al = frag_f16<TRANSPOSE>(img + kH * kH, lane, s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b.hi[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.lo[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b.hi[s], acc, 0, 0, 0);
    }
}

// one fp16 part of a [32 edges][32 channels] tensor, X layout -> swizzled row-major image
__device__ __forceinline__ void write_part_f16(unsigned short* __restrict__ part, int j, int hh, const f16x8 (&p)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint4 u = __builtin_bit_cast(uint4, p[s]);
        // registers 8s..8s+3 hold channels 16s + 4hh + (0..3), registers 8s+4..8s+7 channels 16s + 8 + 4hh + (0..3):
        // neighbours in the image (img_off<1>)
        *reinterpret_cast<uint4*>(part + img_off<1>(j, 16 * s + 4 * hh)) = u;
    }
}

__device__ __forceinline__ void write_image_f16(unsigned short* __restrict__ img, int j, int hh, const F16Parts& b) {
    write_part_f16(img, j, hh, b.hi);
    write_part_f16(img + kPartShorts, j, hh, b.lo);
}

// gW (D layout [c = ch(r,hh)][k = j]) += inv_w * sum over the tile's edges of G'[e][c] * Act'[e][k], and
// gB[.][col] += inv_b * sum over the tile's edges of G'[e][.]  (the bias gradient belonging to G, as a product
// with a B operand that is all ones in column `col`: the matrix core does the sum over the edges).
// G' and Act' are the scaled fp16 images of the gradient and activation tensors; both operands are read
// transposed (k = edge index). inv_w = 1 / (s_G s_Act), inv_b = 1 / s_G.
__device__ __forceinline__ void wgrad_tile_f16(const unsigned short* __restrict__ g_img,
                                               const unsigned short* __restrict__ act_img,
                                               const unsigned* __restrict__ ones, int lane, float inv_w, float inv_b,
                                               f32x16& gW, f32x16& gB) {
    f32x16 t, tb;
#pragma unroll
    for (int r = 0; r < 16; ++r) { t[r] = 0.f; tb[r] = 0.f; }
    const f16x8 one = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(ones + lane * 4));
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f16x8 gh = frag_f16<true>(g_img, lane, s);
        const f16x8 gl = frag_f16<true>(g_img + kPartShorts, lane, s);
        const f16x8 ah = frag_f16<true>(act_img, lane, s);
        const f16x8 al = frag_f16<true>(act_img + kPartShorts, lane, s);
        t = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, ah, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, al, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, ah, t, 0, 0, 0);
        tb = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, one, tb, 0, 0, 0);
        tb = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, one, tb, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        gW[r] = fmaf(t[r], inv_w, gW[r]);
        gB[r] = fmaf(tb[r], inv_b, gB[r]);
    }
}

// ---- weight gradients accumulated IN the matrix core's accumulator (lazy tile scales, round 4) ----------------------
// wgrad_tile_f16 sums a tile into 32 temporary registers and folds them into the running sums with the tile's scales:
// 64 v_fma + 32 live registers per tile in a kernel whose register file is full. Here the running sums ARE the MFMA
// accumulators, kept at the scale of the operand images, and the images' scales move LAZILY: an operand keeps its
// power-of-two scale while the tile's largest magnitude stays within kLazyWindow binades below the scale's ceiling
// (s * max in [2^(13 - kLazyWindow), 2^14)); when it leaves the window the new scale puts it one binade below the
// ceiling, and the accumulators that carry the old scale are multiplied by the (power-of-two, exact) ratio - a rare,
// wave-uniform branch. Cost in accuracy: an element 2^-k below its tile's largest keeps 22 - max(0, k - 16 + d) bits,
// d <= kLazyWindow the distance of the tile maximum from the ceiling (d = 0 with per-tile scales).
// Scale ratios beyond 2^60 (a tile whose gradients are 2^-60 of what the accumulator holds, or the reverse) are not
// applied: the smaller side is below the fp32 resolution of the sum - the tile is skipped, or the accumulator restarts.
// Instantiations WITHOUT edge attention only: with it the bias tile gB also takes per-tile vector updates (the attention
// weight's gradient rides in its idle columns), which would wait out every MFMA that writes it (+22 % per launch), and a
// separate accumulator for those brings the spills back (5-57 VGPRs): they keep wgrad_tile_f16.
__device__ __forceinline__ void wgrad_tile_f16_acc(const unsigned short* __restrict__ g_img,
                                                   const unsigned short* __restrict__ act_img,
                                                   const unsigned* __restrict__ ones, int lane, f32x16& gW, f32x16& gB) {
    const f16x8 one = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(ones + lane * 4));
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const f16x8 gh = frag_f16<true>(g_img, lane, s);
        const f16x8 gl = frag_f16<true>(g_img + kPartShorts, lane, s);
        const f16x8 ah = frag_f16<true>(act_img, lane, s);
        const f16x8 al = frag_f16<true>(act_img + kPartShorts, lane, s);
        gW = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, ah, gW, 0, 0, 0);
        gW = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, al, gW, 0, 0, 0);
        gW = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, ah, gW, 0, 0, 0);
        gB = __builtin_amdgcn_mfma_f32_32x32x16_f16(gl, one, gB, 0, 0, 0);
        gB = __builtin_amdgcn_mfma_f32_32x32x16_f16(gh, one, gB, 0, 0, 0);
    }
}

// The two three-term sums over the coordinate difference d = x_i - x_j with their roundings WRITTEN OUT. Left to the
// compiler ("d0 * d0 + d1 * d1 + d2 * d2" under fp-contract), which products are paired into a packed multiply and which
// one is fused into the sum depends on what else uses d0..d2 in the instantiation - and rho feeds z1, the dot product the
// coordinate branch's gradients: the first-layer form, which has no per-edge coordinate gradient, came out with other
// pairings and every gradient a few ulps away from the general kernel's (tests/test_gpu_first_layer_backward.py). The
// orders below are the ones the general kernels were compiled to (sq_dist_f16 leaves their device code unchanged;
// dot3_f16 is used by the first-layer form alone, see the body).
__device__ __forceinline__ float sq_dist_f16(float d0, float d1, float d2) {
#pragma clang fp contract(off)
    const float a = d0 * d0, b = d1 * d1;
    const float ab = a + b;
    return __builtin_fmaf(d2, d2, ab);
}
__device__ __forceinline__ float dot3_f16(float d0, float d1, float d2, float g0, float g1, float g2) {
#pragma clang fp contract(off)
    const float a = d0 * g0, c = d2 * g2;
    const float ab = __builtin_fmaf(d1, g1, a);
    return ab + c;
}

struct F16Cfg {
    static constexpr int kThreadsPerBlock = 512;                          // two waves per SIMD
    static constexpr int kWavesPerBlock = kThreadsPerBlock / 64;
    static constexpr int kTS = kH + 4;                                    // g_z1 tile row stride (floats) of the padded form; the
                                                                          // BASELINE instantiation uses unpadded rows with rotated quads
    // per wave: a1 image, m image, gradient image (4 KB each), SiLU'(z1) (4 KB)
    static constexpr int kWaveBytes = 3 * kImg2 * 2 + 16 * 64 * 4;
    // shared: W2 and Wc1 images (hi + lo), tables, two ones columns, 4 words of weight maxima, one all-zero image
    // (what a weight-gradient product reads in place of an operand it must not add: pvs_rescale_acc)
    static constexpr int kSharedBytes = 2 * kImg2 * 2 + (5 + PVS_MAX_EDGE_ATTR) * kH * 4 + 2 * 64 * 16 + 16 + kImg2 * 2;
    static_assert(kTile * kTS * 4 + kTile * 16 + kTile * 4 <= 2 * kImg2 * 2, "g_z1 tile + tx + rowbuf must fit the m + gradient images");
};

// ERK: edge residual kind - 0 none; 1 the plain sum m + m_prev (nothing of the residual has to survive the tile's
// coordinate branch); 2 rezero (the gate's gradient needs the pre-residual message at the end); 3 gated (... and m_prev).
// (Before round 4 one kind read rezero or gated from the run-time flags.) Compile-time kinds took rezero from 18 / 31
// spilled VGPRs (without / with edge attention) to 2 / 9 and -11 % / -19 % per launch, gated + attention from 31 to 26 and
// -4 %; gated without attention is faster the old way (profiles/r04_variants_gated_rezero.txt).
// The kernels' text is edge_bwd_f16_body.h, shared with the first-layer form below (why as text: there).
template <int ERK, bool EATT>
__global__ void __launch_bounds__(F16Cfg::kThreadsPerBlock, 2)
k_edge_bwd_f16(PvsGraph g, PvsEdgeW w, uint32_t flags, int att_act, PvsEdgeBwdIO io, int n_chunks, int e_lo, int e_hi) {
    constexpr bool GX = true;
#include "edge_bwd_f16_body.h"
}

// The first-layer form (GX = false) of the BASELINE instantiation: no edge residual, no edge attention. Its own NAME, not a
// third template argument: tools and tests find k_edge_bwd_f16<0, false> by its mangled name.
__global__ void __launch_bounds__(F16Cfg::kThreadsPerBlock, 2)
k_edge_bwd_f16_nogx(PvsGraph g, PvsEdgeW w, uint32_t flags, int att_act, PvsEdgeBwdIO io, int n_chunks, int e_lo, int e_hi) {
    constexpr int ERK = 0;
    constexpr bool EATT = false, GX = false;
#include "edge_bwd_f16_body.h"
}

}  // namespace

// The MFMA backward contract of edge_kernels.h. H = 32 only.
int pvs_launch_edge_bwd_f16(hipStream_t s, int H, const PvsGraph& g, const PvsEdgeW& w, uint32_t flags, int att_act,
                            const PvsEdgeBwdIO& io, int e_lo, int e_hi, int* n_slabs) {
    PVS_REQUIRE(w.n_attr <= 3, "MFMA edge backward supports up to 3 edge classes (got %d)", w.n_attr);
    PVS_REQUIRE(H == 32, "f16x2 edge backward is built for H = 32 (got %d)", H);
    *n_slabs = 0;
    if (e_hi <= e_lo) return 0;
    using Cfg = F16Cfg;
    constexpr int nw = Cfg::kWavesPerBlock;
    // (chunks of 8192 edges: one chunk per wave at cfg2, pvs_chunk_edges)
    const PvsEdgeGrid grid = pvs_edge_grid(e_hi - e_lo, nw, kPvsBwdF16MaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges(8192));
    PVS_TRY(pvs_report_slabs(grid.blocks, n_slabs));
    PvsProfScope prof(s, PVS_PROF_EDGE_BWD);
    const PvsSlabLayout L = pvs_slab_layout(kH);
    size_t lds = (size_t)Cfg::kSharedBytes + (size_t)nw * Cfg::kWaveBytes;
    if (lds < (size_t)L.total * 4) lds = (size_t)L.total * 4;
    // ERK = the residual kind itself: 0 none, 1 sum, 2 rezero, 3 gated, all COMPILE-TIME. Until round 6 gated residual
    // without attention ran kind 4 (the kind read from the flags at run time: 11 spilled VGPRs against 13) - and kind 4 with
    // BOTH the lazy scales and the pair arithmetic compiled in gave g_z2-derived outputs that were 1e-3 ... 1e-1 off and
    // changed from run to run; either feature off, or kind 3, and it is bit-reproducible and within 1e-6 of the exact
    // family (profiles/r06_gated_residual_backward_defect.txt). The cause inside the instantiation was not found; the kind-4
    // code path is no longer instantiated. tools/backward_instantiations_probe.py and the GPU test of the same name run all
    // 24 instantiations of the H = 32 / 64 backward twice on a multi-tile graph.
    const int erk = pvs_edge_residual_kind(flags, io.m_prev != nullptr);
    if (!io.gx_row) {       // the first-layer form (pvs_first_layer_bwd): nobody reads the input coordinates' gradient
        PVS_REQUIRE(erk == 0 && !(flags & PVS_EDGE_ATTENTION) && io.gxagg,
                    "f16x2 edge backward: the first-layer form is built for plain layers with a coordinate update");
        if (set_lds(k_edge_bwd_f16_nogx, lds)) return -2;
        k_edge_bwd_f16_nogx<<<grid.blocks, Cfg::kThreadsPerBlock, lds, s>>>(g, w, flags, att_act, io, grid.n_chunks, e_lo, e_hi);
        PVS_CHECK_LAUNCH();
        return 0;
    }
    return pvs_dispatch<4>(erk, (flags & PVS_EDGE_ATTENTION) != 0, [&](auto ERK, auto EATT) {
        auto kernel = k_edge_bwd_f16<decltype(ERK)::value, decltype(EATT)::value>;
        if (set_lds(kernel, lds)) return -2;
        kernel<<<grid.blocks, Cfg::kThreadsPerBlock, lds, s>>>(g, w, flags, att_act, io, grid.n_chunks, e_lo, e_hi);
        PVS_CHECK_LAUNCH();
        return 0;
    });
}
