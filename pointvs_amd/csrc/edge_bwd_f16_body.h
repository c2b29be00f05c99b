// The tile loop of the H = 32 f16x2 edge backward (edge_bwd_f16.hip), as TEXT: each kernel there includes this file as its
// body, with its template parameters ERK and EATT, a constexpr bool GX and the kernel arguments (g, w, flags, att_act, io,
// n_chunks, e_lo, e_hi) in scope. Not a function: as a __device__ __forceinline__ template the compiler simplifies the
// body once on its own before it inlines it, and the general kernels come out as other code (the BASELINE instantiation
// with 5 spilled VGPRs instead of 2, its block-size read no longer folded: tools/device_code_diff.py against the
// kernel-with-body form, profiles/first_layer_backward.txt). Included text is compiled as if it stood in the kernel.
//
// GX: somebody reads the gradient of the layer's INPUT coordinates. Without it (the first layer of a model whose positions
// need no gradient: pvs_first_layer_bwd, edge_dispatch.h) the tile forms no g_rho = w_rho . g_z1 and no per-edge
// coordinate gradient gd, sums and stores no gx_row, and leaves ONE word per edge - rho | type, which the column gather
// still needs for g_wrho / g_wattr - at io.gd + e instead of the 16-byte record. Everything else (g_z1, gPQ, every
// weight gradient, the coordinate branch's own terms: g_x_out of that layer is live) is the same code in the same order.
// Compile-time only: the kernel has no scalar register left for a run-time flag (tests/test_kernel_resources.py).
    using Cfg = F16Cfg;
    constexpr int H = kH, NT = Cfg::kThreadsPerBlock, NW = Cfg::kWavesPerBlock;
    constexpr bool ERES = ERK != 0;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned short* W2i = reinterpret_cast<unsigned short*>(smem);         // hi, lo: [H][H] fp16 each
    unsigned short* Wc1i = W2i + kImg2;
    float* b2t = smem + kImg2;                                             // (2 images x kImg2 shorts = kImg2 floats)
    float* bc1t = b2t + H;
    float* wc2t = bc1t + H;
    float* wat = wc2t + H;
    float* wrhot = wat + H;
    float* attrt = wrhot + H;                                  // [PVS_MAX_EDGE_ATTR][H]
    unsigned* ones0 = reinterpret_cast<unsigned*>(attrt + PVS_MAX_EDGE_ATTR * H);   // [64 lanes][4]: fp16 ones, column 0 (g_bc1)
    unsigned* ones1 = ones0 + 64 * 4;               // ... column 1 (g_b2)
    unsigned* wmax = ones1 + 64 * 4;                // [0]: max |W2|, [1]: max |Wc1| (fp32 bits)
    unsigned short* ZI = reinterpret_cast<unsigned short*>(wmax + 4);      // kImg2 shorts of zeros
    char* wave_base = reinterpret_cast<char*>(ZI + kImg2);

    const bool upd = (flags & PVS_UPDATE_COORDS) && io.gxagg != nullptr;

    if (threadIdx.x < 4) wmax[threadIdx.x] = 0u;
    __syncthreads();
    pvs_block_absmax(w.w2, H * H, wmax);
    if (upd) pvs_block_absmax(w.wc1, H * H, wmax + 1);
    __syncthreads();
    float inv_sw2, inv_swc1;
    const float sw2 = pvs_f16_scale(wmax[0], &inv_sw2);
    const float swc1 = pvs_f16_scale(wmax[1], &inv_swc1);
    stage_weights_img_f16<1>(W2i, w.w2, sw2);
    if (upd) stage_weights_img_f16<1>(Wc1i, w.wc1, swc1);
    for (int c = threadIdx.x; c < H; c += NT) {
        b2t[c] = w.b2[c];
        bc1t[c] = upd ? w.bc1[c] : 0.f;
        wc2t[c] = upd ? w.wc2[c] : 0.f;
        wat[c] = EATT ? w.wa[c] : 0.f;
        wrhot[c] = w.w1[c * w.ld1 + w.off_rho];
        for (int t = 0; t < PVS_MAX_EDGE_ATTR; ++t)
            attrt[t * H + c] = t < w.n_attr ? w.w1[c * w.ld1 + w.off_rho + 1 + t] : 0.f;
    }
    for (int i = threadIdx.x; i < kImg2 / 2; i += NT) reinterpret_cast<unsigned*>(ZI)[i] = 0u;
    for (int i = threadIdx.x; i < 64 * 4; i += NT) {
        const int col = (i >> 2) & 31;
        ones0[i] = col == 0 ? 0x3c003c00u : 0u;      // fp16 1.0 pairs
        ones1[i] = col == 1 ? 0x3c003c00u : 0u;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = lane & 31, hh = lane >> 5;
    unsigned short* A1I = reinterpret_cast<unsigned short*>(wave_base + wv * Cfg::kWaveBytes);
    unsigned short* MI = A1I + kImg2;
    unsigned short* GI = MI + kImg2;
    float* d1b = reinterpret_cast<float*>(GI + kImg2);         // SiLU'(z1), X layout, lane-private
    // once the m and gradient images are dead (after the W2 weight gradient) their slots hold the g_z1 tile
    float* T1 = reinterpret_cast<float*>(MI);
    // The conflict-free tile layout (pvs_tile_quad_off: four write addresses that differ by an XOR, i.e. three more
    // lane constants than base + immediate) only where the registers are there: the BASELINE instantiation. The others
    // went from 1 / 3 / 9 / 28 to 5 / 11 / 15 / 30 spilled VGPRs with it (+3...16 % per launch) and keep the padded rows.
    constexpr bool TSWZ = ERK == 0 && !EATT;
    float* tx = T1 + kTile * Cfg::kTS;
    int* rowbuf = reinterpret_cast<int*>(tx + kTile * 4);

    const float bac = EATT ? w.ba[0] : 0.f;
    float gate_raw = 0.f, gate = 1.f;
    if constexpr (ERK == 2 || ERK == 3) {
        gate_raw = w.edge_gate[0];
        gate = ERK == 3 ? fmaxf(gate_raw, 0.f) : gate_raw;
    }
    const float res_a = ERK >= 2 ? gate : 1.f;
    const float res_b = ERK == 3 ? 1.f - gate : 1.f;

    // ---- accumulators that live for the whole kernel ----
    f32x16 gW2, gWc1;                          // D layout: [c = ch(r,hh)][k = j]
    // gB, D layout (rows = channels): column 0 = g_bc1, column 1 = g_b2 (ones-column products, wgrad_tile_f16). With
    // edge attention the OTHER 30 columns' lanes carry the attention weight's gradient g_wa as per-lane partial sums
    // (register r of lane (j, hh) is channel xch(r, hh) in the D layout and in the X layout alike, and the partial
    // sums are added over the lanes at the end anyway): the contributions of edges 0 and 1 go to lanes 2 and 3
    // through one DPP move. 16 kernel-lifetime registers less than a separate X-layout accumulator - what this
    // instantiation was spilling.
    f32x16 gB;
    float g_wc2x[16];                          // X layout (channel in the register, edges on lanes)
#pragma unroll
    for (int r = 0; r < 16; ++r) { gB[r] = 0.f; g_wc2x[r] = 0.f; gW2[r] = 0.f; gWc1[r] = 0.f; }
    float g_ba = 0.f, g_gate = 0.f;
    // (LAZY) scale exponents of the four operand images and what the accumulators carry
    constexpr bool LAZY = !EATT;
    // elementwise work on register pairs (common.h pvs_f2): everywhere but gated residual + attention, the instantiation
    // with the most live values per tile (30 spilled registers instead of 26 with it, +7 % per launch)
    constexpr bool PAIR = !(ERK == 3 && EATT);
    // (the four exponents share ONE scalar register, a byte each, 0 = not set yet: the kernel has no scalar register to
    // spare, and a spilled one costs a v_readlane / v_writelane pair per use)
    unsigned lazy_pack = 0u;
    auto lazy_scale = [&](const float (&v)[16], int slot, float* inv) {
        const int e = (int)((lazy_pack >> (8 * slot)) & 0xffu);
        LazyExp st{e ? e : -1};
        const float sc = pvs_lazy_tile_scale(v, st, inv);
        lazy_pack = (lazy_pack & ~(0xffu << (8 * slot))) | ((unsigned)st.e << (8 * slot));
        return sc;
    };
    auto lazy_e = [&](int slot) { return (int)((lazy_pack >> (8 * slot)) & 0xffu); };
    constexpr int kXa1 = 0, kXm = 1, kXg = 2, kXg2 = 3;
    AccUnits u_w2{-1}, u_b2{-1}, u_wc1{-1}, u_bc1{-1};

    const int total_waves = gridDim.x * NW;
    for (int chunk = pvs_xcd_block(blockIdx.x, gridDim.x) * NW + wv; chunk < n_chunks; chunk += total_waves) {
        // (wave-uniform values that come out of global loads: into scalar registers, the vector file is full)
        const int e_begin = __builtin_amdgcn_readfirstlane(chunk_begin(g, chunk, n_chunks, e_lo, e_hi));
        const int e_end = __builtin_amdgcn_readfirstlane(chunk_begin(g, chunk + 1, n_chunks, e_lo, e_hi));
        int cur_row = -1;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), accx = acc;   // open row: lane = (row slot, quad)
        constexpr int QPR = H / 4;
        const int quad = lane % QPR, rsub = lane / QPR;
        auto flush = [&](int row_id) {
            if (row_id >= 0) {
                const float4 tot = sum_row_slots<1>(acc);
                if (rsub == 0) *reinterpret_cast<float4*>(io.gPQ + (size_t)row_id * 2 * H + 4 * quad) = tot;
                if constexpr (GX) {
                    const float4 tx4 = sum_row_slots<1>(accx);
                    if (lane == 0) {
                        io.gx_row[3 * row_id] = tx4.x;
                        io.gx_row[3 * row_id + 1] = tx4.y;
                        io.gx_row[3 * row_id + 2] = tx4.z;
                    }
                }
            }
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            accx = acc;
        };
        // A tile shares ONE power-of-two scale per operand, and two graphs' gradients can differ by many orders of
        // magnitude (a saturated loss), so a tile ends where a graph ends (PvsGraph.graph_eptr, when the caller knows
        // the batch's graphs): gb = the first graph boundary behind the current tile's start.
        int gk = 0, gb = e_hi;
        if (g.graph_eptr) {
            int lo = 0, hi = g.n_graphs;                // last k with graph_eptr[k] <= e_begin
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (__builtin_amdgcn_readfirstlane(g.graph_eptr[mid]) <= e_begin) lo = mid; else hi = mid;
            }
            gk = lo + 1;
            gb = __builtin_amdgcn_readfirstlane(g.graph_eptr[gk]);
        }
        auto tile_end = [&](int start, int bound) { return min(min(start + kTile, e_end), bound > start ? bound : e_end); };
        int t_end = tile_end(e_begin, gb);
        // only what comes out of memory is carried from tile to tile (4 registers); e / ee / valid are recomputed
        struct Loaded { int i, jn, ty, prev_row; };
        auto load_idx = [&](int start, int end) {
            const TileIdx t = load_tile_idx(g, w.n_attr, start, e_begin, end, j);
            return Loaded{t.i, t.jn, t.ty, t.prev_row};
        };
        Loaded I = load_idx(e_begin, t_end);
        for (int e0 = e_begin; e0 < e_end;) {
            const int e_this_end = t_end;
            // the next tile: starts where this one ends; past a graph boundary the next boundary applies
            if (g.graph_eptr)    // (empty graphs repeat a boundary)
                while (gk < g.n_graphs && gb <= e_this_end) { ++gk; gb = __builtin_amdgcn_readfirstlane(g.graph_eptr[gk]); }
            const int e_next = e_this_end < e_end ? e_this_end : e0;
            const int n_end = e_this_end < e_end ? tile_end(e_this_end, gb) : e_this_end;
            const Loaded In = load_idx(e_next, n_end);
            const int e = e0 + j, i = I.i, ty = I.ty;
            const bool valid = e < e_this_end;
            const int ee = min(max(valid ? e : e_this_end - 1, 0), g.n_edges - 1);   // (as load_tile_idx clamps)
            const float vm = valid ? 1.f : 0.f;
            const unsigned bmask = (unsigned)__ballot(valid && hh == 0 && i != I.prev_row);
            float d0, d1, d2, rho;
            F16Parts pb;                      // parts of the tensor being pushed through a product
            float inv_sa1, inv_sm = 1.f;      // 1 / tile scale of the a1 and m images

            // ---- recompute: z1, a1 = SiLU(z1), SiLU'(z1); a1 image; z2 = W2 a1 + b2 ----
            float z2[16];
            {
                TileGather<1> G;
                TileIdx Ig;
                Ig.i = I.i; Ig.jn = I.jn;
                gather_tile<1>(io.PQ, io.x, Ig, hh, G);
                d0 = G.d0; d1 = G.d1; d2 = G.d2;
                rho = sq_dist_f16(d0, d1, d2);
                float a1[1][16];
                assemble_z1<1>(G, attrt, wrhot, ty, hh, rho, a1);
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    float dd[4];
                    if constexpr (PAIR) {
#pragma unroll
                        for (int q = 0; q < 4; q += 2) {
                            pvs_f2 av, dv;
                            pvs_silu_grad2(pvs_f2{a1[0][4 * gq + q], a1[0][4 * gq + q + 1]}, av, dv);
                            a1[0][4 * gq + q] = av.x; a1[0][4 * gq + q + 1] = av.y;
                            dd[q] = dv.x; dd[q + 1] = dv.y;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float z = a1[0][4 * gq + q];
                            const float sg = pvs_sigmoid(z);
                            const float av = z * sg;
                            dd[q] = fmaf(av, 1.0f - sg, sg);       // SiLU'(z) = s + z s (1 - s)
                            a1[0][4 * gq + q] = av;
                        }
                    }
                    *reinterpret_cast<float4*>(d1b + (gq * 64 + lane) * 4) = make_float4(dd[0], dd[1], dd[2], dd[3]);
                }
                const float sa1 = LAZY ? lazy_scale(a1[0], kXa1, &inv_sa1) : pvs_tile_scale(a1[0], &inv_sa1);
                split_f16x2<PAIR>(a1[0], sa1, pb);
                write_image_f16(A1I, j, hh, pb);
                f32x16 acc2;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
                chain_f16<false>(W2i, lane, pb, acc2);
                float bias[1][16];
                load_tab<1>(b2t, hh, bias);
                const float k2 = inv_sa1 * inv_sw2;
                if constexpr (PAIR) {
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const pvs_f2 z = pvs_fma2(pvs_f2{acc2[r], acc2[r + 1]}, pvs_f2{k2, k2}, pvs_f2{bias[0][r], bias[0][r + 1]});
                        z2[r] = z.x; z2[r + 1] = z.y;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) z2[r] = fmaf(acc2[r], k2, bias[0][r]);
                }
            }
            float dz2[16], m[1][16];          // SiLU'(z2) and the message
            float m_new[ERK >= 2 ? 16 : 1], mp[1][16];
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                if constexpr (PAIR) {
                    pvs_f2 mv, dv;
                    pvs_silu_grad2(pvs_f2{z2[r], z2[r + 1]}, mv, dv);
                    m[0][r] = mv.x; m[0][r + 1] = mv.y;
                    dz2[r] = dv.x; dz2[r + 1] = dv.y;
                } else {
                    for (int t = r; t < r + 2; ++t) {
                        const float sg = pvs_sigmoid(z2[t]);
                        m[0][t] = z2[t] * sg;
                        dz2[t] = fmaf(m[0][t], 1.0f - sg, sg);
                    }
                }
                if constexpr (ERK >= 2) { m_new[r] = m[0][r]; m_new[r + 1] = m[0][r + 1]; }
            }
            if constexpr (ERES) {
                load_x<1>(io.m_prev + (size_t)ee * H, hh, mp);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (ERK >= 2) m[0][r] = fmaf(res_a, m_new[r], res_b * mp[0][r]);
                    else m[0][r] += mp[0][r];
                }
            }

            // ---- gradient wrt m: the coordinate branch's term comes from the matrix core first; the external,
            // aggregated-message and attention terms are added AFTER it (g_m is then not live across the
            // coordinate branch) ----
            float gm[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) gm[r] = 0.f;
            float gMi[1][16];
            auto load_row_terms = [&]() { load_x<1>(io.gM + (size_t)i * H, hh, gMi); };
            // Edge attention: everything that needs the message itself - the logit, m . g_M, the gate's gradient g_l
            // and its weight gradient g_wa += g_l m - is evaluated HERE, while m is live anyway; two scalars (the gate
            // value and g_l) cross the coordinate branch and m dies with its split, as in the plain kernel. The g_M
            // row is fetched a second time behind the branch (an L1 hit: a tile's edges share their row).
            float att_v = 1.f, g_l = 0.f;
            if constexpr (EATT) {
                float logit = 0.f, dot = 0.f;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {       // (quad by quad: eight registers of operands at a time)
                    const float4 gq4 = *reinterpret_cast<const float4*>(io.gM + (size_t)i * H + 8 * gq + 4 * hh);
                    const float4 wq4 = *reinterpret_cast<const float4*>(wat + 8 * gq + 4 * hh);
                    logit = fmaf(wq4.x, m[0][4 * gq], logit); dot = fmaf(m[0][4 * gq], gq4.x, dot);
                    logit = fmaf(wq4.y, m[0][4 * gq + 1], logit); dot = fmaf(m[0][4 * gq + 1], gq4.y, dot);
                    logit = fmaf(wq4.z, m[0][4 * gq + 2], logit); dot = fmaf(m[0][4 * gq + 2], gq4.z, dot);
                    logit = fmaf(wq4.w, m[0][4 * gq + 3], logit); dot = fmaf(m[0][4 * gq + 3], gq4.w, dot);
                }
                logit = pvs_xor32_sum(logit);
                dot = pvs_xor32_sum(dot);
                logit += bac;
                const float aval = io.att[ee];
                g_l = (flags & PVS_SOFTMAX_ATT) ? aval * (dot - io.softD[i]) * vm   // softD = M_i . g_M_i
                                                : pvs_att_act_grad(att_act, logit, aval) * dot * vm;
                att_v = aval * vm;
                if (hh == 0) g_ba += g_l;
                const float g_own = j >= 2 ? g_l : 0.f;                    // this lane's own edge, columns 2..31
                const float k_23 = (j == 2 || j == 3) ? 1.f : 0.f;         // lanes that also take edges 0 / 1
                const float g_in = k_23 * __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(g_l), 0x4E, 0xf, 0xf, true));
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // m of lane j ^ 2 (quad_perm [2,3,0,1]); only lanes 2 and 3 use it (g_in is zero elsewhere)
                    const float mt = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m[0][r]), 0x4E, 0xf, 0xf, true));
                    gB[r] = fmaf(g_own, m[0][r], gB[r]);
                    gB[r] = fmaf(g_in, mt, gB[r]);
                }
            }
            auto add_row_terms = [&]() {
                if (io.g_m_out) {
                    float init[1][16];
                    load_x<1>(io.g_m_out + (size_t)ee * H, hh, init);
#pragma unroll
                    for (int r = 0; r < 16; ++r) gm[r] = fmaf(init[0][r], vm, gm[r]);
                }
                if constexpr (EATT) {
                    float wax[1][16];
                    load_tab<1>(wat, hh, wax);
#pragma unroll
                    for (int r = 0; r < 16; ++r) gm[r] += att_v * gMi[0][r] + g_l * wax[0][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) gm[r] = fmaf(vm, gMi[0][r], gm[r]);
                }
            };
            float s_coord = 0.f, nrm = 1.f;
            float gT0 = 0.f, gT1 = 0.f, gT2 = 0.f;
            if (upd) {
                const float* gT = io.gxagg + 3 * i;
                gT0 = gT[0]; gT1 = gT[1]; gT2 = gT[2];
                const float sm = LAZY ? lazy_scale(m[0], kXm, &inv_sm) : pvs_tile_scale(m[0], &inv_sm);
                split_f16x2<PAIR>(m[0], sm, pb);
                write_image_f16(MI, j, hh, pb);
                f32x16 accc;
#pragma unroll
                for (int r = 0; r < 16; ++r) accc[r] = 0.f;
                chain_f16<false>(Wc1i, lane, pb, accc);               // (Wc1 m) s_m s_wc1
                float bias2[1][16], wc2x[1][16];
                load_tab<1>(bc1t, hh, bias2);
                load_tab<1>(wc2t, hh, wc2x);
                const float kc = inv_sm * inv_swc1;
                float q[16], dq[16];
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    if constexpr (PAIR) {
                        const pvs_f2 zc = pvs_fma2(pvs_f2{accc[r], accc[r + 1]}, pvs_f2{kc, kc}, pvs_f2{bias2[0][r], bias2[0][r + 1]});
                        pvs_f2 qv, dv;
                        pvs_silu_grad2(zc, qv, dv);
                        q[r] = qv.x; q[r + 1] = qv.y;
                        dq[r] = dv.x; dq[r + 1] = dv.y;
                    } else {
                        for (int t = r; t < r + 2; ++t) {
                            const float zc = fmaf(accc[t], kc, bias2[0][t]);   // zc = Wc1 m + bc1
                            const float sg = pvs_sigmoid(zc);
                            q[t] = zc * sg;
                            dq[t] = fmaf(q[t], 1.0f - sg, sg);
                        }
                    }
                    // (one running sum: a pair of partial sums, or a wave-uniform fast path for full tiles behind the
                    // chain, each cost this instantiation 3-5 spilled registers)
                    s = fmaf(wc2x[0][r], q[r], s);
                    s = fmaf(wc2x[0][r + 1], q[r + 1], s);
                }
                s = pvs_xor32_sum(s);
                float dact = 1.f;
                if (flags & PVS_TANH) { s = pvs_tanh(s); dact = 1.f - s * s; }
                if (flags & PVS_NORMALIZE) nrm = 1.f / (sqrtf(rho) + 1e-8f);
                s_coord = s;
                // (the general kernels keep the expression they were compiled from - written out, their code changes,
                // though not their arithmetic -; the first-layer form takes their order from dot3_f16)
                const float g_dot = GX ? d0 * gT0 + d1 * gT1 + d2 * gT2 : dot3_f16(d0, d1, d2, gT0, gT1, gT2);
                const float g_s = g_dot * nrm * dact * vm;
                float g_zc[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    g_zc[r] = g_s * wc2x[0][r] * dq[r];
                    g_wc2x[r] = fmaf(g_s, q[r], g_wc2x[r]);
                }
                float inv_sg;
                const float sg_ = LAZY ? lazy_scale(g_zc, kXg, &inv_sg) : pvs_tile_scale(g_zc, &inv_sg);
                split_f16x2<PAIR>(g_zc, sg_, pb);
                write_image_f16(GI, j, hh, pb);
                f32x16 accg;
#pragma unroll
                for (int r = 0; r < 16; ++r) accg[r] = 0.f;
                chain_f16<true>(Wc1i, lane, pb, accg);                // (Wc1^T g_zc) s_g s_wc1
                const float kg = inv_sg * inv_swc1;
#pragma unroll
                for (int r = 0; r < 16; ++r) gm[r] = accg[r] * kg;
                pvs_wave_lds_sync();                                  // the m and g_zc images are complete
                // gWc1 += g_zc (x) m ; g_bc1 += sum_e g_zc
                if constexpr (LAZY) {
                    const int what = pvs_rescale_acc(gWc1, gB, j == 0, u_wc1, u_bc1, lazy_e(kXg), lazy_e(kXm));
                    // (an operand whose product is not to be added is read from the all-zero image instead: the product
                    // itself is never inside a branch, so that its MFMAs can be scheduled among the vector work behind it)
                    wgrad_tile_f16_acc(GI, (what & 1) ? MI : ZI, (what & 2) ? ones0 : reinterpret_cast<unsigned*>(ZI), lane, gWc1, gB);
                } else {
                    wgrad_tile_f16(GI, MI, ones0, lane, inv_sg * inv_sm, inv_sg, gWc1, gB);
                }
                load_row_terms();
            } else {
                load_row_terms();
            }
            add_row_terms();
            // ---- edge residual; g_z2 = g_m_new * SiLU'(z2) ----
            float g_z2[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float gmv = gm[r];
                float gnew = gmv;
                if constexpr (ERK == 1) mp[0][r] = gmv;      // (plain sum: m_prev receives g_m as it is)
                if constexpr (ERK == 2) {           // rezero: m = m_prev + g m_new
                    gnew = gate * gmv;
                    g_gate = fmaf(gmv, m_new[r], g_gate);
                    mp[0][r] = gmv;
                }
                if constexpr (ERK == 3) {           // gated: m = relu(g) m_new + (1 - relu(g)) m_prev
                    gnew = gate * gmv;
                    if (gate_raw > 0.f) g_gate = fmaf(gmv, m_new[r] - mp[0][r], g_gate);
                    mp[0][r] = (1.f - gate) * gmv;
                }
                g_z2[r] = gnew * dz2[r];
            }
            if constexpr (ERES) {
                if (valid) store_x<1>(io.g_m_prev + (size_t)e * H, hh, mp);
            }
            // ---- g_a1 = W2^T g_z2 ; gW2 += g_z2 (x) a1 ; g_b2 += sum_e g_z2 ; g_z1 = g_a1 * SiLU'(z1) ----
            float inv_sg2;
            const float sg2 = LAZY ? lazy_scale(g_z2, kXg2, &inv_sg2) : pvs_tile_scale(g_z2, &inv_sg2);
            split_f16x2<PAIR>(g_z2, sg2, pb);
            pvs_wave_lds_sync();                                      // the g_zc image has been read
            write_image_f16(GI, j, hh, pb);
            f32x16 ga1;
#pragma unroll
            for (int r = 0; r < 16; ++r) ga1[r] = 0.f;
            chain_f16<true>(W2i, lane, pb, ga1);
            pvs_wave_lds_sync();                                      // the a1 and g_z2 images are complete
            if constexpr (LAZY) {
                const int what = pvs_rescale_acc(gW2, gB, j == 1, u_w2, u_b2, lazy_e(kXg2), lazy_e(kXa1));
                wgrad_tile_f16_acc(GI, (what & 1) ? A1I : ZI, (what & 2) ? ones1 : reinterpret_cast<unsigned*>(ZI), lane, gW2, gB);
            } else {
                wgrad_tile_f16(GI, A1I, ones1, lane, inv_sg2 * inv_sa1, inv_sg2, gW2, gB);
            }
            float g_z1[1][16];
            const float k1g = inv_sg2 * inv_sw2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 dd = *reinterpret_cast<const float4*>(d1b + (gq * 64 + lane) * 4);
                g_z1[0][4 * gq] = ga1[4 * gq] * (dd.x * k1g);
                g_z1[0][4 * gq + 1] = ga1[4 * gq + 1] * (dd.y * k1g);
                g_z1[0][4 * gq + 2] = ga1[4 * gq + 2] * (dd.z * k1g);
                g_z1[0][4 * gq + 3] = ga1[4 * gq + 3] * (dd.w * k1g);
            }
            if constexpr (GX) {
                const float g_rho = dot_tab<1>(wrhot, hh, g_z1);
                const float k1 = s_coord * nrm * vm;
                const float gd0 = fmaf(k1, gT0, 2.f * d0 * g_rho);
                const float gd1 = fmaf(k1, gT1, 2.f * d1 * g_rho);
                const float gd2 = fmaf(k1, gT2, 2.f * d2 * g_rho);
                pvs_wave_lds_sync();      // every read of the m / gradient images (their slots become the g_z1 tile) is done
                // per edge: grad wrt (x_row - x_col) and rho, 16 B, for the node gather kernel
                if (hh == 0) {
                    *reinterpret_cast<float4*>(tx + j * 4) = make_float4(gd0, gd1, gd2, 0.f);
                    rowbuf[j] = i;
                    if (valid) {
                        float* gd_at = io.gd + (size_t)e * 4;
                        pvs_store_nt(gd_at, make_float4(gd0, gd1, gd2, pvs_pack_rho_type(rho, ty)));
                    }
                }
            } else {
                pvs_wave_lds_sync();      // (as above)
                // per edge: rho | type alone, 4 B, for the weight sums of the first-layer gather (k_node_gather_rho)
                if (hh == 0) {
                    rowbuf[j] = i;
                    if (valid) __builtin_nontemporal_store(pvs_pack_rho_type(rho, ty), io.gd + e);
                }
            }
            // ---- g_z1 edge-major, then whole rows to HBM + the row-side sums from the same reads ----
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *reinterpret_cast<float4*>(T1 + (TSWZ ? pvs_tile_quad_off<1>(j, 2 * gq + hh) : j * Cfg::kTS + 8 * gq + 4 * hh)) =
                    make_float4(g_z1[0][4 * gq], g_z1[0][4 * gq + 1], g_z1[0][4 * gq + 2], g_z1[0][4 * gq + 3]);
            pvs_wave_lds_sync();
            reduce_rows_tile<1, false, true, TSWZ, GX>(T1, tx, rowbuf, bmask, lane, acc, accx, cur_row, flush,
                                [&](int rl, int q, const float4& v) {
                                    if (e0 + rl < e_this_end) {  // streamed once: non-temporal
                                        float* at = io.gz1 + (size_t)(e0 + rl) * H + 4 * q;
                                        pvs_store_nt(at, v);
                                    }
                                });
            I = In;
            e0 = e_this_end;
            t_end = n_end;
            pvs_wave_lds_sync();
        }
        flush(cur_row);
    }

    // ---- block reduction into one slab, fixed order ----
    const PvsSlabLayout L = pvs_slab_layout(H);
    __syncthreads();
    float* slab = smem;
    for (int i = threadIdx.x; i < L.total; i += NT) slab[i] = 0.f;
    if constexpr (LAZY) {       // the accumulators back to true values: an exact power of two each (in two factors:
        // 1 / (s_G s_Act) = 2^(units - 280), units = the sum of two exponents in [17, 254], need not be a normal float)
        auto pw = [](int u, int n) { return u < 0 ? 1.f : __uint_as_float((unsigned)(n ? u - u / 2 - 13 : u / 2 - 13) << 23); };
        const float a2 = pw(u_w2.cur(), 0), b2 = pw(u_w2.cur(), 1), ac = pw(u_wc1.cur(), 0), bc = pw(u_wc1.cur(), 1);
        const float kb2 = u_b2.cur() < 0 ? 1.f : __uint_as_float((unsigned)(u_b2.cur() - 13) << 23);
        const float kbc = u_bc1.cur() < 0 ? 1.f : __uint_as_float((unsigned)(u_bc1.cur() - 13) << 23);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            gW2[r] = gW2[r] * a2 * b2;
            gWc1[r] = gWc1[r] * ac * bc;
            gB[r] *= j == 0 ? kbc : (j == 1 ? kb2 : 1.f);
        }
    }
    __syncthreads();
    // X-layout vectors: sum over the 32 edge lanes of each half
    auto lanes32 = [](float v) {
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) g_wc2x[r] = lanes32(g_wc2x[r]);
    float g_wax[EATT ? 16 : 1];
    if constexpr (EATT) {
#pragma unroll
        for (int r = 0; r < 16; ++r) g_wax[r] = lanes32(j >= 2 ? gB[r] : 0.f);      // columns 2..31 of gB
    }
    g_ba += __shfl_xor(g_ba, 32, 64);          // only hh == 0 lanes accumulated
    g_ba = lanes32(g_ba);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) g_gate += __shfl_xor(g_gate, o, 64);
    for (int turn = 0; turn < NW; ++turn) {
        if (wv == turn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = xch(r, hh), k = j;
                slab[L.w2 + c * H + k] += gW2[r];
                slab[L.wc1 + c * H + k] += gWc1[r];
            }
            if (j == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = xch(r, hh);
                    slab[L.wc2 + c] += g_wc2x[r];
                    if constexpr (EATT) slab[L.wa + c] += g_wax[r];
                }
            }
            if (j <= 1) {      // bias gradients: column 0 of gB is g_bc1, column 1 is g_b2
#pragma unroll
                for (int r = 0; r < 16; ++r) slab[(j == 0 ? L.bc1 : L.b2) + xch(r, hh)] += gB[r];
            }
            if (lane == 0) { slab[L.ba] += g_ba; slab[L.gate] += g_gate; }
        }
        __syncthreads();
    }
    float* dst = io.slabs + (size_t)blockIdx.x * L.total;
    for (int i = threadIdx.x; i < L.total; i += NT) dst[i] = slab[i];
