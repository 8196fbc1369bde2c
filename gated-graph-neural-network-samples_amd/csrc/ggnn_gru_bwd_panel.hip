// Backward of the GRU node update for LARGE hidden sizes (D = 128, 192, 256) as ONE launch on COLUMN PANELS -- what
// ggnn_gru_bwd_fused.hip computes for D = 32 / 64 / 100 (its header states the formulas), in the geometry of the forward panel GRU
// (ggnn_panel.hip): a transposed D x D weight block does not fit the LDS, so a stage multiplies a wave's 16 x D fragment by ONE
// 64-column panel of one transposed block, and the panel images come through the same two-slot LDS-DMA ring (whole 64 KiB images
// in f32 form; PanelGruSplitCfg::PARTS parts of a chunk-major three-plane bf16 image in split form).
//
//     dpc = g (1-u) act'(c)        dpu = g (h-c) u (1-u)        r*h,  g u                       (element-wise head)
//     drh = dpc Wc^T[h rows]       dpr = drh h r (1-r)
//     dh  = g u + drh r + dpr Wg_r^T[h rows] + dpu Wg_u^T[h rows]
//     dx_s = dpc Wc^T[x_s rows] + dpr Wg_r^T[x_s rows] + dpu Wg_u^T[x_s rows]                    s = 0 .. nx-1
//
// dpr is element-wise in drh, but every later product sums over ALL D columns of dpr, so a pass over a wave's 16 rows has two
// phases: first all NP panels of the h block of Wc^T (-> drh, complete; then dpr), after that the output blocks (dh, dx_0 ..), each
// the sum of three products per output panel.  A block is worked OPERAND by operand -- dpc x its NP panels, dpr x its NP panels,
// dpu x its NP panels -- into NP x 4 accumulator tiles, so only ONE operand fragment is resident: it is split once into bf16 planes
// for its NP stages (split form), and the next operand is re-read from memory under the last of them.  dpc and dpg = [dpr | dpu]
// are outputs anyway (the weight-gradient products read them), so the re-reads are reads of what the same lane has stored --
// output tile nt of a stage IS activation chunk nt (same lane, same columns), the property every chained kernel here rests on.
// g u takes the same way: the head stores it into dh, the drh epilogue turns it into g u + drh r there, and the two dh products,
// accumulated from zero, are added to that at the end (one rounding at the magnitude of g u instead of one per MFMA).
// Every store a lane reads back is separated from the read by at least one stage barrier with a full vector-memory wait.
//
// Stage (= image) order of a pass, 3 (nx + 1) NP images:
//     h block:      Wc^T panels 0..NP-1 | Wg_r^T panels | Wg_u^T panels          then the same three groups for x_0, x_1, ..
// Registers per wave at D = 256, split form: planes 96 + fragment 64 + accumulators 64 + weight operands 12.
#include "ggnn_panel.hpp"
#include "ggnn_gru_bwd.hpp"

namespace ggnn {

// image order: panel_gru_bwd_image_src (ggnn_panel.hpp)
template <int D, bool SPLIT>
__global__ void gru_bwd_panel_pack_kernel(const float* __restrict__ Wg, const float* __restrict__ Wc, int nx, float* __restrict__ out) {
    using C = PanelCfg<D>;
    const int i = blockIdx.y;
    const PanelSrc<true> src = panel_gru_bwd_image_src<D>(Wg, Wc, nx, i);
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if constexpr (SPLIT) pack_panel_gru_split_image_fn<D, kSplitBf16x3>(src, out + (size_t)i * PanelGruSplitCfg<D>::IMG, first, stride);
    else pack_panel_image_fn<D>(src, out + (size_t)i * C::IMG, first, stride);
}

// fragment of rows of a [V, ld] array at column offset c0 (dpu: the second half of dpg's rows)
template <int D>
__device__ __forceinline__ void load_frag_at(Frag<D>& f, const float* base, int row, int ld, int c0, int kq) {
    const unsigned ob = ((unsigned)row * (unsigned)ld + (unsigned)c0 + 4u * (unsigned)kq) * 4u;
    __builtin_assume(ob < 0xF0000000u);
#pragma unroll
    for (int c = 0; c < PanelCfg<D>::NC; ++c) f.v[c] = ld4_b(base, ob + 64u * c);
}

template <int D, int NW, bool SPLIT>
__global__ __launch_bounds__(NW * 64) void ggnn_gru_bwd_panel_kernel(GruBwdArgs a, const float* __restrict__ packed) {
    using C = PanelCfg<D>;
    using SC = PanelGruSplitCfg<D>;
    constexpr int IMGF = SPLIT ? SC::IMG : C::IMG;                   // floats per image in `packed`
    constexpr int SLOTF = SPLIT ? SC::PART : C::IMG;                 // floats per ring slot
    constexpr int PARTS = SPLIT ? SC::PARTS : 1;
    constexpr int NP = C::NP, NC = C::NC;
    static_assert(NP >= 2 && NP <= 4, "stage macros cover 2..4 panels");
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];    // [2][SLOTF]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int nstage = 3 * (a.nx + 1) * NP;

    const int nb = gridDim.x;
    const PanelTickets<NW> tickets(a.V, nb);
    const int n_tk = tickets.n_tk;
    PanelRing<SPLIT ? SC::PART_BYTES : C::IMG_BYTES, NW, SPLIT> ring{ring_lds, wave, lane};
    ring.fill_first(packed);
    ring.first_ready();

    for (int tk = blockIdx.x; tk < n_tk; tk += nb) {
        const int tile = tickets.tile_of(tk, wave);
        const bool active = tile >= 0;                                  // wave-uniform
        const bool last_pass = tk + nb >= n_tk;

        // The pass body exists twice, like the forward kernel's: for a wave WITH a tile, and for a wave without one (thin tail
        // tickets), which only takes part in the image DMA and the barriers.
        auto run_pass = [&](auto active_c) {
            constexpr bool ACT = decltype(active_c)::value;
            const int row = (ACT ? tile : 0) * 16 + li;
            const bool row_ok = ACT && row < a.V;
            const int rc = row < a.V ? row : a.V - 1;                   // (always a valid row to read)

            u32x4 qh[SPLIT ? SC::NC2 : 1], qm[SPLIT ? SC::NC2 : 1], ql[SPLIT ? SC::NC2 : 1];   // resident planes of the operand fragment
            // one stage: PARTS rounds on one image; `after` = this wave's loads for the NEXT group of stages
            auto stage = [&](auto zero_c, f32x4 (&acc)[4], const Frag<D>& A, int img_idx, auto&& after) {
                const int nidx = img_idx + 1 < nstage ? img_idx + 1 : 0;
                const bool more = (img_idx + 1 < nstage) || !last_pass;
                panel_for_parts<PARTS>([&](auto part_c) {
                    constexpr int part = decltype(part_c)::value;
                    panel_round<part, PARTS, ACT, false>(ring, part + 1 < PARTS || more,
                                                         panel_next_part<PARTS, IMGF, SLOTF>(packed, img_idx, part, nidx), [] {},
                        [&] {
                            if constexpr (SPLIT) panel_part_mma_planes<D, decltype(zero_c)::value && part == 0, part>(acc, qh, qm, ql, ring.slot(), li, kq);
                            else panel_mma<D, decltype(zero_c)::value>(acc, A, ring.slot(), li, kq);
                        }, after);
                });
            };
            auto nothing = [] {};
            // a group: the resident fragment x the NP panels of one transposed block; `after` runs in the last of its stages
            Frag<D> af;
            f32x4 acc[NP][4];
            auto group = [&](auto zero_c, int img0, auto&& after) {
                if constexpr (SPLIT && ACT) frag_to_planes<D>(af, qh, qm, ql);
                stage(zero_c, acc[0], af, img0, nothing);
                if constexpr (NP == 2) stage(zero_c, acc[1], af, img0 + 1, after);
                else {
                    stage(zero_c, acc[1], af, img0 + 1, nothing);
                    if constexpr (NP == 3) stage(zero_c, acc[2], af, img0 + 2, after);
                    else {
                        stage(zero_c, acc[2], af, img0 + 2, nothing);
                        stage(zero_c, acc[NP - 1], af, img0 + 3, after);
                    }
                }
            };
            auto load_dpc = [&] { load_frag_at<D>(af, a.dpc, rc, D, 0, kq); };
            auto load_dpr = [&] { load_frag_at<D>(af, a.dpg, rc, 2 * D, 0, kq); };
            auto load_dpu = [&] { load_frag_at<D>(af, a.dpg, rc, 2 * D, D, kq); };

            // ---- element-wise head, four chunks at a time: dpc -> fragment + store; dpu, r*h, g u -> stores ------------------------
            if constexpr (ACT) {
                int hz0 = -1, hz1 = -1, hz2 = -1, hz3 = -1;
                if (a.gz) {
                    const int4 hd = *reinterpret_cast<const int4*>(a.gz_heads + 4 * (size_t)rc);
                    hz0 = hd.x; hz1 = hd.y; hz2 = hd.z; hz3 = hd.w;
                }
                auto dact = [&](float cv) { return a.act == GGNN_ACT_TANH ? 1.0f - cv * cv : (cv > 0.f ? 1.0f : 0.f); };
                const unsigned ol = ((unsigned)rc * (unsigned)D + 4u * (unsigned)kq) * 4u;          // loads (clamped row)
                const unsigned os = ((unsigned)row * (unsigned)D + 4u * (unsigned)kq) * 4u;         // stores (row_ok only)
                const unsigned og = ((unsigned)row * (unsigned)(2 * D) + (unsigned)D + 4u * (unsigned)kq) * 4u;   // dpu inside dpg
                __builtin_assume(ol < 0xF0000000u);
                __builtin_assume(os < 0xF0000000u);
                __builtin_assume(og < 0xF0000000u);
                auto zoff = [&](int hz) { return ((unsigned)hz * (unsigned)D + 4u * (unsigned)kq) * 4u; };
#pragma unroll
                for (int grp = 0; grp < NC / 4; ++grp) {
                    f32x4 gv[4], uv[4], cv[4], hv[4], rv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned o = ol + 64u * (4 * grp + j);
                        gv[j] = ld4_b(a.g, o); uv[j] = ld4_b(a.u, o); cv[j] = ld4_b(a.c, o); hv[j] = ld4_b(a.h, o); rv[j] = ld4_b(a.r, o);
                    }
                    if (a.gz) {
                        // the sums of ggnn_gather_segment_sum_heads_f32(accumulate = 1), in its order: ((0 + z0) + z1 + z2 + z3) + g
                        f32x4 zs[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            f32x4 z0 = {0.f, 0.f, 0.f, 0.f};
                            if (hz0 >= 0) z0 = ld4_b(a.gz, zoff(hz0) + 64u * (4 * grp + j));
                            zs[j] = 0.f + z0;
                            if (hz1 >= 0) zs[j] = zs[j] + ld4_b(a.gz, zoff(hz1) + 64u * (4 * grp + j));
                        }
                        if (hz2 >= 0) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                zs[j] = zs[j] + ld4_b(a.gz, zoff(hz2) + 64u * (4 * grp + j));
                                if (hz3 >= 0) zs[j] = zs[j] + ld4_b(a.gz, zoff(hz3) + 64u * (4 * grp + j));
                            }
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) gv[j] = zs[j] + gv[j];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cc = 4 * grp + j;
                        const f32x4 omu = 1.0f - uv[j];
                        const f32x4 da = {dact(cv[j].x), dact(cv[j].y), dact(cv[j].z), dact(cv[j].w)};
                        const f32x4 dpc = gv[j] * omu * da;
                        af.v[cc] = dpc;
                        if (row_ok) {
                            st4_b(a.dpc, os + 64u * cc, dpc);
                            st4_b(a.dpg, og + 64u * cc, gv[j] * (hv[j] - cv[j]) * uv[j] * omu);
                            st4_b(a.rh, os + 64u * cc, rv[j] * hv[j]);      // the last segment of the [x | r*h] operand of dWc
                            st4_b(a.dh, os + 64u * cc, gv[j] * uv[j]);      // (read back below)
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);                      // one group's 20 loads in flight, not all 80
                }
            }

            // ---- h block, Wc^T: drh = dpc Wc^T[h rows];  dpr = drh h r (1-r) -> the next operand;  dh = g u + drh r so far -------------
            group(std::true_type{}, 0, nothing);
            if constexpr (ACT) {
                const unsigned ol = ((unsigned)rc * (unsigned)D + 4u * (unsigned)kq) * 4u;
                const unsigned os = ((unsigned)row * (unsigned)D + 4u * (unsigned)kq) * 4u;
                const unsigned og = ((unsigned)row * (unsigned)(2 * D) + 4u * (unsigned)kq) * 4u;
                __builtin_assume(ol < 0xF0000000u);          // (so that the +64 nt below folds into the instruction's immediate)
                __builtin_assume(os < 0xF0000000u);
                __builtin_assume(og < 0xF0000000u);
#pragma unroll
                for (int nt = 0; nt < NC; ++nt) {
                    const f32x4 hv = ld4_b(a.h, ol + 64u * nt), rv = ld4_b(a.r, ol + 64u * nt), gu = ld4_b(a.dh, ol + 64u * nt);
                    const f32x4 drh = acc[nt / 4][nt % 4];
                    const f32x4 dpr = drh * (hv * rv * (1.0f - rv));
                    af.v[nt] = dpr;
                    if (row_ok) st4_b(a.dpg, og + 64u * nt, dpr);
                    // g u + drh r goes back into dh and is added to the two products at the END: as the start value of their
                    // accumulators it would put every one of their 12 D / 32 MFMA roundings at the magnitude of g u
                    if (row_ok) st4_b(a.dh, os + 64u * nt, drh * rv + gu);
                    if (nt % 4 == 3) __builtin_amdgcn_sched_barrier(0);     // a panel's 12 loads in flight, not all 3 NC
                }
            }
            // ---- h block, Wg_r^T and Wg_u^T: dh += dpr Wg_r^T + dpu Wg_u^T ---------------------------------------------------------
            group(std::true_type{}, NP, load_dpu);
            group(std::false_type{}, 2 * NP, load_dpc);
            if constexpr (ACT) {
                if (row_ok) {
                    const unsigned os = ((unsigned)row * (unsigned)D + 4u * (unsigned)kq) * 4u;
                    __builtin_assume(os < 0xF0000000u);
#pragma unroll
                    for (int nt = 0; nt < NC; ++nt) {
                        st4_b(a.dh, os + 64u * nt, ld4_b(a.dh, os + 64u * nt) + acc[nt / 4][nt % 4]);
                        if (nt % 4 == 3) __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            // ---- x segments: dx_s = dpc Wc^T + dpr Wg_r^T + dpu Wg_u^T (run-time loop: the segment only enters addresses) ------------
#pragma unroll 1
            for (int s = 0; s < a.nx; ++s) {
                const int img0 = 3 * NP * (1 + s);
                const bool last_seg = s + 1 == a.nx;
                group(std::true_type{}, img0, load_dpr);
                group(std::false_type{}, img0 + NP, load_dpu);
                group(std::false_type{}, img0 + 2 * NP, [&] { if (!last_seg) load_dpc(); });
                if constexpr (ACT) {
                    if (row_ok) {
                        float* out = s == 0 ? a.dx[0] : (s == 1 ? a.dx[1] : a.dx[2]);
                        const bool avg = last_seg && a.use_avg;
                        float den = 1.0f;
                        if (avg) {
                            float deg = 0.f;
                            for (int t = 0; t < a.T; ++t) deg += a.nin[(size_t)row * a.T + t];
                            den = deg + 1e-7f;
                        }
#pragma unroll
                        for (int nt = 0; nt < NC; ++nt) {
                            f32x4 v = acc[nt / 4][nt % 4];
                            if (avg) v = v / den;
                            st4_b(out, ((unsigned)row * D + nt * 16 + 4 * kq) * 4u, v);
                        }
                    }
                }
            }
        };
        if (active) run_pass(std::true_type{});
        else run_pass(std::false_type{});
    }
}

template <int D, bool SPLIT>
static int launch_gru_bwd_panel(const GruBwdArgs& a, const float* Wg, const float* Wc, float* packed, hipStream_t st) {
    using C = PanelCfg<D>;
    if (Wg) {
        hipLaunchKernelGGL((gru_bwd_panel_pack_kernel<D, SPLIT>), dim3(8, panel_gru_bwd_images(D, a.nx)), dim3(256), 0, st, Wg, Wc, a.nx, packed);
        GGNN_CHECK_HIP(hipGetLastError());
    }
    if (a.g == nullptr || a.V == 0) return GGNN_OK;
    if ((unsigned long long)a.V * 2 * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "fused GRU backward indexes with 32-bit byte offsets: V*2D must be < 2^30 (V=%d, D=%d)", a.V, D);
    const size_t lds = (size_t)2 * (SPLIT ? PanelGruSplitCfg<D>::PART_BYTES : C::IMG_BYTES);
    return panel_launch<&ggnn_gru_bwd_panel_kernel<D, kPanelNW, SPLIT>>(lds, 64 * 1024, panel_blocks(a.V, 1), st, a, (const float*)packed);
}

template <int D>
static int gru_bwd_panel_d(const GruBwdArgs& a, const float* Wg, const float* Wc, float* packed, hipStream_t st) {
    if (a.nx < 1 || a.nx > 3) return fail(GGNN_E_INVALID, "nx %d outside 1..3", a.nx);
    return split_matrix_path() ? launch_gru_bwd_panel<D, true>(a, Wg, Wc, packed, st) : launch_gru_bwd_panel<D, false>(a, Wg, Wc, packed, st);
}

int gru_bwd_panel_supported(int D) { return panel_hidden_ok(D); }

size_t gru_bwd_panel_packed_bytes(int D, int nx) {
    if (!gru_bwd_panel_supported(D)) return 0;
    // a split image is D / 32 chunks of three 4 KiB planes (D x 64 x 6 bytes), an f32 image D x 64 floats: D x D x (6 or 4) per block
    const size_t img = split_matrix_path() ? (size_t)(D / 32) * PanelGruSplitCfg<128>::CHUNK_BYTES : (size_t)D * 64 * sizeof(float);
    return (size_t)panel_gru_bwd_images(D, nx) * img;
}

int gru_bwd_panel_dispatch(int D, const GruBwdArgs& a, const float* Wg, const float* Wc, float* packed, hipStream_t st) {
    if (!panel_hidden_ok(D)) return fail(GGNN_E_UNSUPPORTED, "no panel GRU backward for hidden size %d", D);
    return panel_for_D(D, [&](auto d) { return gru_bwd_panel_d<decltype(d)::value>(a, Wg, Wc, packed, st); });
}

}  // namespace ggnn
