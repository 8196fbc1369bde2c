// Register-chained kernels for LARGE hidden sizes (D a multiple of 64: 128, 192, 256 -- BASELINE config "100k nodes / 1M
// edges, h = 256"): the fused GRU node update (chem_tensorflow_sparse.py:211-216) and the compacted per-edge-type message
// transform (:160-164) on COLUMN PANELS of the weight blocks.
//
// Why panels.  The D = 100 kernels (ggnn_gru_fused.hip, ggnn_msg_compact.hip) keep one D x D weight block as a 48 KiB
// k-interleaved image in LDS and a wave owns 16 rows x ALL D output columns of all three gates.  At D = 256 a block is
// 256 KiB (LDS: 160 KiB per CU) and three gates x 16 column tiles are 192 accumulator registers.  Here a stage multiplies
// the wave's 16 x D activation fragment by ONE 64-column panel of one weight block: the panel image is D x 64 floats
// (64 KiB at D = 256; two of them form the LDS-DMA ring) and a stage's accumulators are 4 tiles = 16 registers.
//
// GRU pass of a wave over its 16 rows (NS = NX + 1 input segments x_0 .. x_{NX-1}, h; NP = D / 64 panels):
//   phase R   for every segment s, every panel p:   acc_r[p] += seg_s x Wg[s rows, r columns of panel p]
//             r = sigmoid(acc_r + bg_r);  rh = r * h   -- in activation-fragment layout (output tile nt == k chunk nt, the
//             property the D = 100 kernel chains on), so r*h feeds the candidate stages from registers
//   phase UC  for every panel p:   u_p = sum_s seg_s x Wg[s, u columns of p],  c_p = sum_s x_s x Wc[s, p] + rh x Wc[h rows, p]
//             u = sigmoid(.), c = act(.), h'[:, panel p] = u h + (1 - u) c   -> stored; nothing but x, h is read and h' written
// Only ONE activation fragment is resident besides r*h: the fragment of the next stage's segment is (re)loaded from
// memory (L2 hits after the first touch) right after the wave's MFMA burst of the current stage, i.e. while the partner
// wave of the SIMD owns the matrix pipe.  Per wave: r*h 64 + fragment 64 + accumulators 32 + weight operands 32 VGPRs.
// Every product chain accumulates its segments in [x_0 | .. | h] order like the plain [x|h] Wg / [x|r*h] Wc products.
//
// The transform is the same stage loop without the chain: a persistent workgroup is bound to ONE (edge type, panel),
// keeps that panel image in LDS and walks 16-row tiles of the type's active (source node, type) pairs.
#include "ggnn_panel.hpp"
#include "ggnn_gru_cells.hpp"
#ifndef GGNN_PANEL_PLANES
#define GGNN_PANEL_PLANES 1        // the panel GRU keeps a fragment's planes resident over the stages that multiply it in a row
#endif
#ifndef GGNN_PANEL_DMA_FIRST
#define GGNN_PANEL_DMA_FIRST 1     // every wave of the panel GRU issues its DMA pieces before its burst (0: the early waves behind theirs,
                                   // the D = 100 kernels' rule): a part issued behind a burst lands late in the round -- 497 -> 485-487 us at D = 256
#endif
#include <type_traits>

namespace ggnn {

// acc[0..3] (+)= fragment x split panel image.  The fragment stays f32; the 8 values of a 32-chunk are split right before the
// chunk's 24 MFMAs (the next chunk's while the current one multiplies); weight planes rotate through 12 registers (stage_mma_split).
template <int D, bool ZERO>
__device__ __forceinline__ void panel_mma_split(f32x4 (&acc)[4], const Frag<D>& a, const float* img, int li, int kq) {
    using C = PanelSplitCfg<D>;
    constexpr int NU = C::NC2 * 4;
    constexpr int PL = C::PLANE_BYTES / 16;
    const u32x4* base = reinterpret_cast<const u32x4*>(img) + kq * 64 + li;
    auto slot = [&](int u, int p) { return base[p * PL + (u / 4) * 4 * 64 + (u % 4) * 16]; };
    auto planes = [&](int c2, u32x4& hi, u32x4& mid, u32x4& lo) {
        const f32x4 x = a.v[2 * c2], y = a.v[2 * c2 + 1];
        unsigned h[4], m[4], l[4];
        split_pair(x.x, x.y, h[0], m[0], l[0]); split_pair(x.z, x.w, h[1], m[1], l[1]);
        split_pair(y.x, y.y, h[2], m[2], l[2]); split_pair(y.z, y.w, h[3], m[3], l[3]);
        hi = u32x4{h[0], h[1], h[2], h[3]}; mid = u32x4{m[0], m[1], m[2], m[3]}; lo = u32x4{l[0], l[1], l[2], l[3]};
    };
    u32x4 ah, am, al, nh, nm, nl;
    planes(0, ah, am, al);
    u32x4 wh = slot(0, 0), wm = slot(0, 1), wl = slot(0, 2);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int c2 = u / 4, j = u % 4;
        const bool more = u + 1 < NU;
        if (j == 0 && c2 + 1 < C::NC2) planes(c2 + 1, nh, nm, nl);      // (vector work of the next chunk, under this chunk's MFMAs)
        f32x4 c = (ZERO && c2 == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
        c = mfma_bf16(wl, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wl = slot(u + 1, 2);
        c = mfma_bf16(wm, am, c);
        c = mfma_bf16(wm, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wm = slot(u + 1, 1);
        c = mfma_bf16(wh, al, c);
        c = mfma_bf16(wh, am, c);
        c = mfma_bf16(wh, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wh = slot(u + 1, 0);
        acc[j] = c;
        if (j == 3) { ah = nh; am = nm; al = nl; }
    }
}


// The same product with the panel image read straight from GLOBAL memory (L2-resident) instead of LDS, three chunks of
// read-ahead: the cooperative tail pass, where every wave multiplies by a DIFFERENT panel at the same time (the ring holds one
// image per stage).  Same k order per output element as panel_mma.
template <int D, bool ZERO>
__device__ __forceinline__ void panel_mma_global(f32x4 (&acc)[4], const Frag<D>& a, const float* __restrict__ gimg, int li, int kq) {
    using C = PanelCfg<D>;
    // wave-uniform image base in scalar registers + ONE 32-bit per-lane byte offset; the chunk advances the scalar base and the
    // tile is an instruction immediate (per-lane 64-bit addresses for the 64 loads of a stage get hoisted out of the pass loop
    // by the compiler -- hundreds of register pairs, i.e. kilobytes of scratch)
    const unsigned long long gb = reinterpret_cast<unsigned long long>(gimg);
    const unsigned glo = __builtin_amdgcn_readfirstlane((unsigned)gb), ghi = __builtin_amdgcn_readfirstlane((unsigned)(gb >> 32));
    const float* sbase = reinterpret_cast<const float*>(((unsigned long long)ghi << 32) | glo);
    const unsigned voff = (unsigned)(kq * C::BN + li) * 16u;
    auto chunk = [&](int c, int j) { return ld4_b(sbase + (size_t)c * 4 * C::BN * 4, voff + 256u * j); };
    constexpr int AHEAD = 3;
    f32x4 w[AHEAD + 1][4];
#pragma unroll
    for (int c = 0; c < AHEAD && c < C::NC; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) w[c][j] = chunk(c, j);
#pragma unroll
    for (int c = 0; c < C::NC; ++c) {
        if (c + AHEAD < C::NC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[(c + AHEAD) % (AHEAD + 1)][j] = chunk(c + AHEAD, j);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 cin = (ZERO && c == 0 && e == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c % (AHEAD + 1)][j][e], a.v[c][e], cin, 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- packed GRU weights: one image per stage, in stage order (panel_gru_fwd_image_src, ggnn_panel.hpp) -------------------------------
template <int D, bool SPLIT, int FMT = kSplitBf16x3>
__global__ void gru_panel_pack_kernel(const float* __restrict__ Wg, const float* __restrict__ Wc, int nx, float* __restrict__ out) {
    using C = PanelCfg<D>;
    const int i = blockIdx.y;
    const PanelSrc<false> src = panel_gru_fwd_image_src<D>(Wg, Wc, nx, i);
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if constexpr (SPLIT) pack_panel_gru_split_image_fn<D, FMT>(src, out + (size_t)i * PanelGruSplitCfg<D, FMT>::IMG, first, stride);
    else pack_panel_image_fn<D>(src, out + (size_t)i * C::IMG, first, stride);
}

// SPLIT: the products on the bf16 pipe in 3-way split form; an image comes through the ring in PanelGruSplitCfg::PARTS parts.
// FMT (SPLIT): operand format of the products and images (ggnn_split.hpp), per launch (GruFusedArgs::fmt): kSplitF16x2 (two f16
// pieces, three products, whole 64 KiB images through the ring; the caller's proven operand range) or the exact kSplitBf16x3.
template <int FMT>
__device__ __forceinline__ f32x4 panel_sigmoid4(f32x4 z, f32x4 b_scaled) {      // (sigmoid4_scaled on an accumulator of 1 / acc_scale x the sum)
    constexpr float k = -kLog2e * SplitFmt<FMT>::acc_scale;
    return rcp_4(exp2_4(z * k + b_scaled) + 1.0f);
}
template <int FMT>
__device__ __forceinline__ f32x4 panel_tanh4(f32x4 z, f32x4 b_scaled) {
    constexpr float k = 2.0f * kLog2e * SplitFmt<FMT>::acc_scale;
    return 1.0f - 2.0f * rcp_4(exp2_4(z * k + b_scaled) + 1.0f);
}

// h'[:, panel p] = u h + (1 - u) c for the lane's row (< V) from the panel's u and candidate accumulators; bias_s: the kernel's
// scaled biases [-log2e*bg (2D) | 2 log2e*bc (D) | bc (D)].  The h columns of the panel are fetched here and not a stage ahead: 16
// more live registers across the r*h stage; the ~0.5k clocks of L2 latency per 65k-clock panel are covered by the partner wave.
// H_FIRST (the ring passes): all four h quads in flight before the arithmetic; else (the cooperative tail, whose products hold more
// registers) one quad per tile.
template <int D, int FMT, bool SAVE, bool H_FIRST>
__device__ __forceinline__ void gru_panel_epilogue(const GruFusedArgs& a, const float* bias_s, const f32x4 (&acc_u)[4],
                                                   const f32x4 (&acc_c)[4], int row, int p, int kq) {
    f32x4 hcol[4];
    if constexpr (H_FIRST) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) hcol[nt] = ld4_b(a.h, ((unsigned)row * D + p * 64 + nt * 16 + 4 * kq) * 4u);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = p * 64 + nt * 16 + 4 * kq;
        if constexpr (!H_FIRST) hcol[nt] = ld4_b(a.h, ((unsigned)row * D + col) * 4u);
        const f32x4 u = panel_sigmoid4<FMT>(acc_u[nt], ld4(bias_s + D + col));
        f32x4 c;
        if (a.act == GGNN_ACT_TANH) {
            c = panel_tanh4<FMT>(acc_c[nt], ld4(bias_s + 2 * D + col));
        } else {
            c = acc_c[nt] * SplitFmt<FMT>::acc_scale + ld4(bias_s + 3 * D + col);
            c.x = fmaxf(c.x, 0.f); c.y = fmaxf(c.y, 0.f); c.z = fmaxf(c.z, 0.f); c.w = fmaxf(c.w, 0.f);
        }
        st4_b(a.h_out, ((unsigned)row * D + col) * 4u, u * hcol[nt] + (1.0f - u) * c);
        if constexpr (SAVE) {
            st4_b(a.save_u, ((unsigned)row * D + col) * 4u, u);
            st4_b(a.save_c, ((unsigned)row * D + col) * 4u, c);
        }
    }
}

template <int D, int NX, int NW, bool SAVE, bool SPLIT, int FMT = kSplitBf16x3>
__global__ __launch_bounds__(NW * 64) void ggnn_gru_panel_kernel(GruFusedArgs a, const float* __restrict__ packed) {
    static_assert(SPLIT || FMT == kSplitBf16x3, "the f32-MFMA kernels have no operand format");
    using C = PanelCfg<D>;
    using SC = PanelGruSplitCfg<D, FMT>;
    constexpr int IMGF = SPLIT ? SC::IMG : C::IMG;                   // floats per image in `packed`
    constexpr int SLOTF = SPLIT ? SC::PART : C::IMG;                 // floats per ring slot
    constexpr int PARTS = SPLIT ? SC::PARTS : 1;
    constexpr int NP = C::NP, NC = C::NC, NS = NX + 1;
    constexpr int NSTAGE = 3 * NS * NP;
    constexpr int R_STAGES = NS * NP;
    extern __shared__ __attribute__((aligned(16))) float lds_[];    // [biases | ring [2][IMG]]
    constexpr int BIAS_FLOATS = (4 * D + 63) / 64 * 64;
    float* bias_s = lds_;                      // [-log2e*bg (2D) | 2 log2e*bc (D) | bc (D)]
    float* ring_lds = lds_ + BIAS_FLOATS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const bool late = wave >= NW / 2;          // (the two waves of a SIMD: w and w + NW/2; see ggnn_gru_fused.hip)

    for (int i = tid; i < 4 * D; i += NW * 64)
        bias_s[i] = i < 2 * D ? -kLog2e * a.bg[i] : (i < 3 * D ? 2.0f * kLog2e * a.bc[i - 2 * D] : a.bc[i - 3 * D]);

    const int nb = gridDim.x;
    const PanelTickets<NW> tickets(a.V, nb);
    const int full_tk = tickets.full_tk, n_tk = tickets.n_tk;
    // One-tile tail tickets (tail_w == 1, the usual case) are worked COOPERATIVELY: wave p < NP takes panel p of the tile (phase R
    // for its 64 columns, r*h exchanged through LDS, then phase UC for its panel), weights straight from the images in L2 --
    // 3 NS stages on each of NP waves instead of 3 NS NP stages on one wave while seven idle.
    const bool coop_tail = (tickets.tail_w == 1) && (NP <= NW);
    const int n_main = coop_tail ? full_tk : n_tk;              // tickets [n_main, n_tk) are cooperative tail passes
    auto tile_of = [&](int t) -> int { return tickets.tile_of(t, wave, coop_tail); };
    auto row_of = [&](int t) -> int {          // clamped row of this lane in ticket t (always a valid row to read)
        const int tile = tile_of(t);
        const int r = (tile >= 0 ? tile : 0) * 16 + li;
        return r < a.V ? r : a.V - 1;
    };

    // The ring cursor, the round and the part ladder are PanelRing's, panel_round's and panel_for_parts' (ggnn_panel.hpp) written out:
    // on the shared forms the three D = 256 SAVE bf16x3 instantiations go from 252-253 to 256 registers and 24-28 B of scratch per lane.
    int cur = 0;
    auto dma = [&](const float* src, float* dst) {
        if constexpr (SPLIT) dma_image_asm<SC::PART_BYTES, NW>(src, dst, wave, lane);
        else dma_block<C::IMG_BYTES, NW>(src, dst, wave, lane);
    };
    auto publish = [&]() { if constexpr (SPLIT) dma_wait(); __syncthreads(); };
    dma(packed, ring_lds);
    Frag<D> af;                                // the ONE resident activation fragment (segment of the current stage)
    int tk = blockIdx.x;
    if (tk < n_main) load_frag<D>(af, a.x[0], row_of(tk), kq);
    publish();

    for (; tk < n_main; tk += nb) {
        const int tile = tile_of(tk);
        const bool active = tile >= 0;                                  // wave-uniform
        const int row = active ? tile * 16 + li : a.V;                  // (>= V: nothing is stored)
        const int rowc = row < a.V ? row : a.V - 1;
        const bool last_pass = tk + nb >= n_main;             // (of the passes that use the ring)
        const int rown = last_pass ? 0 : row_of(tk + nb);

        // The pass body exists twice: for a wave WITH a tile, and for a wave without one (thin tail tickets), which only takes
        // part in the image DMA and the barriers.  (One body with `if (active)` around every MFMA block turns each stage into
        // a diamond whose accumulator phis the register allocator does not coalesce: 296 instead of 230 registers at D = 256.)
        auto run_pass = [&](auto active_c) {
            constexpr bool ACT = decltype(active_c)::value;
            // one stage: PARTS rounds of [late waves, or all with GGNN_PANEL_DMA_FIRST: DMA of the next part] MFMAs [early waves: DMA];
            // then `after()` (this wave's loads for the NEXT stage: they fly while the partner wave multiplies) and the barrier
            // Resident planes of the fragment the next stages multiply (GGNN_PANEL_PLANES, split form): phase R multiplies a segment's
            // fragment by NP panels in a row, phase UC multiplies an x segment's by its u and candidate panels back to back -- the
            // fragment is split ONCE for such a run (10 of the 24 splits of an NX = 1 pass go) and its f32 registers are free for
            // the next fragment's loads; stages that multiply a fragment once (h -> u, r*h -> c) split chunk by chunk as before.
            constexpr bool PLANES = SPLIT && GGNN_PANEL_PLANES;
            u32x4 qh[PLANES ? SC::NC2 : 1], qm[PLANES ? SC::NC2 : 1], ql[PLANES ? SC::NC2 : 1];
            auto make_planes = [&](const Frag<D>& A) { if constexpr (PLANES && ACT) frag_to_planes<D, FMT>(A, qh, qm, ql); };
            auto stage = [&](auto zero_c, f32x4 (&acc)[4], const Frag<D>& A, int img_idx, auto&& after, auto planes_c) {
                constexpr bool USEP = PLANES && decltype(planes_c)::value;
                const int nidx = img_idx + 1 < NSTAGE ? img_idx + 1 : 0;
                const bool more = (img_idx + 1 < NSTAGE) || !last_pass;
                auto round = [&](auto part_c) {
                    constexpr int part = decltype(part_c)::value;
                    constexpr bool ZERO = decltype(zero_c)::value && part == 0;
                    const bool more_p = part + 1 < PARTS || more;
                    const float* nsrc = panel_next_part<PARTS, IMGF, SLOTF>(packed, img_idx, part, nidx);
                    const bool dma_first = late || GGNN_PANEL_DMA_FIRST;
                    if (dma_first && more_p) dma(nsrc, ring_lds + (cur ^ 1) * SLOTF);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (ACT) {
                        if constexpr (USEP) panel_part_mma_planes<D, ZERO, part, FMT>(acc, qh, qm, ql, ring_lds + cur * SLOTF, li, kq);
                        else if constexpr (SPLIT) panel_part_mma_split<D, ZERO, false, part, FMT>(acc, A, ring_lds + cur * SLOTF, li, kq);
                        else panel_mma<D, decltype(zero_c)::value>(acc, A, ring_lds + cur * SLOTF, li, kq);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (!dma_first && more_p) dma(nsrc, ring_lds + (cur ^ 1) * SLOTF);
                    if constexpr (ACT) { if constexpr (part == PARTS - 1) after(); }
                    publish();
                    cur ^= 1;
                };
                round(std::integral_constant<int, 0>{});
                if constexpr (PARTS > 1) round(std::integral_constant<int, 1>{});
                if constexpr (PARTS > 2) round(std::integral_constant<int, 2>{});
            };
            auto nothing = [] {};

            // ---- phase R: r columns, all panels, segment by segment ---------------------------------------------------
            f32x4 acc_r[NP][4];
#define GGNN_R_STAGE(S, P)                                                                                          \
            if constexpr ((S) < NS && (P) < NP) {                                                                   \
                auto next_seg = [&] {   /* after the last panel of a segment: fetch the next segment's fragment */   \
                    if constexpr ((P) == NP - 1 && (S) + 1 < NS)                                                     \
                        load_frag<D>(af, (S) + 1 < NX ? a.x[(S) + 1 < NX ? (S) + 1 : 0] : a.h, rowc, kq);          \
                };                                                                                                  \
                if constexpr ((P) == 0) make_planes(af);                                                            \
                stage(std::integral_constant<bool, (S) == 0>{}, acc_r[(P) < NP ? (P) : 0], af, (S) * NP + (P), next_seg, std::true_type{}); \
            }
#define GGNN_R_SEG(S) GGNN_R_STAGE(S, 0) GGNN_R_STAGE(S, 1) GGNN_R_STAGE(S, 2) GGNN_R_STAGE(S, 3)
            GGNN_R_SEG(0) GGNN_R_SEG(1) GGNN_R_SEG(2) GGNN_R_SEG(3)
#undef GGNN_R_SEG
#undef GGNN_R_STAGE
            static_assert(NP <= 4 && NS <= 4, "stage macros cover up to 4 panels x 4 segments");

            // ---- r = sigmoid(.), rh = r * h in activation-fragment layout (af holds h here) ---------------------------------
            Frag<D> rh;
            if constexpr (ACT) {
#pragma unroll
                for (int nt = 0; nt < NC; ++nt) {
                    const int col = nt * 16 + 4 * kq;
                    const f32x4 r = panel_sigmoid4<FMT>(acc_r[nt / 4][nt % 4], ld4(bias_s + col));
                    if constexpr (SAVE) { if (row < a.V) st4_b(a.save_r, ((unsigned)row * D + col) * 4u, r); }
                    rh.v[nt] = r * af.v[nt];
                    __builtin_amdgcn_sched_barrier(0);      // one tile at a time: no 16-deep batch of bias reads in flight
                }
                load_frag<D>(af, a.x[0], rowc, kq);                     // first fragment of phase UC
            }

            // ---- phase UC: u and candidate columns, panel by panel (run-time loop: the panel only enters addresses) ----------
#pragma unroll 1
            for (int p = 0; p < NP; ++p) {
                f32x4 acc_u[4], acc_c[4];
                const int img0 = R_STAGES + p * 2 * NS;
                const bool last_panel = p + 1 == NP;
#define GGNN_X_STAGES(S)                                                                                            \
                if constexpr ((S) < NX) {                                                                           \
                    make_planes(af);                                                                                \
                    stage(std::integral_constant<bool, (S) == 0>{}, acc_u, af, img0 + 2 * (S), nothing, std::true_type{}); \
                    auto next_seg = [&] { load_frag<D>(af, (S) + 1 < NX ? a.x[(S) + 1 < NX ? (S) + 1 : 0] : a.h, rowc, kq); }; \
                    stage(std::integral_constant<bool, (S) == 0>{}, acc_c, af, img0 + 2 * (S) + 1, next_seg, std::true_type{}); \
                }
                GGNN_X_STAGES(0) GGNN_X_STAGES(1) GGNN_X_STAGES(2)
#undef GGNN_X_STAGES
                // h -> u columns; afterwards the fragment registers are free: the next panel's (or next pass's) x_0 goes there
                auto after_h = [&] { load_frag<D>(af, a.x[0], last_panel ? rown : rowc, kq); };
                stage(std::false_type{}, acc_u, af, img0 + 2 * NX, after_h, std::false_type{});
                stage(std::false_type{}, acc_c, rh, img0 + 2 * NX + 1, nothing, std::false_type{});
                if constexpr (ACT) { if (row < a.V) gru_panel_epilogue<D, FMT, SAVE, true>(a, bias_s, acc_u, acc_c, row, p, kq); }
            }
        };
        if (active) run_pass(std::true_type{});
        else run_pass(std::false_type{});
    }

    // ---- cooperative tail passes (the ring is idle from here on; its first bytes carry the r*h exchange block) ---------------
    constexpr int RHP = D + 4;                                  // row pitch of the exchange block [16][RHP]
    for (; tk < n_tk; tk += nb) {
        const int tile = tile_of(tk);                           // the same tile for every wave
        const int row = tile * 16 + li;
        const int rowc = row < a.V ? row : a.V - 1;
        const int p = wave;                                     // this wave's panel
        const bool on = p < NP;
        float* rh_x = ring_lds;
        auto gimg = [&](int img_idx) { return packed + (size_t)img_idx * IMGF; };
        auto gmma = [&](auto zero_c, f32x4 (&acc)[4], const Frag<D>& A, const float* img) {     // whole image, straight from L2
            if constexpr (SPLIT) {
                panel_part_mma_split<D, decltype(zero_c)::value, true, 0, FMT>(acc, A, img, li, kq);
                if constexpr (SC::PARTS > 1) panel_part_mma_split<D, false, true, 1, FMT>(acc, A, img + (size_t)SC::PART, li, kq);
                if constexpr (SC::PARTS > 2) panel_part_mma_split<D, false, true, 2, FMT>(acc, A, img + (size_t)2 * SC::PART, li, kq);
            } else panel_mma_global<D, decltype(zero_c)::value>(acc, A, img, li, kq);
        };
        Frag<D> rh;
        f32x4 accr[4];
        if (on) {
            // phase R for the panel's 64 columns: segments in order, h last
#define GGNN_CR_STAGE(S)                                                                                            \
            if constexpr ((S) < NS) {                                                                               \
                load_frag<D>(af, (S) < NX ? a.x[(S) < NX ? (S) : 0] : a.h, rowc, kq);                               \
                gmma(std::integral_constant<bool, (S) == 0>{}, accr, af, gimg((S) * NP + p));                       \
            }
            GGNN_CR_STAGE(0) GGNN_CR_STAGE(1) GGNN_CR_STAGE(2) GGNN_CR_STAGE(3)
#undef GGNN_CR_STAGE
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int col = p * 64 + nt * 16 + 4 * kq;
                const f32x4 r = panel_sigmoid4<FMT>(accr[nt], ld4(bias_s + col));
                const f32x4 hv = ld4_b(a.h, ((unsigned)rowc * D + col) * 4u);
                if constexpr (SAVE) { if (row < a.V) st4_b(a.save_r, ((unsigned)row * D + col) * 4u, r); }
                *reinterpret_cast<f32x4*>(rh_x + li * RHP + col) = r * hv;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) rh.v[c] = *reinterpret_cast<const f32x4*>(rh_x + li * RHP + 16 * c + 4 * kq);
        __syncthreads();                                        // (the block is rewritten by the next cooperative pass)
        if (on) {
            f32x4 acc_u[4], acc_c[4];
            const int img0 = R_STAGES + p * 2 * NS;
#define GGNN_CX_STAGES(S)                                                                                           \
            if constexpr ((S) < NX) {                                                                               \
                load_frag<D>(af, a.x[(S)], rowc, kq);                                                               \
                gmma(std::integral_constant<bool, (S) == 0>{}, acc_u, af, gimg(img0 + 2 * (S)));                    \
                gmma(std::integral_constant<bool, (S) == 0>{}, acc_c, af, gimg(img0 + 2 * (S) + 1));                \
            }
            GGNN_CX_STAGES(0) GGNN_CX_STAGES(1) GGNN_CX_STAGES(2)
#undef GGNN_CX_STAGES
            load_frag<D>(af, a.h, rowc, kq);
            gmma(std::false_type{}, acc_u, af, gimg(img0 + 2 * NX));
            gmma(std::false_type{}, acc_c, rh, gimg(img0 + 2 * NX + 1));
            if (row < a.V) gru_panel_epilogue<D, FMT, SAVE, false>(a, bias_s, acc_u, acc_c, row, p, kq);
        }
    }
}

template <int D, int NX, bool SAVE, bool SPLIT, int FMT = kSplitBf16x3>
static int launch_gru_panel_m(const GruFusedArgs& a_in, float* packed, hipStream_t st) {
    using C = PanelCfg<D>;
    GruFusedArgs a = a_in;
    if (a.Wg) {   // raw weights given: build the stage images first
        hipLaunchKernelGGL((gru_panel_pack_kernel<D, SPLIT, FMT>), dim3(8, panel_gru_images(D, NX)), dim3(256), 0, st, a.Wg, a.Wc, NX, packed);
        GGNN_CHECK_HIP(hipGetLastError());
    }
    if (a.h == nullptr) return GGNN_OK;   // pack-only call
    if ((unsigned long long)a.V * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "fused GRU indexes with 32-bit byte offsets: V*D must be < 2^30 (V=%d, D=%d)", a.V, D);
    // ring: two images (f32) / two parts of an image (split); the cooperative tail's r*h exchange block [16][D + 4] shares it
    size_t ringb = (size_t)2 * (SPLIT ? PanelGruSplitCfg<D, FMT>::PART_BYTES : C::IMG_BYTES);
    if (ringb < (size_t)16 * (D + 4) * sizeof(float)) ringb = (size_t)16 * (D + 4) * sizeof(float);
    const size_t lds = ringb + (size_t)((4 * D + 63) / 64 * 64) * sizeof(float);
    return panel_launch<&ggnn_gru_panel_kernel<D, NX, kPanelNW, SAVE, SPLIT, FMT>>(lds, 64 * 1024, panel_blocks(a.V, 1), st, a, (const float*)packed);
}

int gru_panel_supported(int D) { return panel_hidden_ok(D); }

int gru_panel_pack_floats(int D, int nx) {
    if (!gru_panel_supported(D)) return 0;
    // (sized for either operand format of the split form: the larger of the two image sizes)
    const int img = !split_matrix_path() ? D * 64 : panel_for_D(D, [](auto d) {
        return std::max(PanelGruSplitCfg<decltype(d)::value>::IMG, PanelGruSplitCfg<decltype(d)::value, kSplitF16x2>::IMG);
    });
    return panel_gru_images(D, nx) * img;
}

// The panel GRU's instantiations are GGNN_GRU_PANEL_TABLE (ggnn_gru_cells.hpp); gru_select() has chosen the cell.
int gru_panel_launch_cell(const GruCell& c, const GruFusedArgs& a, float* packed, hipStream_t st) {
    switch (gru_cell_key(c)) {
#define GGNN_GRU_PANEL_LAUNCH(D, NX, SAVE, FMT)                                                                              \
        case gru_cell_key(GGNN_GRU_PANEL_CELL(D, NX, SAVE, FMT)):                                                             \
            return launch_gru_panel_m<D, NX, SAVE, (FMT) != 0, (FMT) != 0 ? (FMT) : kSplitBf16x3>(a, packed, st);
        GGNN_GRU_PANEL_TABLE(GGNN_GRU_PANEL_LAUNCH)
#undef GGNN_GRU_PANEL_LAUNCH
        default: return fail(GGNN_E_UNSUPPORTED, "no panel GRU for hidden size %d", c.D);
    }
}

// ---- compacted message transform on panels ------------------------------------------------------------------------------
constexpr int kMaxTypesP = 64;
struct PanelRows {
    int row_off[kMaxTypesP + 1];       // compact rows of type t: row_off[t] .. row_off[t+1]-1
    int wg_off[kMaxTypesP + 1];        // workgroups of type t (all its panels): wg_off[t] .. wg_off[t+1]-1, a multiple of NP each
    int T;
};

// the types' compact rows row_off[0 .. T] and `mult` x n workgroups for a type, n in proportion to its rows out of `budget` for all types
// together: no more than it has passes of kPanelNW tiles, at least one where it has rows
static PanelRows panel_rows(const int* row_off, int T, int budget, int mult) {
    PanelRows pr{};
    pr.T = T;
    const int R = row_off[T];
    for (int t = 0; t < T; ++t) {
        pr.row_off[t] = row_off[t];
        const long long rows = row_off[t + 1] - row_off[t];
        long long n = rows * budget / R;
        const long long rounds = (rows + 16 * kPanelNW - 1) / (16 * kPanelNW);
        if (n > rounds) n = rounds;
        if (rows > 0 && n < 1) n = 1;
        pr.wg_off[t + 1] = pr.wg_off[t] + (int)n * mult;
    }
    pr.row_off[T] = R;
    return pr;
}

// workgroup (type t, panel p, j-th of the type's workgroups on that panel): keeps image (t, p) in LDS and walks 16-row tiles
// j*NW + wave, + stride, ... of the type's active pairs; the rows of tile k+1 are fetched under the MFMAs of tile k.
template <int D, int NW, bool SPLIT>
__global__ __launch_bounds__(NW * 64) void msg_transform_panel_kernel(const float* __restrict__ h, const int* __restrict__ pair_node,
                                                                      PanelRows pr, const float* __restrict__ packed,
                                                                      float* __restrict__ Hc) {
    using C = PanelCfg<D>;
    constexpr int IMGF = SPLIT ? PanelSplitCfg<D>::IMG : C::IMG;
    constexpr int NP = C::NP;
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    int t = 0;
    while (t + 1 < pr.T && (int)blockIdx.x >= pr.wg_off[t + 1]) ++t;
    const int wg_in_type = (int)blockIdx.x - pr.wg_off[t];
    const int per_panel = (pr.wg_off[t + 1] - pr.wg_off[t]) / NP;       // workgroups of this type on each panel
    const int p = wg_in_type / per_panel, j = wg_in_type % per_panel;
    const int row_beg = pr.row_off[t], row_end = pr.row_off[t + 1];
    const int n_wt = (row_end - row_beg + 15) / 16;
    const int stride = per_panel * NW;
    int idx = j * NW + wave;

    auto row_of = [&](int i) { const int r = row_beg + i * 16 + li; return r < row_end ? r : row_end - 1; };
    Frag<D> a, an;
    int node_0 = 0, node_n = 0;
    if (idx < n_wt) node_0 = pair_node[row_of(idx)];
    if (idx + stride < n_wt) node_n = pair_node[row_of(idx + stride)];
    if constexpr (SPLIT) dma_image_asm<PanelSplitCfg<D>::IMG_BYTES, NW>(packed + (size_t)(t * NP + p) * IMGF, img, wave, lane);
    else dma_block<C::IMG_BYTES, NW>(packed + (size_t)(t * NP + p) * IMGF, img, wave, lane);
    if (idx < n_wt) load_frag<D>(a, h, node_0, kq);
    if constexpr (SPLIT) dma_wait();
    __syncthreads();

    while (idx < n_wt) {
        const int idx_n = idx + stride;
        if (idx_n < n_wt) load_frag<D>(an, h, node_n, kq);
        if (idx_n + stride < n_wt) node_n = pair_node[row_of(idx_n + stride)];
        f32x4 acc[4];
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SPLIT) panel_mma_split<D, true>(acc, a, img, li, kq);
        else panel_mma<D, true>(acc, a, img, li, kq);
        const int r = row_beg + idx * 16 + li;
        if (r < row_end) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) st4_b(Hc, ((unsigned)r * (unsigned)D + p * 64 + nt * 16 + 4 * kq) * 4u, acc[nt]);
        }
        a = an;
        idx = idx_n;
    }
}

// ---- the same transform with the panel images STREAMED and the rows read once (round 4, split form) ------------------------------
// msg_transform_panel_kernel keeps ONE (type, panel) image per workgroup, so every state row is fetched once per panel (D = 256: four
// times; 1.11 GB of traffic for 0.48 GB algorithmic) and split once per panel.  Here a workgroup is bound to a TYPE: a pass takes
// one 16-row tile per wave, splits its fragment ONCE into resident bf16 planes (96 registers at D = 256; the f32 fragment's registers
// then receive the next tile's rows) and walks the type's NP panels, whose images come through a two-slot LDS ring in
// PanelGruSplitCfg::PARTS parts -- the panel GRU's chunk-major image format and ring (48 KiB parts at D = 256).  Per pass and CU
// NP x 96 KiB of weights from L2 instead of (NP - 1) x 128 KiB of rows from HBM / Infinity Cache, and 352 instead of NP x 352
// split instructions per tile.
// pr.wg_off counts the workgroups of a type (NOT times NP); packed: [T][NP] images in pack_panel_gru_split_image's format
// FMT (round 5): operand format of the products and of the images, per launch (kSplitF16x2: two planes, whole images through the
// ring -- no parts -- for a forward transform whose states and edge weights the caller has proven in range; formats.py).
template <int D, int NW, int FMT = kSplitBf16x3>
__global__ __launch_bounds__(NW * 64) void msg_transform_ring_kernel(const float* __restrict__ h, const int* __restrict__ pair_node,
                                                                     PanelRows pr, const float* __restrict__ packed, float* __restrict__ Hc) {
    using C = PanelCfg<D>;
    using SC = PanelGruSplitCfg<D, FMT>;
    constexpr int NP = C::NP, PARTS = SC::PARTS, SLOTF = SC::PART, IMGF = SC::IMG, NC2 = SC::NC2;
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];     // [2][PART]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    int t = 0;
    while (t + 1 < pr.T && (int)blockIdx.x >= pr.wg_off[t + 1]) ++t;
    const int row_beg = pr.row_off[t], row_end = pr.row_off[t + 1];
    const int n_wt = (row_end - row_beg + 15) / 16;
    const PanelPassWalk<NW> walk(n_wt, (int)blockIdx.x - pr.wg_off[t], pr.wg_off[t + 1] - pr.wg_off[t]);
    const int stride = walk.stride, idx0 = walk.base + wave;
    const float* timg = packed + (size_t)t * NP * IMGF;

    auto row_of = [&](int i) { const int r = row_beg + i * 16 + li; return r < row_end ? r : row_end - 1; };
    PanelRing<SC::PART_BYTES, NW> ring{ring_lds, wave, lane};
    static_assert(C::NC <= 16, "PanelRing's counted waits cover a fragment's row loads + a panel's stores up to D = 256");
    Frag<D> a;
    int node_n = 0;
    if (walk.n_pass > 0) ring.fill_first(timg);
    if (idx0 < n_wt) load_frag<D>(a, h, pair_node[row_of(idx0)], kq);
    if (idx0 + stride < n_wt) node_n = pair_node[row_of(idx0 + stride)];
    ring.first_ready();

    // the rounds of one pass: NP panels x PARTS parts
    walk.run(wave, [&](auto active_c, int idx, bool, bool last_pass) {
        constexpr bool ACT = decltype(active_c)::value;
        u32x4 ph[NC2], pm[NC2], pl[NC2];
        const int r = row_beg + idx * 16 + li;
        if constexpr (ACT) frag_to_planes<D, FMT>(a, ph, pm, pl);
        // the next tile's rows go into the fragment's registers (dead now) in the pass's first round, BEHIND the round's DMA
        const bool has_next = ACT && idx + stride < n_wt;
        const int node_next = node_n;
        if constexpr (ACT) { if (idx + 2 * stride < n_wt) node_n = pair_node[row_of(idx + 2 * stride)]; }    // (older than every DMA of the pass)
        f32x4 acc[4];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            panel_for_parts<PARTS>([&](auto part_c) {
                constexpr int part = decltype(part_c)::value;
                const bool more = part + 1 < PARTS || p + 1 < NP || !last_pass;
                // (a round is ~3k clocks of MFMAs for the SIMD's two waves.)  The rows and the stores are issued BEHIND the round's DMA
                // pieces and nothing follows them: they may stay in flight across the barrier.
                panel_round<part, PARTS, ACT, true>(ring, more, panel_next_part<PARTS, IMGF, SLOTF>(timg, p, part, p + 1 < NP ? p + 1 : 0),
                    [&] {
                        if (!(p == 0 && part == 0 && has_next)) return 0;
                        load_frag<D>(a, h, node_next, kq);
                        return C::NC;
                    },
                    [&] { panel_part_mma_planes<D, part == 0, part, FMT>(acc, ph, pm, pl, ring.slot(), li, kq); },
                    [&] {
                        // (every tile has a valid first row: the four stores are issued by every wave with a tile)
                        if (r < row_end) {
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) st4_b(Hc, ((unsigned)r * (unsigned)D + p * 64 + nt * 16 + 4 * kq) * 4u, acc[nt] * SplitFmt<FMT>::acc_scale);
                        }
                        return 4;
                    });
            });
        }
    });
}

// GGNN_PANEL_TRANSFORM: 1 (default) the ring kernel above (split path only), 0 the stationary-image kernel.  Read once: the packed
// edge-weight images are in the format of the kernel that will multiply them.
static bool transform_ring() {
    static const bool v = [] { const char* e = getenv("GGNN_PANEL_TRANSFORM"); return !e || atoi(e) != 0; }();
    return v && split_matrix_path();
}
// (for the training step's one-launch image preparation, ggnn_train_panel.hip, which writes the same images)
bool transform_panel_ring() { return transform_ring(); }

template <int D, bool SPLIT, int FMT = kSplitBf16x3>
__global__ void edge_weight_panel_pack_kernel(const float* __restrict__ W, float* __restrict__ out, int ring_format) {
    using C = PanelCfg<D>;
    const int t = blockIdx.y / C::NP, p = blockIdx.y % C::NP;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if constexpr (SPLIT) {
        if (ring_format) pack_panel_gru_split_image<D, FMT>(W + (size_t)t * D * D, 0, p * C::BN, D, out + (size_t)blockIdx.y * PanelGruSplitCfg<D, FMT>::IMG, first, stride);
        else pack_panel_split_image<D>(W + (size_t)t * D * D, 0, p * C::BN, D, out + (size_t)blockIdx.y * PanelSplitCfg<D>::IMG, first, stride);
    } else pack_panel_image<D>(W + (size_t)t * D * D, 0, p * C::BN, D, out + (size_t)blockIdx.y * C::IMG, first, stride);
}
static_assert(PanelGruSplitCfg<256>::IMG == PanelSplitCfg<256>::IMG && PanelGruSplitCfg<192>::IMG == PanelSplitCfg<192>::IMG &&
              PanelGruSplitCfg<128>::IMG == PanelSplitCfg<128>::IMG, "both split image formats of the transform have one size");

// floats of ONE (type, panel) image of the transform, in the process's matrix path
int transform_panel_image_floats(int D) {
    const bool sp = split_matrix_path();
    if (!panel_hidden_ok(D)) return 0;
    return panel_for_D(D, [&](auto d) { return sp ? PanelSplitCfg<decltype(d)::value>::IMG : PanelCfg<decltype(d)::value>::IMG; });
}

// ---- which kernel, in which format, on how many workgroups: host arithmetic shared by the launch and the describe query -----------
// The kernel family (GGNN_MSG_TRANSFORM_* of include/ggnn_hip.h), the matrix path and the operand format of a launch asked for `fmt`
// in this process.  Only the ring kernel (split path) has the two-piece f16 form; the stationary-image kernel and the f32 path ignore it.
struct PanelTransformChoice {
    int family;        // GGNN_MSG_TRANSFORM_RING / GGNN_MSG_TRANSFORM_STATIONARY
    bool split;
    int fmt;           // the operand format multiplied in: 0 on the f32 MFMA, else kSplitBf16x3 / kSplitF16x2
};
static PanelTransformChoice transform_panel_choice(int fmt) {
    if (!split_matrix_path()) return {GGNN_MSG_TRANSFORM_STATIONARY, false, 0};
    if (!transform_ring()) return {GGNN_MSG_TRANSFORM_STATIONARY, true, kSplitBf16x3};
    return {GGNN_MSG_TRANSFORM_RING, true, gru_launch_fmt(fmt)};
}

// the workgroups of every type under choice `c`
template <int D>
static PanelRows transform_panel_rows(const PanelTransformChoice& c, const int* row_off, int T) {
    constexpr int NP = PanelCfg<D>::NP;
    // ring: workgroups per type in proportion to its rows (one per CU all types together)
    if (c.family == GGNN_MSG_TRANSFORM_RING) return panel_rows(row_off, T, num_cus(), 1);
    // stationary: one workgroup per CU (64 KiB image + ~176 VGPRs per wave); every type gets workgroups in proportion to its rows,
    // the same number on each of its NP panels, at least one per panel
    return panel_rows(row_off, T, num_cus() / NP > 0 ? num_cus() / NP : 1, NP);
}

template <int D, bool SPLIT, int FMT = kSplitBf16x3>
static int launch_transform_panel_m(const PanelTransformChoice& c, const float* h, const float* W, const int* pair_node, const int* row_off,
                                    int T, int V, float* packed, float* Hc, hipStream_t st) {
    using C = PanelCfg<D>;
    constexpr int NP = C::NP;
    if (W) {
        hipLaunchKernelGGL((edge_weight_panel_pack_kernel<D, SPLIT, FMT>), dim3(8, T * NP), dim3(256), 0, st, W, packed, (int)(c.family == GGNN_MSG_TRANSFORM_RING));
        GGNN_CHECK_HIP(hipGetLastError());
    }
    const int R = row_off[T];
    if (R == 0 || h == nullptr) return GGNN_OK;
    if ((unsigned long long)R * D >= (1ULL << 30) || (unsigned long long)V * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "compacted transform indexes with 32-bit byte offsets: rows*D and V*D must be < 2^30");
    const PanelRows pr = transform_panel_rows<D>(c, row_off, T);
    if constexpr (SPLIT) {
        if (c.family == GGNN_MSG_TRANSFORM_RING)
            return panel_launch<&msg_transform_ring_kernel<D, kPanelNW, FMT>>((size_t)2 * PanelGruSplitCfg<D, FMT>::PART_BYTES, 48 * 1024,
                                                                               pr.wg_off[T], st, h, pair_node, pr, (const float*)packed, Hc);
    }
    return panel_launch<&msg_transform_panel_kernel<D, kPanelNW, SPLIT>>(SPLIT ? PanelSplitCfg<D>::IMG_BYTES : C::IMG_BYTES, 48 * 1024,
                                                                          pr.wg_off[T], st, h, pair_node, pr, (const float*)packed, Hc);
}

template <int D>
static int launch_transform_panel(const float* h, const float* W, const int* pair_node, const int* row_off, int T, int V,
                                  float* packed, float* Hc, int fmt, hipStream_t st) {
    const PanelTransformChoice c = transform_panel_choice(fmt);
    if (!c.split) return launch_transform_panel_m<D, false>(c, h, W, pair_node, row_off, T, V, packed, Hc, st);
    return c.fmt == kSplitF16x2 ? launch_transform_panel_m<D, true, kSplitF16x2>(c, h, W, pair_node, row_off, T, V, packed, Hc, st)
                                : launch_transform_panel_m<D, true>(c, h, W, pair_node, row_off, T, V, packed, Hc, st);
}

// ggnn_msg_transform_compact_describe at a panel hidden size: what launch_transform_panel would start for these rows.  wg[t] (zeroed by
// the caller): the workgroups of type t (all its panels); waves[t]: the waves that share ONE walk over the type's 16-row tiles (a
// stationary type's workgroups are split between its NP panels, each panel's walking all tiles).
int transform_panel_describe(int D, const int* row_off, int T, int fmt, int* family, int* fmt_used, int* nw, int* wg, int* waves) {
    if (T > kMaxTypesP) return fail(GGNN_E_UNSUPPORTED, "more than %d edge types", kMaxTypesP);
    if (!panel_hidden_ok(D)) return fail(GGNN_E_UNSUPPORTED, "no panel transform for hidden size %d", D);
    const PanelTransformChoice c = transform_panel_choice(fmt);
    *family = c.family;
    *fmt_used = c.fmt;
    *nw = kPanelNW;
    if (row_off[T] == 0) return GGNN_OK;      // no rows: the launch returns before its schedule (wg / waves stay as the caller zeroed them)
    return panel_for_D(D, [&](auto d) {
        constexpr int NP = PanelCfg<decltype(d)::value>::NP;
        const PanelRows pr = transform_panel_rows<decltype(d)::value>(c, row_off, T);
        for (int t = 0; t < T; ++t) {
            wg[t] = pr.wg_off[t + 1] - pr.wg_off[t];
            waves[t] = wg[t] / (c.family == GGNN_MSG_TRANSFORM_RING ? 1 : NP) * kPanelNW;
        }
        return GGNN_OK;
    });
}

int transform_panel_dispatch(const float* h, const float* W, const int* pair_node, const int* row_off, int T, int V, int D,
                             float* packed, float* Hc, int fmt, hipStream_t st) {
    if (T > kMaxTypesP) return fail(GGNN_E_UNSUPPORTED, "more than %d edge types", kMaxTypesP);
    if (!panel_hidden_ok(D)) return fail(GGNN_E_UNSUPPORTED, "no panel transform for hidden size %d", D);
    return panel_for_D(D, [&](auto d) { return launch_transform_panel<decltype(d)::value>(h, W, pair_node, row_off, T, V, packed, Hc, fmt, st); });
}

}  // namespace ggnn
