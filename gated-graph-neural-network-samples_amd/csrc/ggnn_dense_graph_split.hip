// K7 in split form: the graph-resident dense GGNN forward (chem_tensorflow_dense.py:93-117; see ggnn_dense_graph.hip for the
// f32-MFMA kernel this one replaces on the default matrix path) with every D x D product on the bf16 matrix pipe (ggnn_split.hpp:
// f32 operands as three bf16 pieces, six products, f32 accumulation).
//
// The f32 kernel is bound by its MFMAs -- ten stages of 2 x 25 v_mfma_f32_16x16x4_f32 per wave and timestep at 3.4-3.8k clocks for
// 3.2k of matrix-pipe time -- and had no registers left for split planes: every wave held the FULL f32 activation fragments of both
// row tiles (100 registers) next to two weight slices.  Here the activations never live in registers:
//   * what a stage group consumes (the state h, the aggregated messages, r*h) sits in LDS ALREADY SPLIT, in the MFMA operand layout
//     [plane][32-chunk][lane group g][row][8 x bf16]: a wave reads one ds_read_b128 per (plane, chunk, row tile) straight into the
//     operand of six MFMAs (conflict-free as laid out: the b128 lane groups cover 16 consecutive 16-byte slots);
//   * the PRODUCER splits: a wave owns column tile `tile` of every block, i.e. the four k values 16 tile + 4 kq .. of rows li and
//     li + 16 -- exactly slots 4 (tile & 1) .. + 3 of lane group kq in chunk tile >> 1 -- splits those eight values (22 vector
//     instructions) and writes three ds_write_b64 per row tile.  Eight waves splitting the same fragments redundantly (what keeping
//     the f32 kernel's structure would have meant) is 800 vector instructions per wave and timestep; this is 66.
//   * a wave's slice of a stage's weights -- its column tile of the split image: 9 x 16 bytes + the remainder float per lane -- comes
//     from L2 into registers one stage ahead (GGNN_DENSE_STAGE; the f32 kernel does the same with its register fragments).
// The operand tile itself (TileW, load_w, tile_to_planes, mma_pair), the LDS layout (DenseSplitLds) and the pieces shared with the f32
// kernel (prologue, aggregation, stage macro) are in ggnn_dense_graph.hpp; the backward uses the same tile.
// Stage order of a timestep: E transforms, h -> r, h -> u (all on the state planes) | aggregation (f32 MFMA: the 0/1 adjacency
// times M_e is exact) | x -> r, x -> u, x -> c | gates | r*h -> c | blend.  The h products come FIRST (the f32 kernel adds them after
// the x products): one operand block live at a time.  r and u are therefore sums in the other order -- within the parity tolerances
// of tests/test_gpu_dense.py, not bit-identical to the three-launch path.
#include "ggnn_dense_graph.hpp"

namespace ggnn {

namespace {

__device__ __forceinline__ float sigm(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-kLog2e * x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.0f * kLog2e * x)); }

}  // namespace

// six GRU images in the order the kernel consumes them: (h,r) (h,u) (x,r) (x,u) (x,c) (r*h,c);  Wg rows [x | h], columns [r | u]
template <int D, int FMT>
__global__ void dense_split_pack_kernel(const float* __restrict__ W, const float* __restrict__ Wg, const float* __restrict__ Wc,
                                        float* __restrict__ out) {
    const int i = blockIdx.y;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    float* img = out + (size_t)i * SplitCfg<D, FMT>::IMG;
    if (W) {                                                          // edge type i
        pack_split_image<D, FMT>(StageValue<D>{W + (size_t)i * D * D, 0, 0, D, -1, nullptr, 0, 0, -1}, img, first, stride);
    } else {
        constexpr int rows[6] = {1, 1, 0, 0, 0, 1}, cols[6] = {0, 1, 0, 1, 0, 0};
        if (i < 4) pack_split_image<D, FMT>(StageValue<D>{Wg, rows[i] * D, cols[i] * D, 2 * D, -1, nullptr, 0, 0, -1}, img, first, stride);
        else pack_split_image<D, FMT>(StageValue<D>{Wc, rows[i] * D, 0, D, -1, nullptr, 0, 0, -1}, img, first, stride);
    }
}

// FMT (round 5): operand format of every D x D product of the kernel, per launch -- the exact kSplitBf16x3 or kSplitF16x2 (two f16
// pieces, three products, two operand planes) when the caller has PROVEN its range for the launch (dense_model.py / formats.py:
// states tanh-bounded, |acts| <= v E (D max|W| S + max|b|), weights <= 255.875).  Accumulators then hold 2^8 x the sums
// (SplitFmt<FMT>::acc_scale is applied where they are consumed).
// SAVE (training, ggnn_dense_propagate_save_f32): the launch also stores, per timestep and for the rows i < v, what the backward
// launch (ggnn_dense_graph_bwd.hip) and the weight-gradient products read -- a.saved [6][steps][b v, D] (each tensor stacked over the
// timesteps: a row operand of the weight-gradient products): the state h_t entering the step, the aggregated messages x_t, r, u, c,
// r*h.  Stores only: the arithmetic, and `out`, are those of the plain launch bit for bit.
template <int D, int E, int NW, int FMT, bool SAVE = false>
__global__ __launch_bounds__(NW * 64) void ggnn_dense_graph_split_kernel(DenseGraphArgs a) {
    using C = StageCfg<D>;
    using SC = SplitCfg<D, FMT>;
    using L = DenseSplitLds<D, E, FMT>;
    constexpr float ASC = SplitFmt<FMT>::acc_scale;
    constexpr int NT = C::NT, NC = C::NC, NR = C::NR;
    constexpr int MP = L::T::MP;                                       // row pitch of the f32 M_e blocks (floats)
    constexpr int NS = E + 6;                                          // stages per timestep
    static_assert(NT <= NW && NS % 2 == 0 && NR <= 1, "one column tile per wave; two weight slots with a fixed phase per timestep");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Mbuf = lds + L::M;                                          // [E][32][MP] f32: the transformed states, for the aggregation
    float* Hblk = lds + L::H, * Xblk = lds + L::X, * Rblk = lds + L::R;   // split operand blocks: state | aggregated messages | r*h
    float* Abuf = lds + L::A, * Nbuf = lds + L::N, * Bbuf = lds + L::B;   // adjacency rows, in-degrees per type, edge biases
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int g = blockIdx.x;
    const int v = a.v;
    const bool mm = wave < NT;
    const int tile = mm ? wave : 0;
    const int col0 = 16 * tile + 4 * kq;
    const bool tail = NR > 0 && tile == NC;                            // the tile of the D % 16 remainder columns (kq == 0 lanes hold them)

    auto image = [&](int s) { return dense_stage_image<E, SC::IMG>(a, s); };
    auto to_lds = [&](float* blk, int t, f32x4 val) { tile_to_lds<D>(blk, t, val, li, kq, tile); };
    auto to_planes = [&](float* blk, int t, f32x4 val) { tile_to_planes<D, FMT>(blk, t, val, li, kq, tile, mm, tail); };

    // (SAVE) this wave's four columns of row tile t -> tensor k of timestep `step`
    auto save_tile = [&](int step, int k, int t, f32x4 val) {
        const int i = t * 16 + li;
        if (mm && i < v && col0 < D)
            *reinterpret_cast<f32x4*>(a.saved + (((size_t)k * a.steps + step) * a.b * v + (size_t)g * v + i) * D + col0) = val;
    };

    dense_load_adjacency<E, NW>(Abuf, a.A, v, tid);
    dense_load_edge_bias<D, E, NW>(Bbuf, a.ebias, tid);
    // the initial state: this wave's column tile of both row tiles (also kept as f32 for r*h and the blend)
    f32x4 htile[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = t * 16 + li;
        f32x4 hv = {0.f, 0.f, 0.f, 0.f};
        if (mm && i < v && col0 < D) hv = *reinterpret_cast<const f32x4*>(a.h0 + ((size_t)g * v + i) * D + col0);
        htile[t] = hv;
        to_planes(Hblk, t, hv);
    }
    __syncthreads();
    dense_in_degrees<E>(Nbuf, Abuf, tid);
    f32x4 b_r, b_u, b_c;
    dense_gate_bias<D>(b_r, b_u, b_c, a.bg, a.bc, col0);

    const int nth = tile_w_nth<D, FMT>(tile);
    const unsigned w_base = tile_w_base<D, FMT>(li, kq, tile), wr_base = tile_wr_base<D, FMT>(li, kq, tile);
    const unsigned w_cst = tile_w_cst(nth), w_pst = (unsigned)SC::NC2 * w_cst;                     // chunk / plane pitch in bytes
    auto load_w = [&](TileW<D, FMT>& w, const float* gimg) { ggnn::load_w<D, FMT>(w, gimg, w_base, w_cst, w_pst, wr_base, nth); };
    auto mma_pair = [&](auto zero_c, f32x4 (&acc)[2], const float* blk, const TileW<D, FMT>& w) {
        ggnn::mma_pair<D, FMT, decltype(zero_c)::value>(acc, blk, w, li, kq);
    };
    TileW<D, FMT> tw[2];
    if (mm) load_w(tw[0], image(0));
    __syncthreads();                                                   // state planes, adjacency, in-degrees, biases

    for (int step = 0; step < a.steps; ++step) {
        const bool last = step + 1 == a.steps;
        GGNN_DENSE_STAMP(step, 0)
        if constexpr (SAVE) { save_tile(step, 0, 0, htile[0]); save_tile(step, 0, 1, htile[1]); }
        // ---- E transform stages: M_e = h W_e, column tile `tile`, into LDS (f32: the aggregation's operand) ------------------
        f32x4 acc[2];
#define GGNN_DGS_XFORM(S)                                                                                  \
        if constexpr ((S) < E) {                                                                           \
            GGNN_DENSE_STAGE(S, acc, Hblk, true)                                                           \
            if (mm) { to_lds(Mbuf + (size_t)(S) * 32 * MP, 0, acc[0] * ASC); to_lds(Mbuf + (size_t)(S) * 32 * MP, 1, acc[1] * ASC); } \
        }
        GGNN_DGS_XFORM(0) GGNN_DGS_XFORM(1) GGNN_DGS_XFORM(2) GGNN_DGS_XFORM(3) GGNN_DGS_XFORM(4) GGNN_DGS_XFORM(5) GGNN_DGS_XFORM(6) GGNN_DGS_XFORM(7)
#undef GGNN_DGS_XFORM
        // ---- the state's share of the gates, while the state planes are the live operand ----------------------------------------
        f32x4 ar[2], au[2], ac[2];
        GGNN_DENSE_STAGE(E + 0, ar, Hblk, true)
        GGNN_DENSE_STAGE(E + 1, au, Hblk, true)
        GGNN_DENSE_STAMP(step, 1)
        __syncthreads();                                               // (1) every M_e is complete
        GGNN_DENSE_STAMP(step, 2)
        // ---- aggregation on the matrix pipe (f32: A_e is 0/1, the products are exact) ------------------------------------------------
        f32x4 aa[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (mm) GGNN_DENSE_AGGREGATE(aa)
        to_planes(Xblk, 0, aa[0]); to_planes(Xblk, 1, aa[1]);
        if constexpr (SAVE) { save_tile(step, 1, 0, aa[0]); save_tile(step, 1, 1, aa[1]); }
        GGNN_DENSE_STAMP(step, 3)
        __syncthreads();                                               // (2) acts complete, split
        GGNN_DENSE_STAMP(step, 4)
        // ---- the messages' share of the gates and of the candidate ----------------------------------------------------------------
        GGNN_DENSE_STAGE(E + 2, ar, Xblk, false)
        GGNN_DENSE_STAGE(E + 3, au, Xblk, false)
        GGNN_DENSE_STAGE(E + 4, ac, Xblk, true)
        f32x4 u4[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x4 r4;
#pragma unroll
            for (int e = 0; e < 4; ++e) { r4[e] = sigm(ar[t][e] * ASC + b_r[e]); u4[t][e] = sigm(au[t][e] * ASC + b_u[e]); }
            to_planes(Rblk, t, r4 * htile[t]);                         // r * h tile
            if constexpr (SAVE) {
                // the saved r*h is a product of ITS OWN (r through an empty asm: not the expression above to the compiler): the operand's
                // r*h stays single-use, so its split contracts to fma(r, h, -hi) exactly where the plain instantiation's does -- a
                // shared product would feed the split the ROUNDED r*h and change the mid / lo pieces, i.e. the bits of `out`
                f32x4 rs = r4;
                asm volatile("" : "+v"(rs));
                save_tile(step, 2, t, r4); save_tile(step, 3, t, u4[t]); save_tile(step, 5, t, rs * htile[t]);
            }
        }
        GGNN_DENSE_STAMP(step, 5)
        __syncthreads();                                               // (3) r*h complete, split
        GGNN_DENSE_STAMP(step, 6)
        GGNN_DENSE_STAGE(E + 5, ac, Rblk, false)
        GGNN_DENSE_STAMP(step, 7)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x4 hn, c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = tanhf_(ac[t][e] * ASC + b_c[e]);
                hn[e] = u4[t][e] * htile[t][e] + (1.0f - u4[t][e]) * c;
                c4[e] = c;
            }
            if constexpr (SAVE) save_tile(step, 4, t, c4);
            if (col0 >= D) hn = f32x4{0.f, 0.f, 0.f, 0.f};              // (the padding columns of the last tile stay zero operands)
            htile[t] = hn;
            if (last) {
                const int i = t * 16 + li;
                if (mm && i < v && col0 < D) *reinterpret_cast<f32x4*>(a.out + ((size_t)g * v + i) * D + col0) = hn;
            } else {
                to_planes(Hblk, t, hn);
            }
        }
        if (!last) __syncthreads();                                    // (4) new state complete, split
    }
}

// (the fit test is the bf16x3 layout's, the larger of the two formats: a shape runs the split kernel in either format or in neither)
int dense_split_supported(int v, int E, int D) {
    return dense_shape_ok(v, E, D) && dense_dispatch(D, E, [](auto d, auto e) {
        return DenseSplitLds<decltype(d)::value, decltype(e)::value, kSplitBf16x3>::BYTES <= kDenseLdsLimit; });
}

// bytes of T images of one format
static size_t images_bytes(int D, int T, int fmt) {
    return dense_for_D(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return (size_t)T * (fmt == kSplitF16x2 ? SplitCfg<DD, kSplitF16x2>::IMG_BYTES : SplitCfg<DD>::IMG_BYTES); });
}
// the split section of a packed buffer: the bf16x3 images followed by the f16x2 ones (the format is chosen per launch)
size_t dense_split_edge_bytes(int D, int T) { return images_bytes(D, T, kSplitBf16x3) + images_bytes(D, T, kSplitF16x2); }
size_t dense_split_gru_bytes(int D) { return dense_split_edge_bytes(D, 6); }
size_t dense_split_images_offset(int D, int T, int fmt) { return fmt == kSplitF16x2 ? images_bytes(D, T, kSplitBf16x3) : 0; }

// T images of both formats: the edge types of W, or (W == NULL) the six GRU images
static int pack_split(const float* W, const float* Wg, const float* Wc, int T, int D, float* packed, hipStream_t st) {
    float* p2 = packed + images_bytes(D, T, kSplitBf16x3) / sizeof(float);
    dense_for_D(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((dense_split_pack_kernel<DD, kSplitBf16x3>), dim3(8, T), dim3(256), 0, st, W, Wg, Wc, packed);
        hipLaunchKernelGGL((dense_split_pack_kernel<DD, kSplitF16x2>), dim3(8, T), dim3(256), 0, st, W, Wg, Wc, p2);
        return 0; });
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
int dense_split_pack_edge(const float* W, int T, int D, float* packed, hipStream_t st) { return pack_split(W, nullptr, nullptr, T, D, packed, st); }
int dense_split_pack_gru(const float* Wg, const float* Wc, int D, float* packed, hipStream_t st) { return pack_split(nullptr, Wg, Wc, 6, D, packed, st); }

template <int D, int E, int FMT>
static int launch_split_fmt(const DenseGraphArgs& a, hipStream_t st) {
    constexpr size_t ldsb = DenseSplitLds<D, E, FMT>::BYTES;
    return a.saved ? dense_graph_launch<&ggnn_dense_graph_split_kernel<D, E, kDenseWaves, FMT, true>>(ldsb, a, st)
                   : dense_graph_launch<&ggnn_dense_graph_split_kernel<D, E, kDenseWaves, FMT, false>>(ldsb, a, st);
}

// a.eimg / a.gimg: the images of the format `fmt` (dense_split_images_offset into the split section of the packed buffers);
// a.saved != NULL: the saving instantiation (training)
int dense_split_launch(const DenseGraphArgs& a, int E, int D, int fmt, hipStream_t st) {
    const bool f2 = gru_launch_fmt(fmt) == kSplitF16x2;
    if (!dense_shape_ok(a.v, E, D)) return fail(GGNN_E_UNSUPPORTED, "graph-resident dense forward (split form): unsupported shape");
    return dense_dispatch(D, E, [&](auto d, auto e) {
        constexpr int DD = decltype(d)::value, EE = decltype(e)::value;
        return f2 ? launch_split_fmt<DD, EE, kSplitF16x2>(a, st) : launch_split_fmt<DD, EE, kSplitBf16x3>(a, st); });
}

}  // namespace ggnn
