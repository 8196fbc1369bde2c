// K7, training: the backward of the graph-resident dense GGNN forward (chem_tensorflow_dense.py:93-117; what TF autodiff derives from
// it through compute_gradients, chem_tensorflow.py:184).  One workgroup per graph walks the timesteps in REVERSE on what the saving
// forward launch wrote (ggnn_dense_graph_split.hip, SAVE): the gradient of the graph's states never leaves its CU.
//
// The structure is the forward's, on the shared tile layer of ggnn_dense_graph.hpp (TileW, load_w, tile_to_planes, mma_pair; the LDS
// layout is DenseBwdLds): operands in LDS already split into MFMA planes ([plane][32-chunk][lane group][row][8 x bf16], written
// by the wave that produced them), one column tile per wave, each wave's weight slice of a stage -- its column tile of a TRANSPOSED
// split image (dense_bwd_pack_kernel) -- fetched from L2 one stage ahead.  Every product runs in the exact bf16x3 format, as every
// backward product of this library does.  Per timestep t = steps-1 .. 0, with g = dL/dh_{t+1}:
//     dpc = g (1-u)(1-c^2)           dpu = g (h-c) u (1-u)                               (registers; split into blocks Bc, Bu)
//     drh = dpc Wc[h]^T              dpr = drh h r (1-r)                                 stage 0; dpr split into block Br
//     dx  = dpr Wg[x,r]^T + dpu Wg[x,u]^T + dpc Wc[x]^T                                  stages 1-3
//     dh  = dpr Wg[h,r]^T + dpu Wg[h,u]^T                                                stages 4-5
//     dM_e[src] = sum_dst A_e[dst,src] dx[dst]                                           f32 MFMA on dx in LDS, like the forward's aggregation
//     dh += dM_e W_e^T   for every e                                                     stages 6 .. 6+E-1, in groups of four operand blocks
//     g <- (dh + drh r) + g u
// 6 + E transposed D x D products, the forward's count.  The accumulator chains start from ZERO and g u is added last: an accumulator
// opened with g u would round every MFMA partial sum at that term's magnitude.
// Rows i >= v of the 32-row tiles and columns >= D of the last column tile are zero operands throughout (g, and every saved tensor,
// load as zero there, and every formula above is linear in g).  No atomics: the same inputs give the same bits.
#include "ggnn_dense_graph.hpp"

namespace ggnn {

// 6 + E transposed images in the order the kernel consumes them: Wc[h]^T, Wg[x,r]^T, Wg[x,u]^T, Wc[x]^T, Wg[h,r]^T, Wg[h,u]^T, W_e^T
// (Wg rows [x | h], columns [r | u];  Wc rows [x | r*h])
template <int D>
__global__ void dense_bwd_pack_kernel(const float* __restrict__ W, const float* __restrict__ Wg, const float* __restrict__ Wc,
                                      float* __restrict__ out) {
    const int i = blockIdx.y;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    float* img = out + (size_t)i * SplitCfg<D>::IMG;
    StageValueT<D> val{W + (size_t)(i >= 6 ? i - 6 : 0) * D * D, 0, 0, D};
    if (i == 0) val = StageValueT<D>{Wc, D, 0, D};
    else if (i == 1) val = StageValueT<D>{Wg, 0, 0, 2 * D};
    else if (i == 2) val = StageValueT<D>{Wg, 0, D, 2 * D};
    else if (i == 3) val = StageValueT<D>{Wc, 0, 0, D};
    else if (i == 4) val = StageValueT<D>{Wg, D, 0, 2 * D};
    else if (i == 5) val = StageValueT<D>{Wg, D, D, 2 * D};
    pack_split_image<D>(val, img, first, stride);
}

template <int D, int E, int NW>
__global__ __launch_bounds__(NW * 64) void ggnn_dense_graph_bwd_kernel(DenseGraphBwdArgs a) {
    using C = StageCfg<D>;
    using SC = SplitCfg<D>;
    using L = DenseBwdLds<D, E>;
    constexpr int FMT = kSplitBf16x3;                                  // every backward product runs in the exact format
    constexpr int NT = C::NT, NC = C::NC, NR = C::NR;
    constexpr int MP = L::T::MP, AP = L::T::AP, PBLK = L::T::PBLK;     // pitch of the f32 dx block, of an adjacency row; one operand block
    constexpr int NS = E + 6;                                          // stages per timestep
    static_assert(NT <= NW && NS % 2 == 0 && NR <= 1, "one column tile per wave; two weight slots with a fixed phase per timestep");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* DXbuf = lds + L::DX;                                        // [32][MP] f32: dx, the aggregation's operand
    float* Pblk = lds + L::P;                                          // [NB] split operand blocks
    float* Abuf = lds + L::A;                                          // [E][32][AP] adjacency rows
    float* Bc = Pblk, * Bu = Pblk + PBLK, * Br = Pblk + 2 * PBLK;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int g = blockIdx.x;
    const int v = a.v;
    const bool mm = wave < NT;
    const int tile = mm ? wave : 0;
    const int col0 = 16 * tile + 4 * kq;
    const bool tail = NR > 0 && tile == NC;                            // the tile of the D % 16 remainder columns (kq == 0 lanes hold them)
    const size_t bv = (size_t)a.b * v;

    auto image = [&](int s) { return a.img + (size_t)s * SC::IMG; };
    auto to_lds = [&](float* blk, int t, f32x4 val) { tile_to_lds<D>(blk, t, val, li, kq, tile); };
    auto to_planes = [&](float* blk, int t, f32x4 val) { tile_to_planes<D, FMT>(blk, t, val, li, kq, tile, mm, tail); };
    // this wave's four columns of row tile t of a [.., ld] tensor of this graph: zero outside the graph's rows and the D columns
    auto in_range = [&](int t) { return mm && t * 16 + li < v && col0 < D; };
    auto load_tile = [&](const float* base, int ld, int t) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (in_range(t)) x = *reinterpret_cast<const f32x4*>(base + ((size_t)g * v + t * 16 + li) * ld + col0);
        return x;
    };
    auto store_tile = [&](float* base, int ld, int t, f32x4 x) {
        if (in_range(t)) *reinterpret_cast<f32x4*>(base + ((size_t)g * v + t * 16 + li) * ld + col0) = x;
    };

    dense_load_adjacency<E, NW>(Abuf, a.A, v, tid);
    f32x4 gt[2] = {load_tile(a.d_out, D, 0), load_tile(a.d_out, D, 1)};

    const int nth = tile_w_nth<D, FMT>(tile);
    const unsigned w_base = tile_w_base<D, FMT>(li, kq, tile), wr_base = tile_wr_base<D, FMT>(li, kq, tile);
    const unsigned w_cst = tile_w_cst(nth), w_pst = (unsigned)SC::NC2 * w_cst;                     // chunk / plane pitch in bytes
    auto load_w = [&](TileW<D, FMT>& w, const float* gimg) { ggnn::load_w<D, FMT>(w, gimg, w_base, w_cst, w_pst, wr_base, nth); };
    auto mma_pair = [&](auto zero_c, f32x4 (&acc)[2], const float* blk, const TileW<D, FMT>& w) {
        ggnn::mma_pair<D, FMT, decltype(zero_c)::value>(acc, blk, w, li, kq);
    };
    TileW<D, FMT> tw[2];
    if (mm) load_w(tw[0], image(0));

    for (int step = a.steps - 1; step >= 0; --step) {
        const int rstep = a.steps - 1 - step;
        const bool last = step == 0;
        const float* sv = a.saved + (size_t)step * bv * D;             // this timestep's [b v, D] block of tensor 0; tensor k: + k TS
        const size_t TS = (size_t)a.steps * bv * D;                    // (saved [6][steps][b v, D]: h_t | x_t | r | u | c | r*h)
        float* o_dpc = a.dpc + (size_t)step * bv * D;
        float* o_dpg = a.dpg + (size_t)step * bv * 2 * D;
        GGNN_DENSE_STAMP(rstep, 0)
        // ---- the pre-activation gradients of the candidate and of the update gate ------------------------------------------------
        f32x4 ht[2], ut[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            ht[t] = load_tile(sv, D, t);
            ut[t] = load_tile(sv + 3 * TS, D, t);
            const f32x4 ct = load_tile(sv + 4 * TS, D, t);
            f32x4 dpc, dpu;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dpc[e] = gt[t][e] * (1.0f - ut[t][e]) * (1.0f - ct[e] * ct[e]);
                dpu[e] = gt[t][e] * (ht[t][e] - ct[e]) * ut[t][e] * (1.0f - ut[t][e]);
            }
            store_tile(o_dpc, D, t, dpc);
            store_tile(o_dpg + D, 2 * D, t, dpu);
            to_planes(Bc, t, dpc);
            to_planes(Bu, t, dpu);
        }
        __syncthreads();                                               // (1) dpc, dpu complete, split (first pass: the adjacency too)
        GGNN_DENSE_STAMP(rstep, 1)
        f32x4 drh[2];
        GGNN_DENSE_STAGE(0, drh, Bc, true)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 rt = load_tile(sv + 2 * TS, D, t);
            f32x4 dpr;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dpr[e] = drh[t][e] * ht[t][e] * rt[e] * (1.0f - rt[e]);
                drh[t][e] *= rt[e];                                    // the state's share through r*h
            }
            store_tile(o_dpg, 2 * D, t, dpr);
            to_planes(Br, t, dpr);
        }
        __syncthreads();                                               // (2) dpr complete, split
        GGNN_DENSE_STAMP(rstep, 2)
        f32x4 dx[2], dh[2];
        GGNN_DENSE_STAGE(1, dx, Br, true)
        GGNN_DENSE_STAGE(2, dx, Bu, false)
        GGNN_DENSE_STAGE(3, dx, Bc, false)
        GGNN_DENSE_STAGE(4, dh, Br, true)
        GGNN_DENSE_STAGE(5, dh, Bu, false)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            store_tile(a.dx + (size_t)step * bv * D, D, t, dx[t]);
            if (mm) to_lds(DXbuf, t, dx[t]);
        }
        GGNN_DENSE_STAMP(rstep, 3)
        __syncthreads();                                               // (3) dx complete; the three operand blocks are free
        GGNN_DENSE_STAMP(rstep, 4)
        // ---- dM_e = A_e^T dx on the matrix pipe (f32, like the forward's aggregation), split into block BI; then dh += dM_e W_e^T ----
#define GGNN_DGB_AGG(EE, BI)                                                                               \
        if constexpr ((EE) < E) {                                                                          \
            f32x4 dm[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};                                    \
            if (mm) {                                                                                      \
                const float* xcol = DXbuf + 16 * tile + li;                                                \
                const float* acol0 = Abuf + ((EE) * 32 + kq) * AP + li;   /* A_e[dst = 4 s4 + kq][src = li] */ \
                _Pragma("unroll")                                                                          \
                for (int s4 = 0; s4 < 8; ++s4) {                                                           \
                    const float wv = xcol[(size_t)(4 * s4 + kq) * MP];                                     \
                    dm[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, acol0[4 * s4 * AP], dm[0], 0, 0, 0);  \
                    dm[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, acol0[4 * s4 * AP + 16], dm[1], 0, 0, 0); \
                }                                                                                          \
            }                                                                                              \
            store_tile(a.dM + (size_t)step * bv * E * D + (EE) * D, E * D, 0, dm[0]);                      \
            store_tile(a.dM + (size_t)step * bv * E * D + (EE) * D, E * D, 1, dm[1]);                      \
            to_planes(Pblk + (size_t)(BI) * PBLK, 0, dm[0]);                                          \
            to_planes(Pblk + (size_t)(BI) * PBLK, 1, dm[1]);                                          \
        }
#define GGNN_DGB_XFORM(EE, BI) if constexpr ((EE) < E) { GGNN_DENSE_STAGE(6 + (EE), dh, Pblk + (size_t)(BI) * PBLK, false) }
#define GGNN_DGB_GROUP(E0)                                                                                 \
        if constexpr ((E0) < E) {                                                                          \
            if constexpr ((E0) > 0) __syncthreads();                   /* the previous group's blocks have been consumed */ \
            GGNN_DGB_AGG((E0) + 0, 0) GGNN_DGB_AGG((E0) + 1, 1) GGNN_DGB_AGG((E0) + 2, 2) GGNN_DGB_AGG((E0) + 3, 3) \
            __syncthreads();                                           /* this group's dM_e complete, split */ \
            GGNN_DGB_XFORM((E0) + 0, 0) GGNN_DGB_XFORM((E0) + 1, 1) GGNN_DGB_XFORM((E0) + 2, 2) GGNN_DGB_XFORM((E0) + 3, 3) \
        }
        GGNN_DGB_GROUP(0)
        GGNN_DENSE_STAMP(rstep, 5)
        GGNN_DGB_GROUP(4)
        GGNN_DENSE_STAMP(rstep, 6)
#undef GGNN_DGB_GROUP
#undef GGNN_DGB_XFORM
#undef GGNN_DGB_AGG
        // ---- g <- dh: the products, the share through r*h, and g u LAST (see the file header) ----------------------------------------
#pragma unroll
        for (int t = 0; t < 2; ++t) gt[t] = (dh[t] + drh[t]) + gt[t] * ut[t];
        GGNN_DENSE_STAMP(rstep, 7)
        if (!last) __syncthreads();                                    // (4) the operand blocks are free for the next pass
    }
    if (a.d_h0) { store_tile(a.d_h0, D, 0, gt[0]); store_tile(a.d_h0, D, 1, gt[1]); }
}

int dense_bwd_supported(int v, int E, int D) {
    return dense_split_supported(v, E, D) && dense_dispatch(D, E, [](auto d, auto e) {
        return DenseBwdLds<decltype(d)::value, decltype(e)::value>::BYTES <= kDenseLdsLimit; });
}

size_t dense_bwd_packed_bytes(int D, int E) {
    if (E <= 0) return 0;
    return dense_for_D(D, [&](auto d) { return (size_t)(6 + E) * SplitCfg<decltype(d)::value>::IMG_BYTES; });
}

}  // namespace ggnn

using namespace ggnn;

extern "C" size_t ggnn_dense_bwd_packed_bytes(int D, int E) { return dense_bwd_packed_bytes(D, E); }

extern "C" int ggnn_dense_bwd_pack_f32(const float* W, const float* Wg, const float* Wc, int E, int D, float* packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(W && Wg && Wc && packed && aligned16(packed) && E > 0 && E <= 64, "null or misaligned pointer, or E = %d outside 1..64", E);
    hipStream_t st = (hipStream_t)stream;
    if (!dense_bwd_packed_bytes(D, E)) return fail(GGNN_E_UNSUPPORTED, "no graph-resident dense backward for hidden size %d", D);
    dense_for_D(D, [&](auto d) {
        hipLaunchKernelGGL((dense_bwd_pack_kernel<decltype(d)::value>), dim3(8, 6 + E), dim3(256), 0, st, W, Wg, Wc, packed);
        return 0; });
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

extern "C" int ggnn_dense_propagate_bwd_f32(const float* d_out, const float* A, const float* bwd_packed, const float* saved, int b, int v,
                                            int E, int D, int steps, float* d_h0, float* dpc, float* dpg, float* dx, float* dM,
                                            ggnn_stream_t stream) {
    GGNN_CHECK_ARG(b >= 0 && steps >= 1, "bad sizes b=%d steps=%d", b, steps);
    if (!ggnn_dense_train_supported(v, E, D))
        return fail(GGNN_E_UNSUPPORTED, "graph-resident dense backward: split matrix path, v <= 32, E in {2,4,6,8}, hidden size 32/64/100 "
                                        "(got v=%d E=%d D=%d)", v, E, D);
    if (b == 0) return GGNN_OK;
    GGNN_CHECK_ARG(d_out && A && bwd_packed && saved && dpc && dpg && dx && dM, "null pointer");
    GGNN_CHECK_ARG(aligned16(d_out) && aligned16(bwd_packed) && aligned16(saved) && aligned16(dpc) && aligned16(dpg) && aligned16(dx) &&
                   aligned16(dM) && (!d_h0 || aligned16(d_h0)), "pointers must be 16-byte aligned");
    const DenseGraphBwdArgs a{d_out, A, bwd_packed, saved, d_h0, dpc, dpg, dx, dM, b, v, steps, stamp_ptr_from_env("GGNN_DGB_TPTR")};
    hipStream_t st = (hipStream_t)stream;
    return dense_dispatch(D, E, [&](auto d, auto e) {
        constexpr int DD = decltype(d)::value, EE = decltype(e)::value;
        return dense_graph_launch<&ggnn_dense_graph_bwd_kernel<DD, EE, kDenseWaves>>(DenseBwdLds<DD, EE>::BYTES, a, st); });
}
