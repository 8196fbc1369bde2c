// K7, training: the backward of the graph-resident dense GGNN forward (chem_tensorflow_dense.py:93-117; what TF autodiff derives from
// it through compute_gradients, chem_tensorflow.py:184).  One workgroup per graph walks the timesteps in REVERSE on what the saving
// forward launch wrote (ggnn_dense_graph_split.hip, SAVE): the gradient of the graph's states never leaves its CU.
//
// The structure is the forward's: operands in LDS already split into MFMA planes ([plane][32-chunk][lane group][row][8 x bf16], written
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
#include "ggnn_split.hpp"
#include <type_traits>

namespace ggnn {

namespace {

// this wave's column tile of one bf16x3 split stage image: three planes x NC2 chunks of 8 halves per lane + the remainder rows
template <int D>
struct TileWB {
    u32x4 p[3][SplitCfg<D>::NC2 > 0 ? SplitCfg<D>::NC2 : 1];
    float r[StageCfg<D>::NR > 0 ? StageCfg<D>::NR : 1];
};

}  // namespace

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
    constexpr int NP = 3;
    constexpr int NT = C::NT, NC = C::NC, NR = C::NR, NC2 = SC::NC2;
    constexpr int MP = C::BN + 4;                                      // row pitch of the f32 dx block (floats)
    constexpr int NS = E + 6;                                          // stages per timestep
    constexpr int AP = 33;
    constexpr int PSLOT = 32 * 4;                                      // floats of one (plane, chunk, g) slab: 32 rows x 16 bytes
    constexpr int PBLK = NP * NC2 * 4 * PSLOT + 32 * 4;                // floats of one split operand block (+ the remainder columns [32][4])
    constexpr int NB = 4;                                              // operand blocks: dpc | dpu | dpr, then four dM_e at a time
    static_assert(NT <= NW && NS % 2 == 0 && NR <= 1, "one column tile per wave; two weight slots with a fixed phase per timestep");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* DXbuf = lds;                                                // [32][MP] f32: dx, the aggregation's operand
    float* Pblk = DXbuf + 32 * MP;                                     // [NB] split operand blocks
    float* Abuf = Pblk + (size_t)NB * PBLK;                            // [E][32][AP] adjacency rows
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

    auto tile_to_lds = [&](float* blk, int t, f32x4 val) {
        *reinterpret_cast<f32x4*>(blk + (size_t)(t * 16 + li) * MP + 16 * tile + 4 * kq) = val;
    };
    // this wave's four columns of row tile t, split, into an operand block (the forward's slot arithmetic)
    auto tile_to_planes = [&](float* blk, int t, f32x4 val) {
        if (!mm) return;
        const int row = t * 16 + li;
        if (tail) {
            if (kq == 0) *reinterpret_cast<f32x4*>(blk + NP * NC2 * 4 * PSLOT + row * 4) = val;      // f32 remainder columns
            return;
        }
        unsigned h0, m0, l0, h1, m1, l1;
        split_pair<kSplitBf16x3>(val.x, val.y, h0, m0, l0);
        split_pair<kSplitBf16x3>(val.z, val.w, h1, m1, l1);
        const int c2 = tile >> 1;
        float* dst = blk + ((size_t)(c2 * 4 + kq)) * PSLOT + row * 4 + 2 * (tile & 1);
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<u32x2*>(dst) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(dst + NC2 * 4 * PSLOT) = u32x2{m0, m1};
        *reinterpret_cast<u32x2*>(dst + 2 * NC2 * 4 * PSLOT) = u32x2{l0, l1};
    };
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

    for (int idx = tid; idx < E * 32 * 32; idx += NW * 64) {
        const int j = idx & 31, i = (idx >> 5) & 31, e = idx >> 10;
        Abuf[(e * 32 + i) * AP + j] = (i < a.v && j < a.v) ? a.A[(((size_t)blockIdx.x * E + e) * a.v + i) * a.v + j] : 0.f;
    }
    f32x4 gt[2] = {load_tile(a.d_out, D, 0), load_tile(a.d_out, D, 1)};

    // byte offsets of this wave's weight slice inside a split image (two column halves, ggnn_split.hpp)
    const bool hb = tile >= SC::TA;
    const int nth = hb ? NT - SC::TA : SC::TA, til = hb ? tile - SC::TA : tile;
    const unsigned w_base = (hb ? (unsigned)SC::HA_BYTES : 0u) + (unsigned)(kq * nth * 16 + li + til * 16) * 16u;
    const unsigned w_cst = (unsigned)(4 * nth * 16) * 16u, w_pst = (unsigned)NC2 * w_cst;          // chunk / plane pitch in bytes
    const unsigned wr_base = (hb ? (unsigned)SC::HA_BYTES : 0u) + (unsigned)NP * w_pst + (unsigned)(kq * nth * 16 + li + til * 16) * 4u;
    auto load_w = [&](TileWB<D>& w, const float* gimg) {
        const unsigned long long p = reinterpret_cast<unsigned long long>(gimg);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
        const float* sb = reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2)
                w.p[pl][c2] = __builtin_bit_cast(u32x4, ld4_b(sb, w_base + (unsigned)pl * w_pst + (unsigned)c2 * w_cst));
#pragma unroll
        for (int q = 0; q < NR; ++q) w.r[q] = ld1_b(sb, wr_base + (unsigned)(q * 4 * nth * 16) * 4u);
    };
    // both row tiles of an operand block against one weight slice: per chunk 6 operand reads feed 12 MFMAs (two accumulator chains)
    auto mma_pair = [&](auto zero_c, f32x4 (&acc)[2], const float* blk, const TileWB<D>& w) {
        constexpr bool ZERO = decltype(zero_c)::value;
        f32x4 c0 = acc[0], c1 = acc[1];
        if constexpr (ZERO) { c0 = f32x4{0.f, 0.f, 0.f, 0.f}; c1 = c0; }
        const u32x4* ob = reinterpret_cast<const u32x4*>(blk) + kq * 32 + li;            // (plane, chunk) slabs are 128 slots apart
#pragma unroll
        for (int c2 = 0; c2 < NC2; ++c2) {
            const u32x4 ah0 = ob[(0 * NC2 + c2) * 128], ah1 = ob[(0 * NC2 + c2) * 128 + 16];
            const u32x4 am0 = ob[(1 * NC2 + c2) * 128], am1 = ob[(1 * NC2 + c2) * 128 + 16];
            const u32x4 al0 = ob[(2 * NC2 + c2) * 128], al1 = ob[(2 * NC2 + c2) * 128 + 16];
            const u32x4 wh = w.p[0][c2], wm = w.p[1][c2], wl = w.p[2][c2];
            c0 = mfma_bf16(wl, ah0, c0); c1 = mfma_bf16(wl, ah1, c1);
            c0 = mfma_bf16(wm, am0, c0); c1 = mfma_bf16(wm, am1, c1);
            c0 = mfma_bf16(wm, ah0, c0); c1 = mfma_bf16(wm, ah1, c1);
            c0 = mfma_bf16(wh, al0, c0); c1 = mfma_bf16(wh, al1, c1);
            c0 = mfma_bf16(wh, am0, c0); c1 = mfma_bf16(wh, am1, c1);
            c0 = mfma_bf16(wh, ah0, c0); c1 = mfma_bf16(wh, ah1, c1);
        }
        if constexpr (NR > 0) {
            const float* rb = blk + NP * NC2 * 4 * PSLOT;                                  // [32][4] remainder columns
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[0], rb[li * 4 + kq], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[0], rb[(16 + li) * 4 + kq], c1, 0, 0, 0);
        }
        acc[0] = c0; acc[1] = c1;
    };
    TileWB<D> tw[2];
    if (mm) load_w(tw[0], a.img);

#define GGNN_DGB_T(K) if (a.tdbg && blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 6) && rstep < 8) \
        a.tdbg[(rstep * 2 + (wave ? 1 : 0)) * 8 + (K)] = __builtin_amdgcn_s_memtime();
    for (int step = a.steps - 1; step >= 0; --step) {
        const int rstep = a.steps - 1 - step;
        const bool last = step == 0;
        const float* sv = a.saved + (size_t)step * bv * D;             // this timestep's [b v, D] block of tensor 0; tensor k: + k TS
        const size_t TS = (size_t)a.steps * bv * D;                    // (saved [6][steps][b v, D]: h_t | x_t | r | u | c | r*h)
        float* o_dpc = a.dpc + (size_t)step * bv * D;
        float* o_dpg = a.dpg + (size_t)step * bv * 2 * D;
        GGNN_DGB_T(0)
#define GGNN_DGB_STAGE(S, ACC, BLK, ZERO)                                                                  \
        {                                                                                                  \
            __builtin_amdgcn_sched_barrier(0);   /* (the look-ahead stays at ONE stage, as in the forward) */ \
            if (mm && !(last && (S) + 1 == NS)) load_w(tw[((S) + 1) & 1], a.img + (size_t)(((S) + 1) % NS) * SC::IMG); \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            if (mm) mma_pair(std::integral_constant<bool, ZERO>{}, ACC, BLK, tw[(S) & 1]);                 \
            __builtin_amdgcn_sched_barrier(0);                                                             \
        }
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
            tile_to_planes(Bc, t, dpc);
            tile_to_planes(Bu, t, dpu);
        }
        __syncthreads();                                               // (1) dpc, dpu complete, split (first pass: the adjacency too)
        GGNN_DGB_T(1)
        f32x4 drh[2];
        GGNN_DGB_STAGE(0, drh, Bc, true)
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
            tile_to_planes(Br, t, dpr);
        }
        __syncthreads();                                               // (2) dpr complete, split
        GGNN_DGB_T(2)
        f32x4 dx[2], dh[2];
        GGNN_DGB_STAGE(1, dx, Br, true)
        GGNN_DGB_STAGE(2, dx, Bu, false)
        GGNN_DGB_STAGE(3, dx, Bc, false)
        GGNN_DGB_STAGE(4, dh, Br, true)
        GGNN_DGB_STAGE(5, dh, Bu, false)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            store_tile(a.dx + (size_t)step * bv * D, D, t, dx[t]);
            if (mm) tile_to_lds(DXbuf, t, dx[t]);
        }
        GGNN_DGB_T(3)
        __syncthreads();                                               // (3) dx complete; the three operand blocks are free
        GGNN_DGB_T(4)
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
            tile_to_planes(Pblk + (size_t)(BI) * PBLK, 0, dm[0]);                                          \
            tile_to_planes(Pblk + (size_t)(BI) * PBLK, 1, dm[1]);                                          \
        }
#define GGNN_DGB_XFORM(EE, BI) if constexpr ((EE) < E) { GGNN_DGB_STAGE(6 + (EE), dh, Pblk + (size_t)(BI) * PBLK, false) }
#define GGNN_DGB_GROUP(E0)                                                                                 \
        if constexpr ((E0) < E) {                                                                          \
            if constexpr ((E0) > 0) __syncthreads();                   /* the previous group's blocks have been consumed */ \
            GGNN_DGB_AGG((E0) + 0, 0) GGNN_DGB_AGG((E0) + 1, 1) GGNN_DGB_AGG((E0) + 2, 2) GGNN_DGB_AGG((E0) + 3, 3) \
            __syncthreads();                                           /* this group's dM_e complete, split */ \
            GGNN_DGB_XFORM((E0) + 0, 0) GGNN_DGB_XFORM((E0) + 1, 1) GGNN_DGB_XFORM((E0) + 2, 2) GGNN_DGB_XFORM((E0) + 3, 3) \
        }
        GGNN_DGB_GROUP(0)
        GGNN_DGB_T(5)
        GGNN_DGB_GROUP(4)
        GGNN_DGB_T(6)
#undef GGNN_DGB_GROUP
#undef GGNN_DGB_XFORM
#undef GGNN_DGB_AGG
#undef GGNN_DGB_STAGE
        // ---- g <- dh: the products, the share through r*h, and g u LAST (see the file header) ----------------------------------------
#pragma unroll
        for (int t = 0; t < 2; ++t) gt[t] = (dh[t] + drh[t]) + gt[t] * ut[t];
        GGNN_DGB_T(7)
        if (!last) __syncthreads();                                    // (4) the operand blocks are free for the next pass
    }
#undef GGNN_DGB_T
    if (a.d_h0) { store_tile(a.d_h0, D, 0, gt[0]); store_tile(a.d_h0, D, 1, gt[1]); }
}

static size_t bwd_lds_bytes(int D, int E) {
    const int bn = (D + 15) / 16 * 16, nc2 = (D / 16) / 2;
    const size_t pblk = (size_t)3 * nc2 * 4 * 128 + 128;
    return ((size_t)32 * (bn + 4) + 4 * pblk + (size_t)E * 32 * 33) * sizeof(float);
}

int dense_bwd_supported(int v, int E, int D) {
    return dense_split_supported(v, E, D) && bwd_lds_bytes(D, E) <= (size_t)160 * 1024;
}

size_t dense_bwd_packed_bytes(int D, int E) {
    if (E <= 0) return 0;
    switch (D) {
        case 100: return (size_t)(6 + E) * SplitCfg<100>::IMG_BYTES;
        case 64: return (size_t)(6 + E) * SplitCfg<64>::IMG_BYTES;
        case 32: return (size_t)(6 + E) * SplitCfg<32>::IMG_BYTES;
        default: return 0;
    }
}

template <int D, int E>
static int launch_bwd(const DenseGraphBwdArgs& a, hipStream_t st) {
    constexpr int NW = 8;
    const size_t ldsb = bwd_lds_bytes(D, E);
    static std::atomic<unsigned long long> lds_ok{0};
    if (ldsb > 64 * 1024) GGNN_CHECK_HIP((allow_dynamic_lds(&ggnn_dense_graph_bwd_kernel<D, E, NW>, ldsb, lds_ok)));
    hipLaunchKernelGGL((ggnn_dense_graph_bwd_kernel<D, E, NW>), dim3(a.b), dim3(NW * 64), ldsb, st, a);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

}  // namespace ggnn

using namespace ggnn;

extern "C" size_t ggnn_dense_bwd_packed_bytes(int D, int E) { return dense_bwd_packed_bytes(D, E); }

extern "C" int ggnn_dense_bwd_pack_f32(const float* W, const float* Wg, const float* Wc, int E, int D, float* packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(W && Wg && Wc && packed && aligned16(packed) && E > 0 && E <= 64, "null or misaligned pointer, or E = %d outside 1..64", E);
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: hipLaunchKernelGGL((dense_bwd_pack_kernel<100>), dim3(8, 6 + E), dim3(256), 0, st, W, Wg, Wc, packed); break;
        case 64: hipLaunchKernelGGL((dense_bwd_pack_kernel<64>), dim3(8, 6 + E), dim3(256), 0, st, W, Wg, Wc, packed); break;
        case 32: hipLaunchKernelGGL((dense_bwd_pack_kernel<32>), dim3(8, 6 + E), dim3(256), 0, st, W, Wg, Wc, packed); break;
        default: return fail(GGNN_E_UNSUPPORTED, "no graph-resident dense backward for hidden size %d", D);
    }
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
    DenseGraphBwdArgs a{d_out, A, bwd_packed, saved, d_h0, dpc, dpg, dx, dM, b, v, steps, nullptr};
    { const char* e = getenv("GGNN_DGB_TPTR"); a.tdbg = e ? (unsigned long long*)strtoull(e, nullptr, 10) : nullptr; }
    hipStream_t st = (hipStream_t)stream;
#define GGNN_DGB_CASE(DD, EE) if (D == DD && E == EE) return launch_bwd<DD, EE>(a, st);
    GGNN_DGB_CASE(100, 4) GGNN_DGB_CASE(100, 2) GGNN_DGB_CASE(100, 6) GGNN_DGB_CASE(100, 8)
    GGNN_DGB_CASE(64, 4) GGNN_DGB_CASE(64, 8) GGNN_DGB_CASE(64, 2) GGNN_DGB_CASE(64, 6)
    GGNN_DGB_CASE(32, 4) GGNN_DGB_CASE(32, 8) GGNN_DGB_CASE(32, 2) GGNN_DGB_CASE(32, 6)
#undef GGNN_DGB_CASE
    return fail(GGNN_E_UNSUPPORTED, "graph-resident dense backward: unsupported shape");
}
