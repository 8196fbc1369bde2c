// The shared tile layer of the graph-resident dense GGNN kernels:
//     ggnn_dense_graph.hip        f32-MFMA forward
//     ggnn_dense_graph_split.hip  split forward (bf16x3 / f16x2, plain and SAVE)
//     ggnn_dense_graph_bwd.hip    backward of all timesteps in one launch
// What the three have in common lives here, each piece once: the argument structs, the LDS layout of every kernel (the kernel carves
// its blocks from it, the launch sizes its dynamic LDS from it, the *_supported queries take the fit test from it), the split operand
// tile (TileW, the weight-slice offsets, load_w, tile_to_planes, mma_pair), the adjacency / bias / in-degree prologue, the forward
// aggregation, the stage and stamp macros, and the host dispatch over the supported (D, E) pairs.  The .hip files keep what is
// theirs: the stage order, the gate math, the SAVE stores, the backward's formulas.
// Device helpers are free __forceinline__ functions that take the lane coordinates BY VALUE: the same code as members of an object
// holding the coordinates costs registers and made the compiler duplicate the split forward's timestep body.  What sits between the
// stages of a timestep (the stage itself, the aggregation) is a macro: the compiler then sees it in the kernel, as before.
// profiles/dense_tile_refactor_codegen.json has every kernel's registers, scratch, MFMA and instruction counts before and after.
#pragma once
#include "ggnn_common.h"
#include "ggnn_split.hpp"
#include <cstdlib>
#include <type_traits>

namespace ggnn {

struct DenseGraphArgs {
    const float* h0;        // [b, v, D]
    const float* A;         // [b, E, v, v]  A[g,e,dst,src]
    const float* eimg;      // E stage images of W_e            (ggnn_dense_edge_pack_f32; the split kernel: E split images)
    const float* gimg;      // 6 stage images: Wg[x,r] Wg[h,r] Wg[x,u] Wg[h,u] Wc[x] Wc[h]   (dense_gru_pack_kernel)
    const float* ebias;     // [E, D] or NULL
    const float* bg;        // [2D]
    const float* bc;        // [D]
    float* out;             // [b, v, D]
    int b, v, steps;
    unsigned long long* tdbg;   // (debug) s_memtime stamps of workgroup 0, waves 0 and 6: [step][wave sel][8]   (GGNN_DG_TPTR)
    float* saved;           // (training; split kernel only) [6][steps][b v, D]: h_t, x_t, r, u, c, r*h -- or NULL
};

// the backward of the launch above (ggnn_dense_graph_bwd.hip): one workgroup per graph walks the timesteps in reverse
struct DenseGraphBwdArgs {
    const float* d_out;     // [b, v, D]  dL/dh_steps
    const float* A;         // [b, E, v, v]
    const float* img;       // 6 + E transposed split images (dense_bwd_pack)
    const float* saved;     // what the saving forward wrote
    float* d_h0;            // [b, v, D] or NULL
    float* dpc;             // [steps, b v, D]
    float* dpg;             // [steps, b v, 2D] = [dpr | dpu]
    float* dx;              // [steps, b v, D]
    float* dM;              // [steps, b v, E D]
    int b, v, steps;
    unsigned long long* tdbg;   // (debug) s_memtime stamps of workgroup 0, waves 0 and 6: [step][wave sel][8]   (GGNN_DGB_TPTR)
};

// split form (ggnn_dense_graph_split.hip): 1 when the kernel exists for the shape and its LDS blocks fit
int dense_split_supported(int v, int E, int D);
size_t dense_split_edge_bytes(int D, int T);      // bytes of the split section of the edge images: T bf16x3 images, then T f16x2 images
size_t dense_split_gru_bytes(int D);              // ... of the six GRU images, in the split kernel's stage order (both formats)
size_t dense_split_images_offset(int D, int T, int fmt);   // byte offset of the images of format `fmt` inside a split section of T images
int dense_split_pack_edge(const float* W, int T, int D, float* packed, hipStream_t st);
int dense_split_pack_gru(const float* Wg, const float* Wc, int D, float* packed, hipStream_t st);
int dense_split_launch(const DenseGraphArgs& a, int E, int D, int fmt, hipStream_t st);
int dense_bwd_supported(int v, int E, int D);     // the backward kernel exists for the shape and its LDS blocks fit
size_t dense_bwd_packed_bytes(int D, int E);

// ---- host: the shapes of the family ---------------------------------------------------------------------------------------------------
constexpr int kDenseWaves = 8;                          // waves of a workgroup: one column tile each (NT <= 7)
constexpr size_t kDenseLdsLimit = (size_t)160 * 1024;   // bytes of LDS one workgroup of a gfx950 CU can have

// a graph of v padded vertices, E edge types, hidden size D has kernels in this family
inline bool dense_shape_ok(int v, int E, int D) {
    return v >= 1 && v <= 32 && (E == 2 || E == 4 || E == 6 || E == 8) && (D == 100 || D == 64 || D == 32);
}

// f(std::integral_constant<int, D>{}) for the three hidden sizes; a value-initialised result for any other D
template <class F>
inline auto dense_for_D(int D, F&& f) -> decltype(f(std::integral_constant<int, 100>{})) {
    switch (D) {
        case 100: return f(std::integral_constant<int, 100>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 32: return f(std::integral_constant<int, 32>{});
        default: return {};
    }
}
// f(integral_constant D, integral_constant E) for the 12 supported pairs; a value-initialised result for any other
template <class F>
inline auto dense_dispatch(int D, int E, F&& f) -> decltype(f(std::integral_constant<int, 100>{}, std::integral_constant<int, 2>{})) {
    return dense_for_D(D, [&](auto d) -> decltype(f(d, std::integral_constant<int, 2>{})) {
        switch (E) {
            case 2: return f(d, std::integral_constant<int, 2>{});
            case 4: return f(d, std::integral_constant<int, 4>{});
            case 6: return f(d, std::integral_constant<int, 6>{});
            case 8: return f(d, std::integral_constant<int, 8>{});
            default: return {};
        }
    });
}

// the debug stamp buffer of a launch: a device pointer in decimal in the environment variable `name`, or NULL
inline unsigned long long* stamp_ptr_from_env(const char* name) {
    const char* e = getenv(name);
    return e ? (unsigned long long*)strtoull(e, nullptr, 10) : nullptr;
}

// one workgroup per graph, kDenseWaves waves, `lds_bytes` of dynamic LDS (the limit is raised once per kernel and device)
template <auto Kernel, class Args>
inline int dense_graph_launch(size_t lds_bytes, const Args& a, hipStream_t st) {
    static std::atomic<unsigned long long> lds_ok{0};
    if (lds_bytes > 64 * 1024) GGNN_CHECK_HIP((allow_dynamic_lds(Kernel, lds_bytes, lds_ok)));
    hipLaunchKernelGGL(Kernel, dim3(a.b), dim3(kDenseWaves * 64), lds_bytes, st, a);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

// ---- tile geometry and the LDS layouts (offsets in floats) ----------------------------------------------------------------------------
template <int D, int FMT = kSplitBf16x3>
struct DenseTile {
    static constexpr int BN = StageCfg<D>::BN;
    static constexpr int MP = BN + 4;                      // row pitch of an f32 [32][MP] block
    static constexpr int AP = 33;                          // pitch of an adjacency row (16 rows x one column: 16 banks)
    static constexpr int PSLOT = 32 * 4;                   // floats of one (plane, chunk, g) slab of a split operand block: 32 rows x 16 bytes
    static constexpr int PMAIN = SplitFmt<FMT>::NP * SplitCfg<D, FMT>::NC2 * 4 * PSLOT;   // the planes [plane][32-chunk][g][row][8 halves]
    static constexpr int PBLK = PMAIN + 32 * 4;            // one split operand block: the planes + the f32 remainder columns [32][4]
};

// f32 forward: M_e [E][32][MP] | exchange blocks acts, r*h, new state [32][MP] | adjacency rows [E][32][AP] | in-degrees [E][32] | edge
// biases [E][BN], zero-padded.  (One exchange block each, so that a block is rewritten a whole timestep after it was last read and
// "everyone has read it" needs no barrier of its own.)
template <int D, int E>
struct DenseF32Lds {
    using T = DenseTile<D>;
    static constexpr int M = 0, X = M + E * 32 * T::MP, R = X + 32 * T::MP, H = R + 32 * T::MP, A = H + 32 * T::MP,
                         N = A + E * 32 * T::AP, B = N + E * 32, END = B + E * T::BN;
    static constexpr size_t BYTES = (size_t)END * sizeof(float);
};
// split forward: M_e [E][32][MP] f32 | split operand blocks state, aggregated messages, r*h | adjacency | in-degrees | edge biases
template <int D, int E, int FMT>
struct DenseSplitLds {
    using T = DenseTile<D, FMT>;
    static constexpr int M = 0, H = M + E * 32 * T::MP, X = H + T::PBLK, R = X + T::PBLK, A = R + T::PBLK,
                         N = A + E * 32 * T::AP, B = N + E * 32, END = B + E * T::BN;
    static constexpr size_t BYTES = (size_t)END * sizeof(float);
};
// backward: dx [32][MP] f32 | NB split operand blocks (dpc | dpu | dpr, then four dM_e at a time) | adjacency
template <int D, int E>
struct DenseBwdLds {
    using T = DenseTile<D>;
    static constexpr int NB = 4;
    static constexpr int DX = 0, P = DX + 32 * T::MP, A = P + NB * T::PBLK, END = A + E * 32 * T::AP;
    static constexpr size_t BYTES = (size_t)END * sizeof(float);
};

// ---- device: prologue pieces ------------------------------------------------------------------------------------------------------------
// the adjacency rows of graph blockIdx.x, zero outside its v vertices: read once, used by every timestep
template <int E, int NW>
__device__ __forceinline__ void dense_load_adjacency(float* Abuf, const float* A, int v, int tid) {
    constexpr int AP = DenseTile<32>::AP;
    for (int idx = tid; idx < E * 32 * 32; idx += NW * 64) {
        const int j = idx & 31, i = (idx >> 5) & 31, e = idx >> 10;
        Abuf[(e * 32 + i) * AP + j] = (i < v && j < v) ? A[(((size_t)blockIdx.x * E + e) * v + i) * v + j] : 0.f;
    }
}
// the edge biases [E][BN], zero-padded (all zero without biases)
template <int D, int E, int NW>
__device__ __forceinline__ void dense_load_edge_bias(float* Bbuf, const float* ebias, int tid) {
    constexpr int BN = StageCfg<D>::BN;
    for (int idx = tid; idx < E * BN; idx += NW * 64) {
        const int e = idx / BN, n = idx - e * BN;
        Bbuf[idx] = (ebias && n < D) ? ebias[(size_t)e * D + n] : 0.f;
    }
}
// incoming edges per (type, vertex): the row sums of A_e (after the barrier that completes Abuf)
template <int E>
__device__ __forceinline__ void dense_in_degrees(float* Nbuf, const float* Abuf, int tid) {
    constexpr int AP = DenseTile<32>::AP;
    if (tid < E * 32) {
        float sum = 0.f;
        for (int j = 0; j < 32; ++j) sum += Abuf[tid * AP + j];
        Nbuf[tid] = sum;
    }
}
// this lane's four columns col0 .. of the gate / candidate biases
template <int D>
__device__ __forceinline__ void dense_gate_bias(f32x4& b_r, f32x4& b_u, f32x4& b_c, const float* bg, const float* bc, int col0) {
    b_r = f32x4{0.f, 0.f, 0.f, 0.f}; b_u = b_r; b_c = b_r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (col0 + e < D) { b_r[e] = bg[col0 + e]; b_u[e] = bg[D + col0 + e]; b_c[e] = bc[col0 + e]; }
    }
}
// stage s of a forward timestep: the E edge images, then the six GRU images (IMG floats each)
template <int E, int IMG>
__device__ __forceinline__ const float* dense_stage_image(const DenseGraphArgs& a, int s) {
    return s < E ? a.eimg + (size_t)s * IMG : a.gimg + (size_t)(s - E) * IMG;
}

// accumulator tile (lane (li,kq): row t*16+li, columns 16*tile + 4kq ..) -> f32 [32][MP] LDS block
template <int D>
__device__ __forceinline__ void tile_to_lds(float* blk, int t, f32x4 val, int li, int kq, int tile) {
    *reinterpret_cast<f32x4*>(blk + (size_t)(t * 16 + li) * DenseTile<D>::MP + 16 * tile + 4 * kq) = val;
}

// ---- device: the split operand tile (split forward: FMT per launch; backward: kSplitBf16x3) -------------------------------------------
// The activations of a stage group sit in LDS ALREADY SPLIT, in the MFMA operand layout [plane][32-chunk][lane group g][row][8 halves].
// The PRODUCER splits: a wave owns column tile `tile` of every block, i.e. the four k values 16 tile + 4 kq .. of rows li and li + 16
// -- exactly slots 4 (tile & 1) .. + 3 of lane group kq in chunk tile >> 1.

// this wave's column tile of one split stage image: NP planes (three bf16 / two f16) x NC2 chunks of 8 halves per lane + the remainder rows
template <int D, int FMT>
struct TileW {
    u32x4 p[SplitFmt<FMT>::NP][SplitCfg<D>::NC2 > 0 ? SplitCfg<D>::NC2 : 1];
    float r[StageCfg<D>::NR > 0 ? StageCfg<D>::NR : 1];
};

// this wave's weight slice inside a split image (two column halves, ggnn_split.hpp), as byte offsets: nth = the tiles of its half,
// the chunk pitch w_cst = 4 nth 16 slots of 16 bytes, the plane pitch w_pst = NC2 chunks, w_base = this lane's first slot, wr_base =
// its first remainder float.  Plain values the kernel computes ONCE and hands to load_w (not members of an object, see the top).
template <int D, int FMT>
__device__ __forceinline__ int tile_w_nth(int tile) {
    using SC = SplitCfg<D, FMT>;
    return tile >= SC::TA ? StageCfg<D>::NT - SC::TA : SC::TA;
}
__device__ __forceinline__ unsigned tile_w_cst(int nth) { return (unsigned)(4 * nth * 16) * 16u; }
template <int D, int FMT>
__device__ __forceinline__ unsigned tile_w_base(int li, int kq, int tile) {
    using SC = SplitCfg<D, FMT>;
    const bool hb = tile >= SC::TA;
    const int nth = tile_w_nth<D, FMT>(tile), til = hb ? tile - SC::TA : tile;
    return (hb ? (unsigned)SC::HA_BYTES : 0u) + (unsigned)(kq * nth * 16 + li + til * 16) * 16u;
}
template <int D, int FMT>
__device__ __forceinline__ unsigned tile_wr_base(int li, int kq, int tile) {
    using SC = SplitCfg<D, FMT>;
    const bool hb = tile >= SC::TA;
    const int nth = tile_w_nth<D, FMT>(tile), til = hb ? tile - SC::TA : tile;
    const unsigned w_pst = (unsigned)SC::NC2 * tile_w_cst(nth);
    return (hb ? (unsigned)SC::HA_BYTES : 0u) + (unsigned)SC::NP * w_pst + (unsigned)(kq * nth * 16 + li + til * 16) * 4u;
}
// the slice straight from L2: a scalar base + ONE per-lane byte offset for every image
template <int D, int FMT>
__device__ __forceinline__ void load_w(TileW<D, FMT>& w, const float* gimg, unsigned w_base, unsigned w_cst, unsigned w_pst, unsigned wr_base,
                                       int nth) {
    constexpr int NP = SplitFmt<FMT>::NP, NC2 = SplitCfg<D, FMT>::NC2, NR = StageCfg<D>::NR;
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
}

// this wave's four columns of row tile t, split, into an operand block: 22 vector instructions and three ds_write_b64 (bf16x3)
template <int D, int FMT>
__device__ __forceinline__ void tile_to_planes(float* blk, int t, f32x4 val, int li, int kq, int tile, bool mm, bool tail) {
    using T = DenseTile<D, FMT>;
    constexpr int NP = SplitFmt<FMT>::NP, PLANE = SplitCfg<D, FMT>::NC2 * 4 * T::PSLOT;
    if (!mm) return;
    const int row = t * 16 + li;
    if (tail) {
        if (kq == 0) *reinterpret_cast<f32x4*>(blk + T::PMAIN + row * 4) = val;                      // f32 remainder columns
        return;
    }
    unsigned h0, m0, l0, h1, m1, l1;
    split_pair<FMT>(val.x, val.y, h0, m0, l0);
    split_pair<FMT>(val.z, val.w, h1, m1, l1);
    const int c2 = tile >> 1;
    float* dst = blk + ((size_t)(c2 * 4 + kq)) * T::PSLOT + row * 4 + 2 * (tile & 1);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u32x2*>(dst) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(dst + PLANE) = u32x2{m0, m1};
    if constexpr (NP > 2) *reinterpret_cast<u32x2*>(dst + 2 * PLANE) = u32x2{l0, l1};
}

// both row tiles of an operand block against one weight slice: per chunk 6 operand reads feed 12 MFMAs (two accumulator chains)
template <int D, int FMT, bool ZERO>
__device__ __forceinline__ void mma_pair(f32x4 (&acc)[2], const float* blk, const TileW<D, FMT>& w, int li, int kq) {
    constexpr int NP = SplitFmt<FMT>::NP, NC2 = SplitCfg<D, FMT>::NC2;
    f32x4 c0 = acc[0], c1 = acc[1];
    if constexpr (ZERO) { c0 = f32x4{0.f, 0.f, 0.f, 0.f}; c1 = c0; }
    const u32x4* ob = reinterpret_cast<const u32x4*>(blk) + kq * 32 + li;                // (plane, chunk) slabs are 128 slots apart
#pragma unroll
    for (int c2 = 0; c2 < NC2; ++c2) {
        const u32x4 ah0 = ob[(0 * NC2 + c2) * 128], ah1 = ob[(0 * NC2 + c2) * 128 + 16];
        const u32x4 am0 = ob[(1 * NC2 + c2) * 128], am1 = ob[(1 * NC2 + c2) * 128 + 16];
        if constexpr (FMT == kSplitF16x2) {                            // three products per chunk and row tile, smallest first
            const u32x4 wh = w.p[0][c2], wm = w.p[1][c2];
            c0 = mfma_f16(wm, ah0, c0); c1 = mfma_f16(wm, ah1, c1);
            c0 = mfma_f16(wh, am0, c0); c1 = mfma_f16(wh, am1, c1);
            c0 = mfma_f16(wh, ah0, c0); c1 = mfma_f16(wh, ah1, c1);
            continue;
        }
        const u32x4 al0 = ob[((NP - 1) * NC2 + c2) * 128], al1 = ob[((NP - 1) * NC2 + c2) * 128 + 16];
        const u32x4 wh = w.p[0][c2], wm = w.p[1][c2], wl = w.p[NP - 1][c2];
        c0 = mfma_bf16(wl, ah0, c0); c1 = mfma_bf16(wl, ah1, c1);
        c0 = mfma_bf16(wm, am0, c0); c1 = mfma_bf16(wm, am1, c1);
        c0 = mfma_bf16(wm, ah0, c0); c1 = mfma_bf16(wm, ah1, c1);
        c0 = mfma_bf16(wh, al0, c0); c1 = mfma_bf16(wh, al1, c1);
        c0 = mfma_bf16(wh, am0, c0); c1 = mfma_bf16(wh, am1, c1);
        c0 = mfma_bf16(wh, ah0, c0); c1 = mfma_bf16(wh, ah1, c1);
    }
    if constexpr (StageCfg<D>::NR > 0) {
        const float* rb = blk + DenseTile<D, FMT>::PMAIN;                                  // [32][4] remainder columns
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[0], rb[li * 4 + kq], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[0], rb[(16 + li) * 4 + kq], c1, 0, 0, 0);
    }
    acc[0] = c0; acc[1] = c1;
}

// ---- the stage, aggregation and stamp macros --------------------------------------------------------------------------------------------------------
// One stage S of a timestep of NS stages: request the NEXT stage's weight slice, multiply both row tiles by this stage's.  The three
// sched_barriers keep the look-ahead at ONE stage (25 / 37 weight registers in flight, not ten times that).  The kernel supplies, in
// scope: mm, last, NS, the two weight slots tw[2], image(s) -- where stage s's image comes from --, load_w(slot, image) and
// mma_pair(integral_constant<bool, ZERO>, ACC, OPERAND, slot).
#define GGNN_DENSE_STAGE(S, ACC, OPERAND, ZERO)                                                            \
    {                                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (mm && !(last && (S) + 1 == NS)) load_w(tw[((S) + 1) & 1], image(((S) + 1) % NS));              \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (mm) mma_pair(std::integral_constant<bool, ZERO>{}, ACC, OPERAND, tw[(S) & 1]);                 \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    }
// The forward aggregation of both row tiles into the zeroed accumulators AA[2], for a wave that owns a column tile:
// acts^T tile = sum_e M_e^T[columns of this tile][src] . A_e^T[src][dst] on the matrix pipe (f32: A_e is 0/1, the products are exact),
// K = 32 source vertices = 8 MFMAs per (edge type, row tile); the bias term sum_j A_e[i,j] b_e = nin_e[i] b_e in the epilogue.  (A
// lane-per-column walk over the non-zeros of each adjacency row -- the form of ggnn_dense_aggregate_f32 -- is a chain of dependent LDS
// reads: 9.3k clocks per timestep against 2.5k here.)  In scope: D, E, a, Mbuf, Abuf, Nbuf, Bbuf, li, kq, tile.
// A macro like the stage (and like the backward's transposed product): as a function the compiler arranges the block on its own before
// it meets the kernel, and the f32 kernel pays for the other address arithmetic -- up to +46 registers and +3.6 % instructions.
#define GGNN_DENSE_AGGREGATE(AA)                                                                           \
    {                                                                                                      \
        constexpr int MP_ = DenseTile<D>::MP, AP_ = DenseTile<D>::AP, BN_ = DenseTile<D>::BN;              \
        _Pragma("unroll")                                                                                  \
        for (int e = 0; e < E; ++e) {                                                                      \
            const float* mcol = Mbuf + (size_t)e * 32 * MP_ + 16 * tile + li;    /* M_e[.][column li of this tile] */ \
            const float* arow0 = Abuf + (e * 32 + li) * AP_ + kq;                /* A_e[row li][.] */      \
            const float* arow1 = arow0 + 16 * AP_;                                                         \
            _Pragma("unroll")                                                                              \
            for (int s4 = 0; s4 < 8; ++s4) {                                                               \
                const float wv = mcol[(size_t)(4 * s4 + kq) * MP_];                                        \
                AA[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, arow0[4 * s4], AA[0], 0, 0, 0);           \
                AA[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, arow1[4 * s4], AA[1], 0, 0, 0);           \
            }                                                                                              \
        }                                                                                                  \
        if (a.ebias) {                                                                                     \
            _Pragma("unroll")                                                                              \
            for (int e = 0; e < E; ++e) {                                                                  \
                const f32x4 be = *reinterpret_cast<const f32x4*>(Bbuf + e * BN_ + 16 * tile + 4 * kq);     \
                AA[0] += Nbuf[e * 32 + li] * be;                                                           \
                AA[1] += Nbuf[e * 32 + 16 + li] * be;                                                      \
            }                                                                                              \
        }                                                                                                  \
    }
// (debug) clock stamp K of pass STEP of workgroup 0, waves 0 and 6, into a.tdbg [step][wave sel][8] (stamp_ptr_from_env)
#define GGNN_DENSE_STAMP(STEP, K) if (a.tdbg && blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 6) && (STEP) < 8) \
        a.tdbg[((STEP) * 2 + (wave ? 1 : 0)) * 8 + (K)] = __builtin_amdgcn_s_memtime();

}  // namespace ggnn
