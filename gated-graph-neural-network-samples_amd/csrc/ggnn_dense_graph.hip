// Graph-resident dense GGNN forward (chem_tensorflow_dense.py:93-117): ALL timesteps of a graph in one workgroup, one launch.
//
// The dense model's batch is b graphs of v <= 32 padded vertices (BASELINE configs[2]: b = 256, v = 29, h = 100, 4 edge types,
// 4 timesteps).  7,424 rows are 464 row tiles for 256 CUs: the per-timestep kernels (h W_e for all e, adjacency aggregation,
// fused GRU -- 12 launches) are each latency-bound at 0.2 of their rooflines.  But a graph only ever reads its OWN vertices
// (A[g] is v x v), so nothing has to leave the CU between timesteps: workgroup g keeps the states of graph g in registers and
// runs, per timestep, E transform stages, the aggregation and the six GRU stages back to back.
//
//   * wave w (w < NT = ceil(h/16)) owns output COLUMN tile w of every stage, for both 16-row tiles of the graph: 25 MFMAs per row
//     tile and stage (h = 100).  Its slice of a stage's weights -- one column tile of the k-interleaved stage image, 25 floats per
//     lane -- comes straight from L2 into registers one stage ahead (tile_mma_regs): no LDS ring, no barrier per stage.
//   * every wave holds the full activation fragments (the MFMA's B operand: state h, then acts / r*h) of both row tiles.  What a
//     stage produces per column tile is exchanged through LDS: the transformed states M_e (all E of them: the aggregation reads
//     rows of OTHER vertices), acts, r*h and the new state -- four workgroup barriers per timestep.
//   * aggregation acts[i] = sum_e sum_j A_e[i,j] (M_e[j] + b_e) (:103-112; bias on every row before A_e, :107-108) runs on the matrix
//     pipe too: the graph's 0/1 adjacency rows sit in LDS for the whole launch, the products A_e[i,j] M_e[j] are exact, and the bias
//     term is nin_e[i] b_e (the row sums of A_e, formed once).
//   * GRU (TF-1.3 GRUCell, :115): r, u = sigmoid([acts|h] Wg + bg), c = tanh([acts | r*h] Wc + bc), h' = u h + (1-u) c; the r*h tile of
//     a wave is r times chunk w of its h fragment (output tile nt == activation chunk nt, as in the fused GRU).
// What this kernel shares with the split forward and the backward (LDS layout DenseF32Lds, prologue, aggregation, stage macro) is in
// ggnn_dense_graph.hpp; its register-fragment load_w / mma_pair are its own.
#include "ggnn_dense_graph.hpp"

namespace ggnn {

template <int D>
__global__ void dense_gru_pack_kernel(const float* __restrict__ Wg, const float* __restrict__ Wc, float* __restrict__ out) {
    const int i = blockIdx.y;                                          // image 0..5
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    float* img = out + (size_t)i * StageCfg<D>::IMG;
    if (i < 4) pack_stage_image<D>(Wg, (i & 1) * D, (i >> 1) * D, 2 * D, img, first, stride);     // rows: x | h;  columns: r | u
    else pack_stage_image<D>(Wc, (i & 1) * D, 0, D, img, first, stride);
}

template <int D, int E, int NW>
__global__ __launch_bounds__(NW * 64) void ggnn_dense_graph_kernel(DenseGraphArgs a) {
    using C = StageCfg<D>;
    using L = DenseF32Lds<D, E>;
    constexpr int NT = C::NT, NC = C::NC, NR = C::NR;
    constexpr int MP = L::T::MP;                                       // row pitch of the LDS blocks (floats)
    constexpr int NS = E + 6;                                          // stages per timestep
    static_assert(NT <= NW && NS % 2 == 0, "one column tile per wave; the two weight slots alternate with a fixed phase per timestep");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Mbuf = lds + L::M;                                          // [E][32][MP] the transformed states
    float* Xbuf = lds + L::X, * Rbuf = lds + L::R, * Hbuf = lds + L::H;   // exchange blocks: acts, r*h, the new state
    float* Abuf = lds + L::A, * Nbuf = lds + L::N, * Bbuf = lds + L::B;   // adjacency rows, in-degrees per type, edge biases
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int g = blockIdx.x;
    const int v = a.v;
    const bool mm = wave < NT;                                         // this wave owns a column tile
    const int tile = mm ? wave : 0;

    auto image = [&](int s) { return dense_stage_image<E, C::IMG>(a, s); };
    // fragment (rows t*16 + li, k = 16c + 4kq ..) of a [32][MP] LDS block
    auto frag_from_lds = [&](Frag<D>& f, const float* blk, int t) {
        const float* rowp = blk + (size_t)(t * 16 + li) * MP + 4 * kq;
#pragma unroll
        for (int c = 0; c < NC; ++c) f.v[c] = *reinterpret_cast<const f32x4*>(rowp + 16 * c);
#pragma unroll
        for (int q = 0; q < NR; ++q) f.r[q] = rowp[16 * NC + 4 * q - 4 * kq + kq];
    };
    auto to_lds = [&](float* blk, int t, f32x4 val) { tile_to_lds<D>(blk, t, val, li, kq, tile); };

    dense_load_adjacency<E, NW>(Abuf, a.A, v, tid);
    dense_load_edge_bias<D, E, NW>(Bbuf, a.ebias, tid);
    __syncthreads();
    dense_in_degrees<E>(Nbuf, Abuf, tid);
    Frag<D> hf[2], xf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = t * 16 + li;
        if (i < v) load_frag<D>(hf[t], a.h0 + (size_t)g * v * D, i, kq);
        else {
#pragma unroll
            for (int c = 0; c < (NC > 0 ? NC : 1); ++c) hf[t].v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < (NR > 0 ? NR : 1); ++q) hf[t].r[q] = 0.f;
        }
    }
    const int col0 = 16 * tile + 4 * kq;
    f32x4 b_r, b_u, b_c;
    dense_gate_bias<D>(b_r, b_u, b_c, a.bg, a.bc, col0);

    // this wave's column tile of a stage image, straight from L2: ONE per-lane byte offset for every image (scalar base + 32-bit
    // offset + immediate; per-load 64-bit lane addresses get hoisted for all ten images of a timestep and spill)
    const unsigned w_off = (unsigned)(kq * C::BN + li + tile * 16) * 16u;
    const unsigned wr_off = (unsigned)(C::MAIN + kq * C::BN + li + tile * 16) * 4u;
    auto load_w = [&](TileWeights<D>& w, const float* gimg) {
        const unsigned long long p = reinterpret_cast<unsigned long long>(gimg);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
        const float* sb = reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
#pragma unroll
        for (int c = 0; c < NC; ++c) w.v[c] = ld4_b(sb, w_off + (unsigned)(c * 4 * C::BN) * 16u);
#pragma unroll
        for (int q = 0; q < NR; ++q) w.r[q] = ld1_b(sb, wr_off + (unsigned)(q * 4 * C::BN) * 4u);
    };
    // both row tiles against one weight slice, the two accumulators alternating: a single accumulator would make the 25 MFMAs of a
    // tile one dependent chain (40 clocks per link instead of 32)
    auto mma_pair = [&](auto zero_c, f32x4 (&acc)[2], const Frag<D> (&f)[2], const TileWeights<D>& w) {
        constexpr bool ZERO = decltype(zero_c)::value;
        f32x4 c0 = acc[0], c1 = acc[1];
        if constexpr (ZERO) { c0 = f32x4{0.f, 0.f, 0.f, 0.f}; c1 = c0; }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.v[c][e], f[0].v[c][e], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.v[c][e], f[1].v[c][e], c1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[q], f[0].r[q], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.r[q], f[1].r[q], c1, 0, 0, 0);
        }
        acc[0] = c0; acc[1] = c1;
    };
    TileWeights<D> tw[2];
    if (mm) load_w(tw[0], image(0));

    for (int step = 0; step < a.steps; ++step) {
        const bool last = step + 1 == a.steps;
        GGNN_DENSE_STAMP(step, 0)
        // ---- E transform stages: M_e = h W_e, column tile `tile`, into LDS ------------------------------------------------------
        f32x4 acc[2];
#define GGNN_DG_XFORM(S)                                                                                   \
        if constexpr ((S) < E) {                                                                           \
            GGNN_DENSE_STAGE(S, acc, hf, true)                                                                \
            if (mm) { to_lds(Mbuf + (size_t)(S) * 32 * MP, 0, acc[0]); to_lds(Mbuf + (size_t)(S) * 32 * MP, 1, acc[1]); } \
        }
        GGNN_DG_XFORM(0) GGNN_DG_XFORM(1) GGNN_DG_XFORM(2) GGNN_DG_XFORM(3) GGNN_DG_XFORM(4) GGNN_DG_XFORM(5) GGNN_DG_XFORM(6) GGNN_DG_XFORM(7)
#undef GGNN_DG_XFORM
        GGNN_DENSE_STAMP(step, 1)
        __syncthreads();                                               // (1) every M_e is complete
        GGNN_DENSE_STAMP(step, 2)
        // ---- aggregation on the matrix pipe (GGNN_DENSE_AGGREGATE) -----------------------------------------------------------------
        f32x4 aa[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (mm) {
            GGNN_DENSE_AGGREGATE(aa)
            to_lds(Xbuf, 0, aa[0]); to_lds(Xbuf, 1, aa[1]);
        }
        GGNN_DENSE_STAMP(step, 3)
        __syncthreads();                                               // (2) acts complete
        frag_from_lds(xf[0], Xbuf, 0); frag_from_lds(xf[1], Xbuf, 1);
        GGNN_DENSE_STAMP(step, 4)
        // ---- gates --------------------------------------------------------------------------------------------------------------
        f32x4 ar[2], au[2], ac[2];
        GGNN_DENSE_STAGE(E + 0, ar, xf, true)
        GGNN_DENSE_STAGE(E + 1, ar, hf, false)
        GGNN_DENSE_STAGE(E + 2, au, xf, true)
        GGNN_DENSE_STAGE(E + 3, au, hf, false)
        GGNN_DENSE_STAGE(E + 4, ac, xf, true)                             // candidate, acts part (acts are still in xf)
        f32x4 htile[2], u4[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // chunk `tile` of the state fragment = the state at this lane's accumulator positions (row li, columns 16*tile + 4kq ..)
            f32x4 hv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NC; ++c) if (c == tile) hv = hf[t].v[c];
            if constexpr (NR > 0) { if (tile == NC) { hv = f32x4{0.f, 0.f, 0.f, 0.f}; hv.x = __shfl(hf[t].r[0], li); hv.y = __shfl(hf[t].r[0], li + 16); hv.z = __shfl(hf[t].r[0], li + 32); hv.w = __shfl(hf[t].r[0], li + 48); if (kq) hv = f32x4{0.f, 0.f, 0.f, 0.f}; } }
            htile[t] = hv;
            f32x4 r4;
#pragma unroll
            for (int e = 0; e < 4; ++e) { r4[e] = sigmoid_f(ar[t][e] + b_r[e]); u4[t][e] = sigmoid_f(au[t][e] + b_u[e]); }
            ar[t] = r4 * hv;                                           // r * h tile
        }
        GGNN_DENSE_STAMP(step, 5)
        if (mm) { to_lds(Rbuf, 0, ar[0]); to_lds(Rbuf, 1, ar[1]); }
        __syncthreads();                                               // (3) r*h complete
        frag_from_lds(xf[0], Rbuf, 0); frag_from_lds(xf[1], Rbuf, 1);
        GGNN_DENSE_STAMP(step, 6)
        GGNN_DENSE_STAGE(E + 5, ac, xf, false)                            // candidate, r*h part
        GGNN_DENSE_STAMP(step, 7)
        f32x4 hn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = tanh_f(ac[t][e] + b_c[e]);
                hn[t][e] = u4[t][e] * htile[t][e] + (1.0f - u4[t][e]) * c;
            }
        }
        if (last) {
            if (mm) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int i = t * 16 + li;
                    if (i < v && col0 < D) *reinterpret_cast<f32x4*>(a.out + ((size_t)g * v + i) * D + col0) = hn[t];
                }
            }
        } else {
            if (mm) { to_lds(Hbuf, 0, hn[0]); to_lds(Hbuf, 1, hn[1]); }
            __syncthreads();                                           // (4) new state complete
            frag_from_lds(hf[0], Hbuf, 0); frag_from_lds(hf[1], Hbuf, 1);
        }
    }
}

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_dense_propagate_supported(int v, int E, int D) {
    return dense_shape_ok(v, E, D) && dense_dispatch(D, E, [](auto d, auto e) {
        return DenseF32Lds<decltype(d)::value, decltype(e)::value>::BYTES <= kDenseLdsLimit; });
}

// The E edge-weight stage images of the graph-resident kernel: always the f32 stage image (this kernel reads its weights as f32
// register tiles; ggnn_edge_weights_pack_f32 writes the format of the process's matrix path, which may be the split one).
template <int D>
__global__ void dense_edge_pack_kernel(const float* __restrict__ W, float* __restrict__ out) {
    const int t = blockIdx.y;
    pack_stage_image<D>(W + (size_t)t * D * D, 0, 0, D, out + (size_t)t * StageCfg<D>::IMG, blockIdx.x * blockDim.x + threadIdx.x,
                        gridDim.x * blockDim.x);
}

// bytes of T f32 stage images (0: no kernel for the hidden size)
static size_t dense_f32_images_bytes(int D, int T) {
    return dense_for_D(D, [&](auto d) { return (size_t)T * StageCfg<decltype(d)::value>::IMG * sizeof(float); });
}
// (the packed buffers hold the f32 stage images FOLLOWED by the split ones: which kernel runs is decided per launch -- matrix
// path of the process, and whether the split kernel's LDS blocks fit the launch's number of edge types)
extern "C" size_t ggnn_dense_edge_packed_bytes(int D, int T) {
    if (T <= 0 || !dense_f32_images_bytes(D, T)) return 0;
    return dense_f32_images_bytes(D, T) + dense_split_edge_bytes(D, T);
}

extern "C" int ggnn_dense_edge_pack_f32(const float* W, int T, int D, float* packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(W && packed && aligned16(packed) && T > 0 && T <= 64, "null or misaligned pointer, or T = %d outside 1..64", T);
    hipStream_t st = (hipStream_t)stream;
    if (!dense_f32_images_bytes(D, T)) return fail(GGNN_E_UNSUPPORTED, "no graph-resident dense kernel for hidden size %d", D);
    dense_for_D(D, [&](auto d) {
        hipLaunchKernelGGL((dense_edge_pack_kernel<decltype(d)::value>), dim3(8, T), dim3(256), 0, st, W, packed);
        return 0; });
    GGNN_CHECK_HIP(hipGetLastError());
    return dense_split_pack_edge(W, T, D, packed + dense_f32_images_bytes(D, T) / sizeof(float), st);
}

extern "C" size_t ggnn_dense_gru_packed_bytes(int D) {
    return dense_f32_images_bytes(D, 6) ? dense_f32_images_bytes(D, 6) + dense_split_gru_bytes(D) : 0;
}

extern "C" int ggnn_dense_gru_pack_f32(const float* Wg, const float* Wc, int D, float* packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(Wg && Wc && packed && aligned16(packed), "null or misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!dense_f32_images_bytes(D, 6)) return fail(GGNN_E_UNSUPPORTED, "no graph-resident dense kernel for hidden size %d", D);
    dense_for_D(D, [&](auto d) {
        hipLaunchKernelGGL((dense_gru_pack_kernel<decltype(d)::value>), dim3(8, 6), dim3(256), 0, st, Wg, Wc, packed);
        return 0; });
    GGNN_CHECK_HIP(hipGetLastError());
    return dense_split_pack_gru(Wg, Wc, D, packed + dense_f32_images_bytes(D, 6) / sizeof(float), st);
}

// split form (bf16 pipe, ggnn_dense_graph_split.hip) where it exists and fits; GGNN_DENSE_SPLIT=0 keeps the f32-MFMA kernel
extern "C" int ggnn_dense_propagate_is_split(int v, int E, int D) {
    static const bool want_split = [] { const char* e = getenv("GGNN_DENSE_SPLIT"); return !e || atoi(e) != 0; }();
    return (want_split && split_matrix_path() && ggnn_dense_propagate_supported(v, E, D) && dense_split_supported(v, E, D)) ? 1 : 0;
}

extern "C" int ggnn_dense_train_supported(int v, int E, int D) {
    return (ggnn_dense_propagate_is_split(v, E, D) && dense_bwd_supported(v, E, D)) ? 1 : 0;
}

extern "C" size_t ggnn_dense_train_saved_bytes(int b, int v, int D, int steps) {
    if (b <= 0 || v <= 0 || D <= 0 || steps <= 0) return 0;
    return (size_t)6 * steps * b * v * D * sizeof(float);
}

// saved != NULL: the saving launch of the training route (split kernel only)
static int dense_propagate(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                           const float* edge_bias, const float* bg, const float* bc, float* out, int b, int v, int E,
                           int D, int steps, int fmt, float* saved, hipStream_t st) {
    GGNN_CHECK_ARG(b >= 0 && steps >= 1, "bad sizes b=%d steps=%d", b, steps);
    GGNN_CHECK_ARG(fmt == 0 || fmt == GGNN_GRU_FMT_F16X2 || fmt == GGNN_GRU_FMT_BF16X3, "fmt %d is not a GGNN_GRU_FMT_* value", fmt);
    if (!ggnn_dense_propagate_supported(v, E, D))
        return fail(GGNN_E_UNSUPPORTED, "graph-resident dense forward: v <= 32, E in {2,4,6,8}, hidden size 32/64/100 (got v=%d E=%d D=%d)", v, E, D);
    if (b == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && A && edge_packed && gru_packed && bg && bc && out, "null pointer");
    GGNN_CHECK_ARG(aligned16(h0) && aligned16(out) && aligned16(edge_packed) && aligned16(gru_packed) && (!edge_bias || aligned16(edge_bias)),
                   "pointers must be 16-byte aligned");
    const DenseGraphArgs a{h0, A, edge_packed, gru_packed, edge_bias, bg, bc, out, b, v, steps, stamp_ptr_from_env("GGNN_DG_TPTR"), saved};
    if (ggnn_dense_propagate_is_split(v, E, D)) {
        DenseGraphArgs s = a;
        s.eimg = edge_packed + (dense_f32_images_bytes(D, E) + dense_split_images_offset(D, E, fmt)) / sizeof(float);
        s.gimg = gru_packed + (dense_f32_images_bytes(D, 6) + dense_split_images_offset(D, 6, fmt)) / sizeof(float);
        return dense_split_launch(s, E, D, fmt, st);
    }
    return dense_dispatch(D, E, [&](auto d, auto e) {
        constexpr int DD = decltype(d)::value, EE = decltype(e)::value;
        return dense_graph_launch<&ggnn_dense_graph_kernel<DD, EE, kDenseWaves>>(DenseF32Lds<DD, EE>::BYTES, a, st); });
}

extern "C" int ggnn_dense_propagate_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                                        const float* edge_bias, const float* bg, const float* bc, float* out, int b, int v, int E,
                                        int D, int steps, int fmt, ggnn_stream_t stream) {
    return dense_propagate(h0, A, edge_packed, gru_packed, edge_bias, bg, bc, out, b, v, E, D, steps, fmt, nullptr, (hipStream_t)stream);
}

extern "C" int ggnn_dense_propagate_save_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                                             const float* edge_bias, const float* bg, const float* bc, float* out, int b, int v, int E,
                                             int D, int steps, int fmt, float* saved, size_t saved_bytes, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(b >= 0 && steps >= 1, "bad sizes b=%d steps=%d", b, steps);
    if (!ggnn_dense_train_supported(v, E, D))
        return fail(GGNN_E_UNSUPPORTED, "graph-resident dense training: split matrix path, v <= 32, E in {2,4,6,8}, hidden size 32/64/100 "
                                        "(got v=%d E=%d D=%d)", v, E, D);
    if (b == 0) return GGNN_OK;
    GGNN_CHECK_ARG(saved && aligned16(saved), "saved: null or misaligned pointer");
    GGNN_CHECK_ARG(saved_bytes >= ggnn_dense_train_saved_bytes(b, v, D, steps), "saved_bytes %zu < %zu", saved_bytes,
                   ggnn_dense_train_saved_bytes(b, v, D, steps));
    return dense_propagate(h0, A, edge_packed, gru_packed, edge_bias, bg, bc, out, b, v, E, D, steps, fmt, saved, (hipStream_t)stream);
}
