// The gather-fused BasicRNNCell of ggnn_rnn_fused.hip (chem_tensorflow_sparse.py:109-110, 198-216) for hidden sizes 128 / 192 / 256,
// on COLUMN PANELS of W, in one launch:
//
//     incoming[v] = (sum over slots row_ptr[v] .. row_ptr[v+1] of Hrows[gather_row[slot]]) / (sum_t nin[v,t] + 1e-7)
//     h'          = act([x_0 | .. | x_{nx-2} | incoming | h] W + b)          W [(nx+1) D, D], act = tanh / ReLU
//
// At D <= 100 all nx + 1 weight blocks stay in LDS for the whole launch (ggnn_rnn_fused.hip); at D = 128 two exact three-piece blocks
// are already 192 KiB.  Here, on the shared panel layer (ggnn_panel.hpp), one workgroup of 8 waves per CU owns
// a PASS of 8 x 16 rows, each wave a 16-row tile, and the (nx + 1) D / 64 panel images [D, 64] of W stream through a two-slot LDS-DMA
// ring in PanelGruSplitCfg::PARTS parts (D = 128: whole 48 KiB images; 192: thirds of 24 KiB; 256: halves of 48 KiB).
//
// Loop order: the K SEGMENT is outermost, the panel inside it.  A wave holds ONE segment's fragment (D / 4 registers) and multiplies
// it into a resident full-row accumulator set acc[D / 64][4] (another D / 4 registers) for each of the segment's D / 64 panels, then
// loads the next segment's fragment; bias, activation and the store run once per panel, in the last segment.  Every operand row is
// therefore read from HBM once whatever nx (the forward panel GRU re-reads its fragments per panel), no [V, D] intermediate exists,
// and a panel image is read from L2 once per pass and CU.
//
// Segment order.  The images lie in memory in W's own order, image s NP + p = rows s D .., columns 64 p .. (s = nx - 1: incoming,
// s = nx: h).  A pass WALKS them incoming first, then x_0 .. x_{nx-2}, then h -- ggnn_rnn_fused.hip's order -- and not 0 .. nx: the
// gather needs the partial sum and the rows in flight beside it (D = 256: 64 + 2 x 64 registers), which fits only while the
// accumulators are not yet live.  The order is fixed, so h' is bit-identical from run to run, and save_incoming is a plain store of
// the gathered fragment: h' does not depend on it.
//
// Schedule of a workgroup: [DMA part 0 of the first image] | pass: gather (per wave, no barrier) -> (nx + 1) NP PARTS rounds of
// {DMA of the next part into the other slot, (first round of a segment: its fragment load), MFMA burst on this slot, (last segment,
// last part of a panel: epilogue + 4 stores), barrier}.  The last round of a pass brings in the first part of the NEXT pass, so a
// pass's gather meets a ready ring.  The round barrier is PanelRing's counted wait.  The segment loop is a run-time loop
// (the rounds of ONE segment are unrolled, not all of them: D = 256 / nx = 3 would be 3072 MFMAs of straight-line code).
//
// Exact bf16x3 only: ReLU states have no bound, so the two-piece f16 format's operand range cannot be proven (ggnn_rnn_fused.hip).
//
// Addressing is that kernel's: rows >= V are neither read nor written (their lanes read row V - 1 and store nothing), row_ptr values
// are clamped to [0, M], a gather_row outside [0, num_rows) adds nothing and is not dereferenced.  32-bit byte offsets: V * D and
// num_rows * D must stay below 2^30 (the entry point refuses larger calls).
#include "ggnn_panel.hpp"
#include <algorithm>

namespace ggnn {
namespace {

constexpr int kRnnPanelNW = kPanelNW;

template <int D>
using RnnPanelImg = PanelGruSplitCfg<D, kSplitBf16x3>;

constexpr bool rnn_panel_ok(int D, int nx) { return panel_hidden_ok(D) && nx >= 1 && nx <= 3; }

template <int D>
constexpr size_t rnn_panel_bytes(int nx) { return (size_t)(nx + 1) * PanelCfg<D>::NP * RnnPanelImg<D>::IMG_BYTES; }

struct RnnPanelArgs {
    const float* x[2];                                 // residual segments (nx - 1 of them)
    const float* h;
    const float* packed;                               // (nx + 1) NP panel images, image s NP + p
    const float* b;
    float* h_out;
    const float* H;                                    // [num_rows, D]
    const int* row_ptr;
    const int* gidx;
    const float* nin;
    float* save;                                       // null or [V, D]
    int num_rows, M, T, use_avg, V, act;
};

// g += the rows of slots k .. k+N-1, in slot order (rnn_fused_kernel's expression: f += ok ? t : 0); all N rows in flight first
template <int D, int N>
__device__ __forceinline__ void rnn_panel_gather(Frag<D>& g, const float* __restrict__ H, const int* __restrict__ gidx, int k,
                                                 int num_rows, int kq) {
    Frag<D> t[N];
    bool ok[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int j = gidx[k + i];
        ok[i] = (unsigned)j < (unsigned)num_rows;
        load_frag<D>(t[i], H, ok[i] ? j : 0, kq);
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < PanelCfg<D>::NC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) g.v[c][e] += ok[i] ? t[i].v[c][e] : 0.f;
}

template <int D>
__global__ void rnn_panel_pack_kernel(const float* __restrict__ W, float* __restrict__ packed) {
    using C = PanelCfg<D>;
    const int p = blockIdx.y, s = blockIdx.z;          // image s NP + p: rows s D .. of W, columns 64 p ..
    float* dst = packed + (size_t)(s * C::NP + p) * RnnPanelImg<D>::IMG;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    pack_panel_gru_split_image<D, kSplitBf16x3, false>(W, s * D, p * C::BN, D, dst, first, stride);
}

template <int D, int NX>
__global__ __launch_bounds__(kRnnPanelNW * 64) void rnn_panel_kernel(RnnPanelArgs a) {
    using C = PanelCfg<D>;
    using SC = RnnPanelImg<D>;
    constexpr int NW = kRnnPanelNW, NP = C::NP, NC = C::NC, PARTS = SC::PARTS, SLOTF = SC::PART, IMGF = SC::IMG;
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];     // [2][PART]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V;
    const PanelPassWalk<NW> walk((V + 15) / 16, blockIdx.x, gridDim.x);
    const float* packed = a.packed;
    PanelRing<SC::PART_BYTES, NW> ring{ring_lds, wave, lane};
    // the image segment walked at position q of a pass: incoming (nx - 1) first, then x_0 .., then h (nx)
    auto seg_at = [](int q) { return q == 0 ? NX - 1 : (q == NX ? NX : q - 1); };
    if (walk.n_pass > 0) ring.fill_first(packed + (size_t)seg_at(0) * NP * IMGF);

    walk.run(wave, [&](auto active_c, int idx, bool first_pass, bool last_pass) {
        constexpr bool ACT = decltype(active_c)::value;
        const int r = idx * 16 + li;
        const bool live = r < V;
        const int rc = live ? r : V - 1;                    // (a row of its own for every lane: nothing beyond V is read)
        Frag<D> f;
        if constexpr (ACT) {
            int beg = 0, end = 0;
            if (live) {
                beg = min(max(a.row_ptr[r], 0), a.M);
                end = min(max(a.row_ptr[r + 1], beg), a.M);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) f.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            panel_gather_ladder<D>(beg, end, [&](auto n_c, int k) {
                rnn_panel_gather<D, decltype(n_c)::value>(f, a.H, a.gidx, k, a.num_rows, kq);
            });
            if (a.use_avg) {                                // :206-209, the expression of the stand-alone segment sum
                float deg = 0.f;
                for (int t = 0; t < a.T; ++t) deg += a.nin[(size_t)rc * a.T + t];
                const float den = deg + 1e-7f;
#pragma unroll
                for (int c = 0; c < NC; ++c) f.v[c] = f.v[c] / den;
            }
            if (a.save && live) {
                const unsigned ob = ((unsigned)r * (unsigned)D + 4u * (unsigned)kq) * 4u;
#pragma unroll
                for (int c = 0; c < NC; ++c) st4_b(a.save, ob + 64u * c, f.v[c]);
            }
        }
        if (first_pass) ring.first_ready();                 // (later passes: the previous pass's last round)
        f32x4 acc[NP][4];
        if constexpr (ACT) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[p][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll 1
        for (int q = 0; q <= NX; ++q) {
            const int seg = seg_at(q), nseg = seg_at(q == NX ? 0 : q + 1);
            const bool last_q = q == NX;
            auto panel = [&](auto p_c) {
                constexpr int p = decltype(p_c)::value;
                panel_for_parts<PARTS>([&](auto part_c) {
                    constexpr int part = decltype(part_c)::value;
                    const bool more = part + 1 < PARTS || p + 1 < NP || !last_q || !last_pass;
                    const float* nsrc = panel_next_part<PARTS, IMGF, SLOTF>(packed, seg * NP + p, part, p + 1 < NP ? seg * NP + p + 1 : nseg * NP);
                    panel_round<part, PARTS, ACT, true>(ring, more, nsrc,
                        [&] {
                            // the fragment of a residual segment or of h, behind the round's DMA pieces: the burst below waits for it
                            if constexpr (p == 0 && part == 0) { if (q > 0) load_frag<D>(f, last_q ? a.h : (q == 1 ? a.x[0] : a.x[1]), rc, kq); }
                            return 0;
                        },
                        [&] { panel_part_mma_split<D, false, false, part, kSplitBf16x3>(acc[p], f, ring.slot(), li, kq); },
                        [&] {
                            if (!last_q) return 0;
                            // EpiBiasAct, term for term.  The bias quads are loaded by every lane of a wave with a tile and each store's value
                            // depends on one, so hipcc's own waits have retired them when the last store is issued: the four stores are the
                            // last vector-memory instructions of the round.
                            f32x4 c[4];
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                c[nt] = acc[p][nt] + ld4(a.b + p * 64 + nt * 16 + 4 * kq);
                                if (a.act == GGNN_ACT_TANH) { c[nt].x = tanh_f(c[nt].x); c[nt].y = tanh_f(c[nt].y); c[nt].z = tanh_f(c[nt].z); c[nt].w = tanh_f(c[nt].w); }
                                else { c[nt].x = fmaxf(c[nt].x, 0.f); c[nt].y = fmaxf(c[nt].y, 0.f); c[nt].z = fmaxf(c[nt].z, 0.f); c[nt].w = fmaxf(c[nt].w, 0.f); }
                            }
                            // (every tile has a valid first row: the four stores are issued by every wave with a tile)
                            if (live) {
#pragma unroll
                                for (int nt = 0; nt < 4; ++nt)
                                    st4_b(a.h_out, ((unsigned)r * (unsigned)D + (unsigned)(p * 64 + nt * 16 + 4 * kq)) * 4u, c[nt]);
                            }
                            return 4;
                        });
                });
            };
            panel(std::integral_constant<int, 0>{});
            panel(std::integral_constant<int, 1>{});
            if constexpr (NP > 2) panel(std::integral_constant<int, 2>{});
            if constexpr (NP > 3) panel(std::integral_constant<int, 3>{});
        }
    });
}

template <int D, int NX>
int rnn_panel_launch(const RnnPanelArgs& a, hipStream_t st) {
    return panel_launch<&rnn_panel_kernel<D, NX>>((size_t)2 * RnnPanelImg<D>::PART_BYTES, 48 * 1024, panel_blocks(a.V, kRnnPanelNW), st, a);
}

template <int D>
int rnn_panel_dispatch_nx(const RnnPanelArgs& a, int nx, hipStream_t st) {
    switch (nx) {
        case 1: return rnn_panel_launch<D, 1>(a, st);
        case 2: return rnn_panel_launch<D, 2>(a, st);
        default: return rnn_panel_launch<D, 3>(a, st);
    }
}

template <int D>
int rnn_panel_pack(const float* W, int nx, float* packed, hipStream_t st) {
    hipLaunchKernelGGL((rnn_panel_pack_kernel<D>), dim3(8, PanelCfg<D>::NP, (unsigned)(nx + 1)), dim3(256), 0, st, W, packed);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

int rnn_panel_unsupported(int D, int nx) {
    return fail(GGNN_E_UNSUPPORTED, "panel RNN cell supports D = 128, 192, 256 with nx = 1..3 (got D=%d nx=%d)", D, nx);
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_rnn_panel_supported(int D, int nx) { return rnn_panel_ok(D, nx) ? 1 : 0; }

extern "C" size_t ggnn_rnn_panel_packed_bytes(int D, int nx) {
    if (!rnn_panel_ok(D, nx)) return 0;
    return panel_for_D(D, [&](auto d) { return rnn_panel_bytes<decltype(d)::value>(nx); });
}

extern "C" void ggnn_rnn_panel_launch_geometry(int D, int nx, int* rows_per_workgroup, int* max_workgroups) {
    const bool ok = rnn_panel_ok(D, nx);
    if (rows_per_workgroup) *rows_per_workgroup = ok ? kRnnPanelNW * 16 : 0;
    if (max_workgroups) *max_workgroups = ok ? num_cus() : 0;
}

extern "C" int ggnn_rnn_panel_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream) {
    if (!rnn_panel_ok(D, nx)) return rnn_panel_unsupported(D, nx);
    GGNN_CHECK_ARG(W && packed && aligned16(packed) && (const void*)W != (const void*)packed, "null, misaligned or aliasing pointer");
    return panel_for_D(D, [&](auto d) { return rnn_panel_pack<decltype(d)::value>(W, nx, packed, (hipStream_t)stream); });
}

extern "C" int ggnn_rnn_panel_gather_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* b,
                                         float* h_out, const float* Hrows, int64_t num_rows, const int32_t* row_ptr,
                                         const int32_t* gather_row, int64_t M, const float* nin, int T, int use_avg,
                                         float* save_incoming, int V, int D, int act, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && num_rows >= 0 && M >= 0 && M < (1LL << 31), "bad sizes V=%d D=%d rows=%lld M=%lld", V, D,
                   (long long)num_rows, (long long)M);
    GGNN_CHECK_ARG(act == GGNN_ACT_TANH || act == GGNN_ACT_RELU, "unknown activation %d", act);
    if (!rnn_panel_ok(D, nx)) return rnn_panel_unsupported(D, nx);
    if ((unsigned long long)V * D >= (1ULL << 30) || (unsigned long long)num_rows * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "V*D and num_rows*D must be < 2^30 (32-bit byte offsets)");
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h && packed && b && h_out && row_ptr, "null pointer");
    GGNN_CHECK_ARG(M == 0 || num_rows == 0 || (Hrows && gather_row), "Hrows / gather_row missing");
    GGNN_CHECK_ARG(!use_avg || (nin && T > 0), "nin [V, T] is required for mean aggregation");
    GGNN_CHECK_ARG(nx == 1 || x_segs, "residual segments missing");
    GGNN_CHECK_ARG(aligned16(h) && aligned16(packed) && aligned16(b) && aligned16(h_out) && aligned16(Hrows) &&
                   (!save_incoming || aligned16(save_incoming)), "pointers must be 16-byte aligned");
    RnnPanelArgs a{};
    const void* inputs[8] = {h, packed, b, Hrows, nin, nullptr, nullptr, nullptr};
    for (int s = 0; s + 1 < nx; ++s) {
        GGNN_CHECK_ARG(x_segs[s] && aligned16(x_segs[s]), "residual segment %d null or misaligned", s);
        a.x[s] = x_segs[s];
        inputs[5 + s] = x_segs[s];
    }
    for (const void* in : inputs)
        GGNN_CHECK_ARG(!in || ((const void*)h_out != in && (const void*)save_incoming != in), "h_out / save_incoming aliases an input");
    GGNN_CHECK_ARG(h_out != save_incoming, "h_out aliases save_incoming");
    a.h = h; a.packed = packed; a.b = b; a.h_out = h_out; a.H = Hrows; a.row_ptr = row_ptr; a.gidx = gather_row; a.nin = nin;
    a.save = save_incoming;
    a.num_rows = (int)num_rows;
    a.M = (num_rows > 0 && Hrows && gather_row) ? (int)M : 0;      // no rows to gather from: every node's slot range is empty
    a.T = T; a.use_avg = use_avg ? 1 : 0; a.V = V; a.act = act;
    return panel_for_D(D, [&](auto d) { return rnn_panel_dispatch_nx<decltype(d)::value>(a, nx, (hipStream_t)stream); });
}
