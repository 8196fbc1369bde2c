// The fused GCN layer of ggnn_gcn.hip for hidden sizes 128 / 192 / 256, on COLUMN PANELS of W:
//
//     S   = A_hat x            A_hat sparse (CSR: row_ptr, col, val), x [V, D]
//     out = dropout(relu(S W + b))     (bias, ReLU and dropout each optional; S stored on request)
//
// At D <= 100 the D x D weight image stays in LDS for the whole launch and a wave's 16 rows x D accumulators fit its registers; at
// D = 256 the exact three-piece image is 384 KiB and the accumulators alone would be 64 registers next to the 64 of the aggregate.
// Here a workgroup of 8 waves owns a PASS of 8 x 16 rows.  Each wave builds the aggregate S of its 16-row tile ONCE, in registers
// (the slot-order fmaf chain of ggnn_gcn.hip: deterministic, no atomics), stores it if asked, and then the workgroup walks the
// D / 64 column panels of W: a panel image (pack_panel_gru_split_image's chunk-major format) comes through a two-slot LDS-DMA ring
// in PanelGruSplitCfg::PARTS parts (D = 256: halves of 48 KiB), each wave multiplies its resident fragment with
// panel_part_mma_split (exact bf16x3 form: there is no range proof for GCN states, so no f16x2 here), runs gcn_epilogue on the panel's
// 64 columns and stores them.  No [V, D] intermediate: x is gathered once, out written once.
//
// This is the row binding (the streamed ring transform's, ggnn_panel.hip), not the stationary one (a workgroup per panel, the
// aggregation repeated per panel): the gather is the HBM side of this kernel -- every aggregate row is deg(row) gathered rows --
// and the stationary binding would repeat it D / 64 times and store S from one panel's workgroups only, while the images it
// saves are read from L2 (NP x 96 KiB per pass and CU).
//
// Schedule of a workgroup: [DMA part 0 of panel 0] | pass: gather (per wave, no barrier) -> NP x PARTS rounds of
// {DMA of the next part into the other slot, MFMA burst on this slot, (last part of a panel: epilogue + stores), barrier}.  The
// last round of a pass brings in part 0 of panel 0 for the NEXT pass, so a pass's gather meets a ready ring and the only waits are
// the workgroup's own round barriers -- neither the gather nor a ring wait is a launch-wide phase.
//
// The backward's dx = A_hat^T (dP W^T) is the same launch on the transposed CSR with the panels of W^T (transpose = 1 packs them).
// The BWD instantiation (ggnn_gcn_panel_layer_bwd_f32, the twin of ggnn_gcn.hip's) writes the dP of the layer BELOW: in the last
// part of each panel the epilogue applies that layer's dropout mask and the ReLU gate of its forward output gate_out =
// dropout(relu(P)), read at the lane's own row and column quad -- bit for bit the panel launch followed by ggnn_dropout_f32 and
// ggnn_act_bwd_f32, without their [V, D] round trips.  BWD is a template parameter: the forward instantiations keep their code
// and registers.  ggnn_gcn_panel_train_pack_f32 builds every panel image of a training step (W_l and W_l^T) in one launch.
#include "ggnn_gcn.hpp"
#include "ggnn_panel.hpp"

namespace ggnn {
namespace {

constexpr int kGcnPanelNW = kPanelNW;

template <int D>
using GcnPanelImg = PanelGruSplitCfg<D, kSplitBf16x3>;

// a packed layer image: the D / 64 panel images of one weight matrix, back to back
template <int D>
constexpr size_t gcn_panel_layer_image_bytes() { return (size_t)PanelCfg<D>::NP * GcnPanelImg<D>::IMG_BYTES; }

template <int D>
__global__ void gcn_panel_pack_kernel(const float* __restrict__ W, int transpose, float* __restrict__ img) {
    using C = PanelCfg<D>;
    const int p = blockIdx.y;
    float* dst = img + (size_t)p * GcnPanelImg<D>::IMG;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (transpose) pack_panel_gru_split_image<D, kSplitBf16x3, true>(W, 0, p * C::BN, D, dst, first, stride);
    else pack_panel_gru_split_image<D, kSplitBf16x3, false>(W, 0, p * C::BN, D, dst, first, stride);
}

// a += sum over N slots k .. k+N-1 of val * x[col, :], in slot order; all N rows are in flight before the first fmaf.  A column index
// outside [0, V) contributes nothing (the host layer validates the CSR; the kernel only guarantees that it never reads outside x).
template <int D, int N>
__device__ __forceinline__ void gcn_panel_gather(Frag<D>& a, const float* __restrict__ x, const int* __restrict__ col,
                                                 const float* __restrict__ val, int k, int V, int kq) {
    Frag<D> t[N];
    float w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int j = col[k + i];
        const bool ok = (unsigned)j < (unsigned)V;
        w[i] = ok ? val[k + i] : 0.f;
        load_frag<D>(t[i], x, ok ? j : 0, kq);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) frag_fma<D>(a, w[i], t[i]);
}

// Every panel image of a training step in ONE launch: blockIdx.z = slot j of `images`, slot j < L the D / 64 panel images of W_j,
// slot L + (l - 1) those of W_l^T for l >= 1 (layer 0 forms no dx); blockIdx.y = the panel.  pack_panel_gru_split_image writes word
// i as a function of (i, W) alone: the images are gcn_panel_pack_kernel's bit for bit whatever the grid.
constexpr int kGcnPanelTrainMaxLayers = 64;
struct GcnPanelPackList { const float* W[kGcnPanelTrainMaxLayers]; };

template <int D>
__global__ __launch_bounds__(256) void gcn_panel_train_pack_kernel(GcnPanelPackList w, int L, float* __restrict__ images,
                                                                   unsigned slot_floats) {
    using C = PanelCfg<D>;
    const int j = blockIdx.z, p = blockIdx.y;
    const bool transpose = j >= L;
    const float* W = w.W[transpose ? j - L + 1 : j];
    float* dst = images + (size_t)j * slot_floats + (size_t)p * GcnPanelImg<D>::IMG;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (transpose) pack_panel_gru_split_image<D, kSplitBf16x3, true>(W, 0, p * C::BN, D, dst, first, stride);
    else pack_panel_gru_split_image<D, kSplitBf16x3, false>(W, 0, p * C::BN, D, dst, first, stride);
}

// BWD: x = dP of this layer, (row_ptr, col, val) = the transposed CSR, packed = the panel images of W^T, ep = the dropout of the
// layer below (no bias, no ReLU), gate_out [V, D] = that layer's forward output; out = its dP.  s_out is not written.
template <int D, bool BWD = false>
__global__ __launch_bounds__(kGcnPanelNW * 64) void gcn_panel_layer_kernel(
        const float* __restrict__ x, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val,
        int nnz, const float* __restrict__ packed, GcnEpilogue ep, float* __restrict__ out, float* __restrict__ s_out, int V,
        const float* __restrict__ gate_out) {
    using C = PanelCfg<D>;
    using SC = GcnPanelImg<D>;
    constexpr int NW = kGcnPanelNW, NP = C::NP, NC = C::NC, PARTS = SC::PARTS, SLOTF = SC::PART, IMGF = SC::IMG;
    extern __shared__ __attribute__((aligned(16))) float ring_lds[];     // [2][PART]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const PanelPassWalk<NW> walk((V + 15) / 16, blockIdx.x, gridDim.x);
    PanelRing<SC::PART_BYTES, NW> ring{ring_lds, wave, lane};
    if (walk.n_pass > 0) ring.fill_first(packed);

    walk.run(wave, [&](auto active_c, int idx, bool first_pass, bool last_pass) {
        constexpr bool ACT = decltype(active_c)::value;
        const int r = idx * 16 + li;
        Frag<D> a;
        if constexpr (ACT) {
            int beg = 0, end = 0;
            if (r < V) {
                // (clamped to [0, nnz]: a corrupt row_ptr cannot send the gather out of the index arrays)
                beg = min(max(row_ptr[r], 0), nnz);
                end = min(max(row_ptr[r + 1], beg), nnz);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) a.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            panel_gather_ladder<D>(beg, end, [&](auto n_c, int k) { gcn_panel_gather<D, decltype(n_c)::value>(a, x, col, val, k, V, kq); });
            if (!BWD && s_out && r < V) {
                const unsigned ob = ((unsigned)r * (unsigned)D + 4u * (unsigned)kq) * 4u;
#pragma unroll
                for (int c = 0; c < NC; ++c) st4_b(s_out, ob + 64u * c, a.v[c]);
            }
        }
        if (first_pass) ring.first_ready();                     // (later passes: the previous pass's last round)
        f32x4 acc[4];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            panel_for_parts<PARTS>([&](auto part_c) {
                constexpr int part = decltype(part_c)::value;
                const bool more = part + 1 < PARTS || p + 1 < NP || !last_pass;
                f32x4 gate[4];
                panel_round<part, PARTS, ACT, true>(ring, more, panel_next_part<PARTS, IMGF, SLOTF>(packed, p, part, p + 1 < NP ? p + 1 : 0),
                    [&] {
                        // BWD: the lane's four gate quads of this panel, issued BEHIND the round's DMA pieces and in front of the burst that
                        // hides them.  The counted wait below still holds, by construction: every st4_b's value is a select on one of these
                        // loads (and on ep.row_key[r], where given), so hipcc's own waits have retired all of them when the last store is
                        // issued, and no vector-memory instruction follows the stores.  A row r >= V loads nothing (and stores nothing).
                        if constexpr (BWD && part == PARTS - 1) {
                            if (r < V) {
#pragma unroll
                                for (int nt = 0; nt < 4; ++nt)
                                    gate[nt] = ld4_b(gate_out, ((unsigned)r * (unsigned)D + (unsigned)(p * 64 + nt * 16 + 4 * kq)) * 4u);
                            }
                        }
                        return 0;
                    },
                    [&] { panel_part_mma_split<D, part == 0, false, part, kSplitBf16x3>(acc, a, ring.slot(), li, kq); },
                    [&] {
                        // (every tile has a valid first row: the four stores are issued by every wave with a tile, behind the round's DMA)
                        if (r < V) {
                            // (the lane's column passes through an empty asm: without it hipcc hoists the first Philox round of all D / 4
                            //  column quads out of the pass loop -- 48 registers live across the gather, 44 B of scratch at D = 256)
                            int kqe = kq;
                            asm volatile("" : "+v"(kqe));
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                const int c0 = p * 64 + nt * 16 + 4 * kqe;
                                f32x4 v = gcn_epilogue(acc[nt], r, c0, ep);
                                if constexpr (BWD) v = gcn_relu_gate(v, gate[nt]);
                                st4_b(out, ((unsigned)r * (unsigned)D + (unsigned)c0) * 4u, v);
                            }
                        }
                        return 4;
                    });
            });
        }
    });
}

template <int D>
int gcn_panel_pack(const float* W, int transpose, float* img, hipStream_t st) {
    hipLaunchKernelGGL((gcn_panel_pack_kernel<D>), dim3(8, PanelCfg<D>::NP), dim3(256), 0, st, W, transpose, img);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D, bool BWD = false>
int gcn_panel_launch(const float* x, const int* row_ptr, const int* col, const float* val, int nnz, const float* img,
                     const GcnEpilogue& ep, float* out, float* s_out, int V, hipStream_t st, const float* gate_out = nullptr) {
    return panel_launch<&gcn_panel_layer_kernel<D, BWD>>((size_t)2 * GcnPanelImg<D>::PART_BYTES, 48 * 1024, panel_blocks(V, kGcnPanelNW), st,
                                                          x, row_ptr, col, val, nnz, img, ep, out, s_out, V, gate_out);
}

template <int D>
int gcn_panel_train_pack(const float* const* W, int L, float* images, hipStream_t st) {
    GcnPanelPackList w{};
    for (int l = 0; l < L; ++l) w.W[l] = W[l];
    const unsigned slot_floats = (unsigned)(align256g(gcn_panel_layer_image_bytes<D>()) / sizeof(float));
    hipLaunchKernelGGL((gcn_panel_train_pack_kernel<D>), dim3(8, PanelCfg<D>::NP, (unsigned)(2 * L - 1)), dim3(256), 0, st, w, L, images,
                       slot_floats);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

int gcn_panel_dispatch(const float* x, const int* row_ptr, const int* col, const float* val, int nnz, const float* img,
                       const GcnEpilogue& ep, float* out, float* s_out, int V, int D, hipStream_t st) {
    return panel_for_D(D, [&](auto d) { return gcn_panel_launch<decltype(d)::value>(x, row_ptr, col, val, nnz, img, ep, out, s_out, V, st); });
}

// the layer backward: out = relu_gate(dropout(A_hat^T (dP W^T)), gate_out)
int gcn_panel_dispatch_bwd(const float* dP, const int* row_ptr_t, const int* col_t, const float* val_t, int nnz, const float* img_T,
                           const GcnEpilogue& ep, const float* gate_out, float* out, int V, int D, hipStream_t st) {
    return panel_for_D(D, [&](auto d) {
        return gcn_panel_launch<decltype(d)::value, true>(dP, row_ptr_t, col_t, val_t, nnz, img_T, ep, out, nullptr, V, st, gate_out);
    });
}

int gcn_panel_unsupported(int D) {
    return fail(GGNN_E_UNSUPPORTED, "panel GCN layer supports hidden sizes 128, 192, 256 (got %d)", D);
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_gcn_panel_supported(int D) { return panel_hidden_ok(D); }

extern "C" size_t ggnn_gcn_panel_image_bytes(int D) {
    if (!panel_hidden_ok(D)) return 0;
    return panel_for_D(D, [](auto d) { return gcn_panel_layer_image_bytes<decltype(d)::value>(); });
}

extern "C" void ggnn_gcn_panel_launch_geometry(int* rows_per_workgroup, int* max_workgroups) {
    if (rows_per_workgroup) *rows_per_workgroup = kGcnPanelNW * 16;
    if (max_workgroups) *max_workgroups = num_cus();
}

extern "C" int ggnn_gcn_panel_pack_weights_f32(const float* W, int D, int transpose, float* img, ggnn_stream_t stream) {
    if (!ggnn_gcn_panel_supported(D)) return gcn_panel_unsupported(D);
    GGNN_CHECK_ARG(W && img && aligned16(img), "null or misaligned pointer");
    return panel_for_D(D, [&](auto d) { return gcn_panel_pack<decltype(d)::value>(W, transpose, img, (hipStream_t)stream); });
}

extern "C" int ggnn_gcn_panel_layer_f32(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                                        const float* img, const float* bias, int relu, const int64_t* row_key, int64_t row_key_base,
                                        uint64_t seed, float keep_prob, float* out, float* s_out, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d nnz=%lld", V, (long long)nnz);
    if (!ggnn_gcn_panel_supported(D)) return gcn_panel_unsupported(D);
    GGNN_CHECK_ARG(gcn_epilogue_args(bias, keep_prob), "keep_prob %g outside (0, 1] or misaligned bias", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(x && row_ptr && img && out && (nnz == 0 || (col && val)), "null pointer");
    GGNN_CHECK_ARG(aligned16(x) && aligned16(img) && aligned16(out) && (!s_out || aligned16(s_out)), "pointers must be 16-byte aligned");
    GGNN_CHECK_ARG(x != out && (!s_out || (s_out != x && s_out != out)), "out / s_out must not alias x");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    const GcnEpilogue ep{bias, relu ? 1 : 0, row_key, row_key_base, (uint32_t)seed, (uint32_t)(seed >> 32), keep_prob};
    return gcn_panel_dispatch(x, row_ptr, col, val, (int)nnz, img, ep, out, s_out, V, D, (hipStream_t)stream);
}

extern "C" int ggnn_gcn_panel_layer_bwd_f32(const float* dP, const int32_t* row_ptr_t, const int32_t* col_t, const float* val_t,
                                            int64_t nnz, const float* img_T, const float* gate_out, const int64_t* row_key,
                                            int64_t row_key_base, uint64_t seed, float keep_prob, float* out, int V, int D,
                                            ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d nnz=%lld", V, (long long)nnz);
    if (!ggnn_gcn_panel_supported(D)) return gcn_panel_unsupported(D);
    GGNN_CHECK_ARG(gcn_epilogue_args(nullptr, keep_prob), "keep_prob %g outside (0, 1]", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(dP && row_ptr_t && img_T && out && gate_out && (nnz == 0 || (col_t && val_t)), "null pointer");
    GGNN_CHECK_ARG(aligned16(dP) && aligned16(img_T) && aligned16(out) && aligned16(gate_out), "pointers must be 16-byte aligned");
    GGNN_CHECK_ARG(dP != out && gate_out != out, "out must not alias dP or gate_out");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    const GcnEpilogue ep{nullptr, 0, row_key, row_key_base, (uint32_t)seed, (uint32_t)(seed >> 32), keep_prob};
    return gcn_panel_dispatch_bwd(dP, row_ptr_t, col_t, val_t, (int)nnz, img_T, ep, gate_out, out, V, D, (hipStream_t)stream);
}

extern "C" int ggnn_gcn_panel_train_pack_f32(const float* const* W, int num_layers, int D, float* images, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(num_layers > 0 && num_layers <= kGcnPanelTrainMaxLayers, "layers=%d outside [1, %d]", num_layers,
                   kGcnPanelTrainMaxLayers);
    if (!ggnn_gcn_panel_supported(D)) return gcn_panel_unsupported(D);
    GGNN_CHECK_ARG(W && images && aligned16(images), "null or misaligned pointer");
    for (int l = 0; l < num_layers; ++l) GGNN_CHECK_ARG(W[l] != nullptr, "null weight pointer of layer %d", l);
    return panel_for_D(D, [&](auto d) { return gcn_panel_train_pack<decltype(d)::value>(W, num_layers, images, (hipStream_t)stream); });
}

extern "C" size_t ggnn_gcn_panel_workspace_bytes(int V, int D, int num_layers) {
    if (V < 0 || num_layers <= 0 || !ggnn_gcn_panel_supported(D)) return 256;
    return 256 + (size_t)num_layers * align256g(ggnn_gcn_panel_image_bytes(D)) + 2 * align256g((size_t)V * D * sizeof(float));
}

// ggnn_gcn_propagate_f32 at the panel sizes: the weight images are packed into ws, the states ping-pong between two [V, D] buffers of
// ws, the last layer (linear) writes `out`.  W / bias: HOST arrays of num_layers device pointers (bias may be NULL).
extern "C" int ggnn_gcn_panel_propagate_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                                            const float* val, int64_t nnz, const float* const* W, const float* const* bias, float* out,
                                            void* ws, size_t ws_bytes, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && num_layers > 0 && num_layers <= 64 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d layers=%d",
                   V, num_layers);
    if (!ggnn_gcn_panel_supported(D)) return gcn_panel_unsupported(D);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && row_ptr && W && out && ws && (nnz == 0 || (col && val)), "null pointer");
    GGNN_CHECK_ARG(aligned16(h0) && aligned16(out), "pointers must be 16-byte aligned");
    for (int l = 0; l < num_layers; ++l) {
        GGNN_CHECK_ARG(W[l] != nullptr, "null weight pointer of layer %d", l);
        GGNN_CHECK_ARG(!bias || (bias[l] && aligned16(bias[l])), "null or misaligned bias pointer of layer %d", l);
    }
    GGNN_CHECK_ARG(h0 != out, "out must not alias h0");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    if (ws_bytes < ggnn_gcn_panel_workspace_bytes(V, D, num_layers))
        return fail(GGNN_E_WORKSPACE, "GCN workspace too small: %zu < %zu", ws_bytes, ggnn_gcn_panel_workspace_bytes(V, D, num_layers));
    hipStream_t st = (hipStream_t)stream;
    char* p = reinterpret_cast<char*>(align256g(reinterpret_cast<size_t>(ws)));
    const size_t img_bytes = align256g(ggnn_gcn_panel_image_bytes(D)), state_bytes = align256g((size_t)V * D * sizeof(float));
    float* buf[2] = {reinterpret_cast<float*>(p + num_layers * img_bytes), reinterpret_cast<float*>(p + num_layers * img_bytes + state_bytes)};
    const float* cur = h0;
    for (int l = 0; l < num_layers; ++l) {
        float* img = reinterpret_cast<float*>(p + l * img_bytes);
        if (int rc = ggnn_gcn_panel_pack_weights_f32(W[l], D, 0, img, stream)) return rc;
        const bool last = l == num_layers - 1;
        float* dst = last ? out : buf[l & 1];
        const GcnEpilogue ep{bias ? bias[l] : nullptr, last ? 0 : 1, nullptr, 0, 0u, 0u, 1.0f};
        if (int rc = gcn_panel_dispatch(cur, row_ptr, col, val, (int)nnz, img, ep, dst, nullptr, V, D, st)) return rc;
        cur = dst;
    }
    return GGNN_OK;
}
