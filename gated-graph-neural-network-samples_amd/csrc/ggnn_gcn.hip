// One Kipf-style GCN layer (chem_tensorflow_gcn.py:68-80) in one launch:
//
//     S   = A_hat x            A_hat sparse (CSR: row_ptr, col, val), x [V, D]
//     out = dropout(relu(S W + b))     (bias, ReLU and dropout each optional)
//
// Aggregate first, then transform -- the reference's order -- with no [V, D] intermediate in HBM.  The structure is that of the
// compacted message transform (ggnn_msg_compact.hip): a workgroup brings the D x D weight image into LDS once (LDS-DMA), then
// each wave walks over 16-row tiles.  There the A operand of a tile is 16 gathered state rows; here each lane builds its part of
// the A fragment as the weighted CSR sum of its row, S[i, :] = sum_{k in row_ptr[i] .. row_ptr[i+1]} val[k] * x[col[k], :], one
// fmaf chain per element in slot order (deterministic, no atomics).  The product S W runs on the bf16 matrix pipe in the exact
// three-piece split form (ggnn_split.hpp); the epilogue adds the bias, applies ReLU and the counter-based dropout of
// ggnn_dropout_f32 (same Philox counter and key per (row key, column quad): bit-identical masks).  Optionally S is stored too
// (the training path's dW = S^T dP).
//
// The backward pass reuses the kernel: dx = A_hat^T (dP W^T) = (A_hat^T dP) W^T, i.e. the same launch on the transposed CSR with
// the image of W^T (ggnn_gcn_pack_weights_f32(transpose = 1)).  Its BWD instantiation (ggnn_gcn_layer_bwd_f32) goes one step
// further and writes the dP of the layer BELOW: the epilogue applies that layer's dropout mask and the ReLU gate of its forward
// output gate_out = dropout(relu(P)), read at the lane's own row and column quad -- the two element-wise launches
// (ggnn_dropout_f32, ggnn_act_bwd_f32) and their [V, D] round trips between two layer launches are gone.  The gather, split, product
// and tile walk are the forward's; BWD is a template parameter, so the forward instantiations keep their code and registers.
//
// Memory per layer at V = 1e5, D = 100, ~3.1 nonzeros per row: x is read ~once through L2 (each row is gathered by ~3 neighbours
// of nearby rows), out written once, the CSR read once -- about 83 MB, against ~245 MB for the segment sum + GEMM + epilogue
// composition.
#include "ggnn_gcn.hpp"

namespace ggnn {
namespace {

constexpr int kGcnNW = 8;                                          // waves per workgroup; two workgroups per CU

template <int D>
using GcnImg = SplitCfg<D, kSplitBf16x3>;

template <int D>
__global__ void gcn_pack_kernel(const float* __restrict__ W, int transpose, float* __restrict__ img) {
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (transpose) pack_split_image<D, kSplitBf16x3>(StageValueT<D>{W, 0, 0, D}, img, first, stride);
    else pack_split_image<D, kSplitBf16x3>(StageValue<D>{W, 0, 0, D, -1, nullptr, 0, 0, -1}, img, first, stride);
}

// Every weight image of a training step in ONE launch (2L launches of gcn_pack_kernel before): blockIdx.y = slot j of `images`,
// slot j < L the image of W_j, slot L + (l - 1) the image of W_l^T for l >= 1 (layer 0 forms no dx).  pack_split_image writes word i
// as a function of (i, W) alone: the images are gcn_pack_kernel's bit for bit whatever the grid.
constexpr int kGcnTrainMaxLayers = 64;
struct GcnPackList { const float* W[kGcnTrainMaxLayers]; };

template <int D>
__global__ __launch_bounds__(256) void gcn_train_pack_kernel(GcnPackList w, int L, float* __restrict__ images, unsigned slot_floats) {
    const int j = blockIdx.y;
    const bool transpose = j >= L;
    const float* W = w.W[transpose ? j - L + 1 : j];
    float* img = images + (size_t)j * slot_floats;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    if (transpose) pack_split_image<D, kSplitBf16x3>(StageValueT<D>{W, 0, 0, D}, img, first, stride);
    else pack_split_image<D, kSplitBf16x3>(StageValue<D>{W, 0, 0, D, -1, nullptr, 0, 0, -1}, img, first, stride);
}

// BWD: x = dP of this layer, (row_ptr, col, val) = the transposed CSR, packed = the image of W^T, ep = the dropout of the layer
// below (no bias, no ReLU), gate_out [V, D] = that layer's forward output; out = its dP.  s_out is not written.
template <int D, bool BWD = false>
__global__ __launch_bounds__(kGcnNW * 64, 4) /* 4 waves per SIMD = 2 workgroups per CU, <= 128 VGPRs */ void gcn_layer_kernel(
        const float* __restrict__ x, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ val,
        int nnz, const float* __restrict__ packed, GcnEpilogue ep, float* __restrict__ out, float* __restrict__ s_out, int V,
        const float* __restrict__ gate_out) {
    using S = StageCfg<D>;
    using I = GcnImg<D>;
    constexpr int NT = S::NT;
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int n_tiles = (V + 15) / 16;
    const int stride = gridDim.x * kGcnNW;

    dma_image_asm<I::IMG_BYTES, kGcnNW>(packed, img, wave, lane);
    dma_wait();
    __syncthreads();                                        // the image has landed

    for (int idx = blockIdx.x * kGcnNW + wave; idx < n_tiles; idx += stride) {
        const int r = idx * 16 + li;
        int beg = 0, end = 0;
        if (r < V) {
            // (clamped to [0, nnz]: a corrupt row_ptr cannot send the gather out of the index arrays)
            beg = min(max(row_ptr[r], 0), nnz);
            end = min(max(row_ptr[r + 1], beg), nnz);
        }
        Frag<D> a;
#pragma unroll
        for (int c = 0; c < S::NC; ++c) a.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < S::NR; ++q) a.r[q] = 0.f;
        // two gathered rows in flight per iteration; the sum stays in slot order.  A column index outside [0, V) contributes
        // nothing (the host layer validates the CSR; the kernel only guarantees that it never reads outside x).
        int k = beg;
        for (; k + 1 < end; k += 2) {
            const int j0 = col[k], j1 = col[k + 1];
            const float w0 = val[k], w1 = val[k + 1];
            const bool ok0 = (unsigned)j0 < (unsigned)V, ok1 = (unsigned)j1 < (unsigned)V;
            Frag<D> t0, t1;
            load_frag<D>(t0, x, ok0 ? j0 : 0, kq);
            load_frag<D>(t1, x, ok1 ? j1 : 0, kq);
            frag_fma<D>(a, ok0 ? w0 : 0.f, t0);
            frag_fma<D>(a, ok1 ? w1 : 0.f, t1);
        }
        if (k < end) {
            const int j0 = col[k];
            const bool ok0 = (unsigned)j0 < (unsigned)V;
            Frag<D> t0;
            load_frag<D>(t0, x, ok0 ? j0 : 0, kq);
            frag_fma<D>(a, ok0 ? val[k] : 0.f, t0);
        }
        if (!BWD && s_out && r < V) {
            const unsigned ob = ((unsigned)r * (unsigned)D + 4u * (unsigned)kq) * 4u;
#pragma unroll
            for (int c = 0; c < S::NC; ++c) st4_b(s_out, ob + 64u * c, a.v[c]);
#pragma unroll
            for (int q = 0; q < S::NR; ++q) s_out[(size_t)r * D + 16 * S::NC + 4 * q + kq] = a.r[q];
        }
        f32x4 acc[NT];
        SFrag<D> sf;
        split_frag<D, kSplitBf16x3>(sf, a);
        stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc, sf, a, img, li, kq);
        if (r < V) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c0 = nt * 16 + 4 * kq;
                if (c0 < D) {
                    const unsigned ob = ((unsigned)r * (unsigned)D + c0) * 4u;
                    f32x4 v = gcn_epilogue(acc[nt], r, c0, ep);
                    if constexpr (BWD) v = gcn_relu_gate(v, ld4_b(gate_out, ob));
                    st4_b(out, ob, v);
                }
            }
        }
    }
}

// the composed path's epilogue (hidden sizes without the fused kernel): out = dropout(relu(P + b)), one thread per column quad
__global__ __launch_bounds__(256) void gcn_epilogue_kernel(const float* __restrict__ P, GcnEpilogue ep, float* __restrict__ out,
                                                            int V, int D) {
    const int quads = D / 4;
    const long long total = (long long)V * quads;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / quads), c0 = 4 * (int)(i - (long long)r * quads);
        const size_t off = (size_t)r * D + c0;
        *reinterpret_cast<f32x4*>(out + off) = gcn_epilogue(*reinterpret_cast<const f32x4*>(P + off), r, c0, ep);
    }
}

template <int D>
int gcn_pack(const float* W, int transpose, float* img, hipStream_t st) {
    hipLaunchKernelGGL((gcn_pack_kernel<D>), dim3(16), dim3(256), 0, st, W, transpose, img);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D>
int gcn_train_pack(const float* const* W, int L, float* images, hipStream_t st) {
    GcnPackList w{};
    for (int l = 0; l < L; ++l) w.W[l] = W[l];
    const unsigned slot_floats = (unsigned)(align256g(GcnImg<D>::IMG_BYTES) / sizeof(float));
    hipLaunchKernelGGL((gcn_train_pack_kernel<D>), dim3(16, (unsigned)(2 * L - 1)), dim3(256), 0, st, w, L, images, slot_floats);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D, bool BWD = false>
int gcn_launch(const float* x, const int* row_ptr, const int* col, const float* val, int nnz, const float* img,
               const GcnEpilogue& ep, float* out, float* s_out, int V, hipStream_t st, const float* gate_out = nullptr) {
    constexpr int BYTES = GcnImg<D>::IMG_BYTES;
    static std::atomic<unsigned long long> lds_ok{0};
    if (BYTES > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&gcn_layer_kernel<D, BWD>, BYTES, lds_ok));
    const long long n_tiles = (V + 15) / 16;
    const long long blocks = std::min<long long>((n_tiles + kGcnNW - 1) / kGcnNW, 2LL * num_cus());
    hipLaunchKernelGGL((gcn_layer_kernel<D, BWD>), dim3((unsigned)blocks), dim3(kGcnNW * 64), BYTES, st, x, row_ptr, col, val, nnz, img,
                       ep, out, s_out, V, gate_out);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

int gcn_dispatch(const float* x, const int* row_ptr, const int* col, const float* val, int nnz, const float* img,
                 const GcnEpilogue& ep, float* out, float* s_out, int V, int D, hipStream_t st) {
    switch (D) {
        case 100: return gcn_launch<100>(x, row_ptr, col, val, nnz, img, ep, out, s_out, V, st);
        case 64: return gcn_launch<64>(x, row_ptr, col, val, nnz, img, ep, out, s_out, V, st);
        default: return gcn_launch<32>(x, row_ptr, col, val, nnz, img, ep, out, s_out, V, st);
    }
}

// the layer backward: out = relu_gate(dropout(A_hat^T (dP W^T)), gate_out)
int gcn_dispatch_bwd(const float* dP, const int* row_ptr_t, const int* col_t, const float* val_t, int nnz, const float* img_T,
                     const GcnEpilogue& ep, const float* gate_out, float* out, int V, int D, hipStream_t st) {
    switch (D) {
        case 100: return gcn_launch<100, true>(dP, row_ptr_t, col_t, val_t, nnz, img_T, ep, out, nullptr, V, st, gate_out);
        case 64: return gcn_launch<64, true>(dP, row_ptr_t, col_t, val_t, nnz, img_T, ep, out, nullptr, V, st, gate_out);
        default: return gcn_launch<32, true>(dP, row_ptr_t, col_t, val_t, nnz, img_T, ep, out, nullptr, V, st, gate_out);
    }
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_gcn_fused_supported(int D) { return D == 32 || D == 64 || D == 100; }

extern "C" size_t ggnn_gcn_image_bytes(int D) {
    switch (D) {
        case 100: return GcnImg<100>::IMG_BYTES;
        case 64: return GcnImg<64>::IMG_BYTES;
        case 32: return GcnImg<32>::IMG_BYTES;
        default: return 0;
    }
}

extern "C" int ggnn_gcn_pack_weights_f32(const float* W, int D, int transpose, float* img, ggnn_stream_t stream) {
    if (!ggnn_gcn_fused_supported(D)) return fail(GGNN_E_UNSUPPORTED, "fused GCN layer supports hidden sizes 32, 64, 100 (got %d)", D);
    GGNN_CHECK_ARG(W && img && aligned16(img), "null or misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return gcn_pack<100>(W, transpose, img, st);
        case 64: return gcn_pack<64>(W, transpose, img, st);
        default: return gcn_pack<32>(W, transpose, img, st);
    }
}

extern "C" int ggnn_gcn_layer_f32(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                                  const float* img, const float* bias, int relu, const int64_t* row_key, int64_t row_key_base,
                                  uint64_t seed, float keep_prob, float* out, float* s_out, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d nnz=%lld", V, (long long)nnz);
    if (!ggnn_gcn_fused_supported(D)) return fail(GGNN_E_UNSUPPORTED, "fused GCN layer supports hidden sizes 32, 64, 100 (got %d)", D);
    GGNN_CHECK_ARG(gcn_epilogue_args(bias, keep_prob), "keep_prob %g outside (0, 1] or misaligned bias", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(x && row_ptr && img && out && (nnz == 0 || (col && val)), "null pointer");
    GGNN_CHECK_ARG(aligned16(x) && aligned16(img) && aligned16(out) && (!s_out || aligned16(s_out)), "pointers must be 16-byte aligned");
    GGNN_CHECK_ARG(x != out && (!s_out || (s_out != x && s_out != out)), "out / s_out must not alias x");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    const GcnEpilogue ep{bias, relu ? 1 : 0, row_key, row_key_base, (uint32_t)seed, (uint32_t)(seed >> 32), keep_prob};
    return gcn_dispatch(x, row_ptr, col, val, (int)nnz, img, ep, out, s_out, V, D, (hipStream_t)stream);
}

extern "C" int ggnn_gcn_layer_bwd_f32(const float* dP, const int32_t* row_ptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                                      const float* img_T, const float* gate_out, const int64_t* row_key, int64_t row_key_base,
                                      uint64_t seed, float keep_prob, float* out, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d nnz=%lld", V, (long long)nnz);
    if (!ggnn_gcn_fused_supported(D)) return fail(GGNN_E_UNSUPPORTED, "fused GCN layer supports hidden sizes 32, 64, 100 (got %d)", D);
    GGNN_CHECK_ARG(gcn_epilogue_args(nullptr, keep_prob), "keep_prob %g outside (0, 1]", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(dP && row_ptr_t && img_T && out && gate_out && (nnz == 0 || (col_t && val_t)), "null pointer");
    GGNN_CHECK_ARG(aligned16(dP) && aligned16(img_T) && aligned16(out) && aligned16(gate_out), "pointers must be 16-byte aligned");
    GGNN_CHECK_ARG(dP != out && gate_out != out, "out must not alias dP or gate_out");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    const GcnEpilogue ep{nullptr, 0, row_key, row_key_base, (uint32_t)seed, (uint32_t)(seed >> 32), keep_prob};
    return gcn_dispatch_bwd(dP, row_ptr_t, col_t, val_t, (int)nnz, img_T, ep, gate_out, out, V, D, (hipStream_t)stream);
}

extern "C" int ggnn_gcn_train_pack_f32(const float* const* W, int num_layers, int D, float* images, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(num_layers > 0 && num_layers <= kGcnTrainMaxLayers, "layers=%d outside [1, %d]", num_layers, kGcnTrainMaxLayers);
    if (!ggnn_gcn_fused_supported(D)) return fail(GGNN_E_UNSUPPORTED, "fused GCN layer supports hidden sizes 32, 64, 100 (got %d)", D);
    GGNN_CHECK_ARG(W && images && aligned16(images), "null or misaligned pointer");
    for (int l = 0; l < num_layers; ++l) GGNN_CHECK_ARG(W[l] != nullptr, "null weight pointer of layer %d", l);
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return gcn_train_pack<100>(W, num_layers, images, st);
        case 64: return gcn_train_pack<64>(W, num_layers, images, st);
        default: return gcn_train_pack<32>(W, num_layers, images, st);
    }
}

extern "C" int ggnn_gcn_epilogue_f32(const float* P, const float* bias, int relu, const int64_t* row_key, int64_t row_key_base,
                                     uint64_t seed, float keep_prob, float* out, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && D % 4 == 0, "bad sizes V=%d D=%d", V, D);
    GGNN_CHECK_ARG(gcn_epilogue_args(bias, keep_prob), "keep_prob %g outside (0, 1] or misaligned bias", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(P && out && aligned16(P) && aligned16(out), "null or misaligned pointer");
    const GcnEpilogue ep{bias, relu ? 1 : 0, row_key, row_key_base, (uint32_t)seed, (uint32_t)(seed >> 32), keep_prob};
    const long long total = (long long)V * (D / 4);
    const int blocks = (int)std::min<long long>((total + 255) / 256, (long long)num_cus() * 16);
    hipLaunchKernelGGL(gcn_epilogue_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, ep, out, V, D);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

extern "C" size_t ggnn_gcn_workspace_bytes(int V, int D, int num_layers) {
    if (V < 0 || num_layers <= 0 || !ggnn_gcn_fused_supported(D)) return 256;
    return 256 + (size_t)num_layers * align256g(ggnn_gcn_image_bytes(D)) + 2 * align256g((size_t)V * D * sizeof(float));
}

// All num_layers layers of compute_final_node_representations (chem_tensorflow_gcn.py:62-82, inference: no dropout) behind one
// call: the weight images are packed into ws, the states ping-pong between two [V, D] buffers of ws, the last layer (linear) writes
// `out`.  W / bias: HOST arrays of num_layers device pointers (bias may be NULL: gcn_use_bias off).
extern "C" int ggnn_gcn_propagate_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                                      const float* val, int64_t nnz, const float* const* W, const float* const* bias, float* out,
                                      void* ws, size_t ws_bytes, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && num_layers > 0 && num_layers <= 64 && nnz >= 0 && nnz < (1LL << 31), "bad sizes V=%d layers=%d",
                   V, num_layers);
    if (!ggnn_gcn_fused_supported(D)) return fail(GGNN_E_UNSUPPORTED, "fused GCN layer supports hidden sizes 32, 64, 100 (got %d)", D);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && row_ptr && W && out && ws && (nnz == 0 || (col && val)), "null pointer");
    GGNN_CHECK_ARG(aligned16(h0) && aligned16(out), "pointers must be 16-byte aligned");
    for (int l = 0; l < num_layers; ++l) {
        GGNN_CHECK_ARG(W[l] != nullptr, "null weight pointer of layer %d", l);
        GGNN_CHECK_ARG(!bias || (bias[l] && aligned16(bias[l])), "null or misaligned bias pointer of layer %d", l);
    }
    GGNN_CHECK_ARG(h0 != out, "out must not alias h0");
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    if (ws_bytes < ggnn_gcn_workspace_bytes(V, D, num_layers))
        return fail(GGNN_E_WORKSPACE, "GCN workspace too small: %zu < %zu", ws_bytes, ggnn_gcn_workspace_bytes(V, D, num_layers));
    hipStream_t st = (hipStream_t)stream;
    char* p = reinterpret_cast<char*>(align256g(reinterpret_cast<size_t>(ws)));
    const size_t img_bytes = align256g(ggnn_gcn_image_bytes(D)), state_bytes = align256g((size_t)V * D * sizeof(float));
    float* buf[2] = {reinterpret_cast<float*>(p + num_layers * img_bytes), reinterpret_cast<float*>(p + num_layers * img_bytes + state_bytes)};
    const float* cur = h0;
    for (int l = 0; l < num_layers; ++l) {
        float* img = reinterpret_cast<float*>(p + l * img_bytes);
        if (int rc = ggnn_gcn_pack_weights_f32(W[l], D, 0, img, stream)) return rc;
        const bool last = l == num_layers - 1;
        float* dst = last ? out : buf[l & 1];
        const GcnEpilogue ep{bias ? bias[l] : nullptr, last ? 0 : 1, nullptr, 0, 0u, 0u, 1.0f};
        if (int rc = gcn_dispatch(cur, row_ptr, col, val, (int)nnz, img, ep, dst, nullptr, V, D, st)) return rc;
        cur = dst;
    }
    return GGNN_OK;
}
