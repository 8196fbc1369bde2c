// The optimisation step of the sparse GCN (chem_tensorflow.py:183-191 over chem_tensorflow_gcn.py:62-82) as native launch sequences,
// the GCN twin of ggnn_train.hip / ggnn_dense_train.hip.  ggnn_gcn_train_forward_f32 enqueues one launch that builds every weight
// image of the step (ggnn_gcn_train_pack_f32: W_l for the forward, W_l^T for the backward of the layers l >= 1) and the L fused layer
// launches (ggnn_gcn_layer_f32), which keep S_l = A_hat h_l and the layer outputs in a caller-provided workspace.
// ggnn_gcn_train_backward_f32 walks the layers down: with dP_{L-1} = d_final (the last layer is linear),
//
//     side stream:  g_W[l] += S_l^T dP_l  (ggnn_xty_acc_f32),  g_b[l] += colsum(dP_l)  (ggnn_colsum_f32, with biases only)
//     main stream:  dP_{l-1} = gate(dropout(A_hat^T (dP_l W_l^T)))          one ggnn_gcn_layer_bwd_f32, l >= 1 (h0 is data: no dx of layer 0)
//
// -- all ADDED into the optimizer's gradient buffers, which the caller zeroes.  Between the two calls the host runs the readout +
// loss (ggnn_readout_loss_{fwd,bwd}_f32).  Nothing is allocated (one workspace, laid out by gcn_layout below), nothing synchronises.
//
// Why: through torch.autograd every layer's backward is a dropout and an activation-gradient launch over [V, D], a ggnn_gemm_tn_f32
// and a ggnn_colsum_f32 for the weight and bias gradients and a fresh weight-image launch in each direction (gcn_model.GCNLayerFn).
//
// The bias gradient is NOT the ones row of the product, although ggnn_xty_acc_f32 offers it in the same pass: measured against
// float64 on ~2000-row batches the ones row lands at one f32 epsilon of the largest entry, ggnn_colsum_f32's 256-block tree at half
// of one, and the step is held to twice the autograd route's own error.  With ggnn_colsum_f32 on the same dP bits the bias
// gradients are the autograd route's bit for bit; the two small launches ride on the side stream.
//
// Cross-stream hazards.  The product of layer l reads S_l (written by the forward call, main stream, before this call) and dP_l
// (written by the layer-backward launch of layer l + 1 on the main stream, or the caller's d_final): the side stream is ordered
// behind the main stream by one event per layer, recorded after that launch.  Every layer has its OWN dP buffer, so the main
// stream's next launch (which writes dP_{l-1} and reads dP_l and the output of layer l - 1) touches nothing the side stream writes,
// and writes nothing it reads: no write-after-read hazard inside a step.  The products write g_W[l] / g_b[l], which nothing on the
// main stream touches inside the call; they run serially on the side stream and share one product workspace (and one column-sum
// workspace with its [D] result, added into g_b[l] by a one-block launch behind it).  The call ends with
// the main stream waiting for the side stream's last product: the caller's next launches (optimizer, next forward, which rewrites
// the workspace) see every gradient and overwrite nothing in use.
//
// Two routes share these sequences (GcnTrainRoute below: image size, pack-all, layer, layer backward, supported sizes): the fused
// layer kernels of ggnn_gcn.hip at hidden sizes 32 / 64 / 100 (ggnn_gcn_train_*) and the column-panel kernels of
// ggnn_gcn_panel.hip at 128 / 192 / 256 (ggnn_gcn_panel_train_*).  Workspace layout, streams, events and products are the same.
#include "ggnn_common.h"

namespace ggnn {
namespace {

constexpr int kGcnTrainMaxLayers = 64;              // ggnn_gcn_train_pack_f32's limit

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// what a route brings: the kernels of one family of hidden sizes behind the signatures both families share
struct GcnTrainRoute {
    int (*supported)(int D);
    size_t (*image_bytes)(int D);
    int (*pack_all)(const float* const* W, int num_layers, int D, float* images, ggnn_stream_t stream);
    int (*layer)(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int64_t nnz, const float* img,
                 const float* bias, int relu, const int64_t* row_key, int64_t row_key_base, uint64_t seed, float keep_prob, float* out,
                 float* s_out, int V, int D, ggnn_stream_t stream);
    int (*layer_bwd)(const float* dP, const int32_t* row_ptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                     const float* img_T, const float* gate_out, const int64_t* row_key, int64_t row_key_base, uint64_t seed,
                     float keep_prob, float* out, int V, int D, ggnn_stream_t stream);
    const char* sizes;                                 // for the error message
};

const GcnTrainRoute kGcnFusedRoute{ggnn_gcn_train_supported, ggnn_gcn_image_bytes, ggnn_gcn_train_pack_f32, ggnn_gcn_layer_f32,
                                   ggnn_gcn_layer_bwd_f32, "32, 64, 100"};
const GcnTrainRoute kGcnPanelRoute{ggnn_gcn_panel_train_supported, ggnn_gcn_panel_image_bytes, ggnn_gcn_panel_train_pack_f32,
                                   ggnn_gcn_panel_layer_f32, ggnn_gcn_panel_layer_bwd_f32, "128, 192, 256"};

struct GcnTrainLayout {
    size_t images, S, H, dP, xty, colsum, db, total;   // byte offsets from the 256-aligned base; S / H / dP: L buffers of `state` bytes each
    size_t slot, state, xty_bytes, colsum_bytes;
};

GcnTrainLayout gcn_layout(const GcnTrainRoute& rt, int V, int D, int L) {
    GcnTrainLayout o{};
    o.slot = al256(rt.image_bytes(D));
    o.state = al256((size_t)V * D * sizeof(float));
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += al256(bytes); return at; };
    o.images = take((size_t)(2 * L - 1) * o.slot);
    o.S = take((size_t)L * o.state);
    o.H = take((size_t)L * o.state);
    o.dP = take((size_t)L * o.state);
    o.xty_bytes = ggnn_xty_workspace_bytes(V, D, D, 1);
    o.xty = take(o.xty_bytes);
    o.colsum_bytes = ggnn_colsum_workspace_bytes(D);
    o.colsum = take(o.colsum_bytes);
    o.db = take((size_t)D * sizeof(float));
    o.total = p + 256;                              // (the base is aligned inside the caller's buffer)
    return o;
}

// g[i] += t[i]: the column sums of one layer into the caller's (accumulating) bias-gradient buffer
__global__ __launch_bounds__(256) void gcn_bias_add_kernel(float* __restrict__ g, const float* __restrict__ t, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = g[i] + t[i];
}

int check_shape(const GcnTrainRoute& rt, int V, int D, int L) {
    GGNN_CHECK_ARG(V >= 0 && L >= 1 && L <= kGcnTrainMaxLayers, "bad sizes V=%d layers=%d", V, L);
    if (!rt.supported(D))
        return fail(GGNN_E_UNSUPPORTED, "native GCN training step: hidden sizes %s on this route (got %d)", rt.sizes, D);
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    return GGNN_OK;
}

size_t gcn_train_workspace_bytes(const GcnTrainRoute& rt, int V, int D, int num_layers) {
    if (V < 0 || num_layers <= 0 || !rt.supported(D)) return 0;
    return gcn_layout(rt, V, D, num_layers).total;
}

int gcn_train_forward(const GcnTrainRoute& rt, const float* h0, int V, int D, int num_layers, const int32_t* row_ptr,
                      const int32_t* col, const float* val, int64_t nnz, const float* const* W, const float* const* bias,
                      const int64_t* row_key, const uint64_t* seeds, float keep_prob, void* ws, size_t ws_bytes, int64_t* final_off,
                      ggnn_stream_t stream) {
    const int L = num_layers;
    if (int rc = check_shape(rt, V, D, L)) return rc;
    GGNN_CHECK_ARG(nnz >= 0 && nnz < (1LL << 31), "bad nnz=%lld", (long long)nnz);
    GGNN_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "keep_prob %g outside (0, 1]", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && row_ptr && W && ws && final_off && (nnz == 0 || (col && val)), "null pointer");
    GGNN_CHECK_ARG(keep_prob >= 1.0f || L == 1 || seeds, "dropout needs the layers' seeds");
    for (int l = 0; l < L; ++l) {
        GGNN_CHECK_ARG(W[l] != nullptr, "null weight pointer of layer %d", l);
        GGNN_CHECK_ARG(!bias || (bias[l] && aligned16(bias[l])), "null or misaligned bias pointer of layer %d", l);
    }
    const GcnTrainLayout o = gcn_layout(rt, V, D, L);
    if (ws_bytes < o.total) return fail(GGNN_E_WORKSPACE, "GCN training workspace too small: %zu < %zu", ws_bytes, o.total);
    char* base = reinterpret_cast<char*>(al256(reinterpret_cast<size_t>(ws)));
    auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };

    if (int rc = rt.pack_all(W, L, D, f(o.images), stream)) return rc;
    const float* cur = h0;
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;                                     // ReLU and dropout on all but the last layer (:75-78)
        const bool drop = !last && keep_prob < 1.0f;
        float* out = f(o.H + (size_t)l * o.state);
        if (int rc = rt.layer(cur, row_ptr, col, val, nnz, f(o.images + (size_t)l * o.slot), bias ? bias[l] : nullptr, last ? 0 : 1,
                              row_key, 0, drop ? seeds[l] : 0, drop ? keep_prob : 1.0f, out, f(o.S + (size_t)l * o.state), V, D, stream))
            return rc;
        cur = out;
    }
    *final_off = (int64_t)((base - static_cast<char*>(ws)) + o.H + (size_t)(L - 1) * o.state);
    return GGNN_OK;
}

int gcn_train_backward(const GcnTrainRoute& rt, const float* d_final, int V, int D, int num_layers, const int32_t* row_ptr_t,
                       const int32_t* col_t, const float* val_t, int64_t nnz, const int64_t* row_key, const uint64_t* seeds,
                       float keep_prob, float* const* g_W, float* const* g_b, void* ws, size_t ws_bytes, ggnn_stream_t stream,
                       ggnn_stream_t side_stream) {
    const int L = num_layers;
    if (int rc = check_shape(rt, V, D, L)) return rc;
    GGNN_CHECK_ARG(nnz >= 0 && nnz < (1LL << 31), "bad nnz=%lld", (long long)nnz);
    GGNN_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f, "keep_prob %g outside (0, 1]", (double)keep_prob);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(d_final && aligned16(d_final) && row_ptr_t && g_W && ws && (nnz == 0 || (col_t && val_t)), "null or misaligned pointer");
    GGNN_CHECK_ARG(keep_prob >= 1.0f || L == 1 || seeds, "dropout needs the layers' seeds");
    for (int l = 0; l < L; ++l) {
        GGNN_CHECK_ARG(g_W[l] != nullptr, "null weight-gradient pointer of layer %d", l);
        GGNN_CHECK_ARG(!g_b || g_b[l] != nullptr, "null bias-gradient pointer of layer %d", l);
    }
    const GcnTrainLayout o = gcn_layout(rt, V, D, L);
    if (ws_bytes < o.total) return fail(GGNN_E_WORKSPACE, "GCN training workspace too small: %zu < %zu", ws_bytes, o.total);
    char* base = reinterpret_cast<char*>(al256(reinterpret_cast<size_t>(ws)));
    auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    hipStream_t st = (hipStream_t)stream, side = side_stream ? (hipStream_t)side_stream : (hipStream_t)stream;
    const bool drop = keep_prob < 1.0f;
    const int32_t row_off[2] = {0, V};
    const int32_t ldx[1] = {D};

    const float* dP = d_final;                                            // dP_{L-1}: the last layer is linear
    for (int l = L - 1; l >= 0; --l) {
        // ---- side stream: g_W[l] += S_l^T dP_l; with biases g_b[l] += colsum(dP_l) (see the file header: not the ones row) ----
        if (int rc = stream_order_after(side, st)) return rc;
        const float* X[1] = {f(o.S + (size_t)l * o.state)};
        if (int rc = ggnn_xty_acc_f32(X, 1, D, ldx, nullptr, dP, D, g_W[l], nullptr, 1, D, D, 0, row_off, 1, base + o.xty, o.xty_bytes,
                                      (ggnn_stream_t)side))
            return rc;
        if (g_b) {
            if (int rc = ggnn_colsum_f32(dP, D, V, D, f(o.db), base + o.colsum, o.colsum_bytes, (ggnn_stream_t)side)) return rc;
            hipLaunchKernelGGL(gcn_bias_add_kernel, dim3((D + 255) / 256), dim3(256), 0, side, g_b[l], (const float*)f(o.db), D);
            GGNN_CHECK_HIP(hipGetLastError());
        }
        if (l == 0) break;                                                // h0 is data: no dx of layer 0
        // ---- main stream: dP_{l-1} = [out_{l-1} > 0] * mask_{l-1} / keep * A_hat^T (dP_l W_l^T) ----
        float* below = f(o.dP + (size_t)(l - 1) * o.state);
        if (int rc = rt.layer_bwd(dP, row_ptr_t, col_t, val_t, nnz, f(o.images + (size_t)(L + l - 1) * o.slot),
                                  f(o.H + (size_t)(l - 1) * o.state), row_key, 0, drop ? seeds[l - 1] : 0, drop ? keep_prob : 1.0f,
                                  below, V, D, stream))
            return rc;
        dP = below;
    }
    return stream_order_after(st, side);          // the caller's next launches (optimizer, next forward) see every product
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_gcn_train_supported(int D) { return D == 32 || D == 64 || D == 100; }

extern "C" size_t ggnn_gcn_train_workspace_bytes(int V, int D, int num_layers) {
    return gcn_train_workspace_bytes(kGcnFusedRoute, V, D, num_layers);
}

extern "C" int ggnn_gcn_train_forward_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                                          const float* val, int64_t nnz, const float* const* W, const float* const* bias,
                                          const int64_t* row_key, const uint64_t* seeds, float keep_prob, void* ws, size_t ws_bytes,
                                          int64_t* final_off, ggnn_stream_t stream) {
    return gcn_train_forward(kGcnFusedRoute, h0, V, D, num_layers, row_ptr, col, val, nnz, W, bias, row_key, seeds, keep_prob, ws,
                             ws_bytes, final_off, stream);
}

extern "C" int ggnn_gcn_train_backward_f32(const float* d_final, int V, int D, int num_layers, const int32_t* row_ptr_t,
                                           const int32_t* col_t, const float* val_t, int64_t nnz, const int64_t* row_key,
                                           const uint64_t* seeds, float keep_prob, float* const* g_W, float* const* g_b, void* ws,
                                           size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    return gcn_train_backward(kGcnFusedRoute, d_final, V, D, num_layers, row_ptr_t, col_t, val_t, nnz, row_key, seeds, keep_prob, g_W,
                              g_b, ws, ws_bytes, stream, side_stream);
}

// ---- the same sequences on the column-panel kernels (hidden sizes 128 / 192 / 256) ------------------------------------------------
extern "C" int ggnn_gcn_panel_train_supported(int D) { return D == 128 || D == 192 || D == 256; }

extern "C" size_t ggnn_gcn_panel_train_workspace_bytes(int V, int D, int num_layers) {
    return gcn_train_workspace_bytes(kGcnPanelRoute, V, D, num_layers);
}

extern "C" int ggnn_gcn_panel_train_forward_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr,
                                                const int32_t* col, const float* val, int64_t nnz, const float* const* W,
                                                const float* const* bias, const int64_t* row_key, const uint64_t* seeds,
                                                float keep_prob, void* ws, size_t ws_bytes, int64_t* final_off, ggnn_stream_t stream) {
    return gcn_train_forward(kGcnPanelRoute, h0, V, D, num_layers, row_ptr, col, val, nnz, W, bias, row_key, seeds, keep_prob, ws,
                             ws_bytes, final_off, stream);
}

extern "C" int ggnn_gcn_panel_train_backward_f32(const float* d_final, int V, int D, int num_layers, const int32_t* row_ptr_t,
                                                 const int32_t* col_t, const float* val_t, int64_t nnz, const int64_t* row_key,
                                                 const uint64_t* seeds, float keep_prob, float* const* g_W, float* const* g_b, void* ws,
                                                 size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    return gcn_train_backward(kGcnPanelRoute, d_final, V, D, num_layers, row_ptr_t, col_t, val_t, nnz, row_key, seeds, keep_prob, g_W,
                              g_b, ws, ws_bytes, stream, side_stream);
}
