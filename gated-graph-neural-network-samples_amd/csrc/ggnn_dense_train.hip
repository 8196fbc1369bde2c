// The optimisation step of the dense model (chem_tensorflow.py:183-191 over chem_tensorflow_dense.py:93-117) as native launch
// sequences, the dense twin of ggnn_train.hip: ggnn_dense_train_forward_f32 enqueues the saving graph-resident forward
// (ggnn_dense_propagate_save_f32) into a caller-provided workspace, ggnn_dense_train_backward_f32 the graph-resident backward
// (ggnn_dense_propagate_bwd_f32; no gradient of h0, which is data), the two GRU weight-gradient products with their ones rows on a
// side stream (ggnn_xty_acc_f32: dWc, dbc += [x | r*h]^T dpc;  dWg, dbg += [x | h]^T dpg) and the edge-weight / edge-bias gradients
// (ggnn_dense_edge_grad_f32) -- all ADDED into the optimizer's gradient buffers, which the caller zeroes.  Between the two calls the
// host runs the readout + loss (ggnn_readout_loss_{fwd,bwd}_f32).
//
// Why: driven from Python through torch.autograd the same launches cost ~1.1 ms of host time per step (autograd nodes, tensor
// allocations, copies) around 0.13 ms of propagation.  Here a step is two calls; nothing is allocated (one workspace, laid out by
// dense_layout below), nothing synchronises.
//
// Cross-stream hazards.  The side-stream products read the forward's saved tensors and the backward launch's dpc / dpg: they are
// ordered behind the backward launch (and with it behind everything queued on the main stream before, the zeroed gradient buffers
// included) by one event.  They write g_Wg / g_bg / g_Wc / g_bc, which nothing on the main stream touches inside the call; the
// edge-gradient kernel on the main stream writes g_W / g_b and reads dM / dx / saved[0], which the side stream only reads.  The two
// streams have separate product workspaces.  The call ends with the main stream waiting for the side stream's last product: the
// caller's next launches (optimizer, next forward, which rewrites the workspace) see every gradient and overwrite nothing in use.
#include "ggnn_common.h"

namespace ggnn {
namespace {

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

struct DenseTrainLayout {
    size_t saved, out, dpc, dpg, dx, dM, xty, eg, total;
    size_t saved_bytes, xty_bytes, eg_bytes;
};

DenseTrainLayout dense_layout(int b, int v, int E, int D, int steps) {
    DenseTrainLayout L{};
    const size_t rows = (size_t)b * v, nd = rows * steps * D * sizeof(float);
    const int N = (int)(rows * steps);
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += al256(bytes); return at; };
    L.saved_bytes = ggnn_dense_train_saved_bytes(b, v, D, steps);
    L.saved = take(L.saved_bytes);
    L.out = take(rows * D * sizeof(float));
    L.dpc = take(nd); L.dpg = take(2 * nd); L.dx = take(nd); L.dM = take((size_t)E * nd);
    const size_t x1 = ggnn_xty_workspace_bytes(N, 2 * D, D, 1), x2 = ggnn_xty_workspace_bytes(N, 2 * D, 2 * D, 1);
    L.xty_bytes = x1 > x2 ? x1 : x2;
    L.xty = take(L.xty_bytes);
    L.eg_bytes = ggnn_dense_edge_grad_workspace_bytes(N, E, D);
    L.eg = take(L.eg_bytes);
    L.total = p + 256;
    return L;
}

int check_shape(int b, int v, int E, int D, int steps) {
    GGNN_CHECK_ARG(b >= 0 && steps >= 1 && (long long)b * v * steps < (1LL << 31) / 8, "bad sizes b=%d v=%d steps=%d", b, v, steps);
    if (!ggnn_dense_train_supported(v, E, D))
        return fail(GGNN_E_UNSUPPORTED, "native dense training step: split matrix path, v <= 32, E in {2,4,6,8}, hidden size 32/64/100 "
                                        "(got v=%d E=%d D=%d)", v, E, D);
    return GGNN_OK;
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" size_t ggnn_dense_train_workspace_bytes(int b, int v, int E, int D, int steps) {
    if (b < 0 || v <= 0 || E <= 0 || D <= 0 || steps <= 0) return 0;
    return dense_layout(b, v, E, D, steps).total;
}

extern "C" int ggnn_dense_train_forward_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                                            const float* edge_bias, const float* bg, const float* bc, int b, int v, int E, int D,
                                            int steps, int fmt, void* ws, size_t ws_bytes, int64_t* final_off, ggnn_stream_t stream) {
    if (int rc = check_shape(b, v, E, D, steps)) return rc;
    if (b == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && A && edge_packed && gru_packed && bg && bc && ws && final_off, "null pointer");
    GGNN_CHECK_ARG((reinterpret_cast<size_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
    const DenseTrainLayout L = dense_layout(b, v, E, D, steps);
    if (ws_bytes < L.total) return fail(GGNN_E_WORKSPACE, "dense training workspace too small: %zu < %zu", ws_bytes, L.total);
    char* base = static_cast<char*>(ws);
    if (int rc = ggnn_dense_propagate_save_f32(h0, A, edge_packed, gru_packed, edge_bias, bg, bc, reinterpret_cast<float*>(base + L.out),
                                               b, v, E, D, steps, fmt, reinterpret_cast<float*>(base + L.saved), L.saved_bytes, stream))
        return rc;
    *final_off = (int64_t)L.out;
    return GGNN_OK;
}

extern "C" int ggnn_dense_train_backward_f32(const float* d_final, const float* A, const float* nin, const float* bwd_packed, int b,
                                             int v, int E, int D, int steps, float* g_W, float* g_b, float* g_Wg, float* g_bg,
                                             float* g_Wc, float* g_bc, void* ws, size_t ws_bytes, ggnn_stream_t stream,
                                             ggnn_stream_t side_stream) {
    if (int rc = check_shape(b, v, E, D, steps)) return rc;
    if (b == 0) return GGNN_OK;
    GGNN_CHECK_ARG(d_final && A && bwd_packed && ws, "null pointer");
    GGNN_CHECK_ARG(g_W && g_Wg && g_bg && g_Wc && g_bc, "gradient buffers missing");
    GGNN_CHECK_ARG((nin != nullptr) == (g_b != nullptr), "the in-degrees and the edge biases' gradient buffer come together (both or neither)");
    GGNN_CHECK_ARG((reinterpret_cast<size_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
    const DenseTrainLayout L = dense_layout(b, v, E, D, steps);
    if (ws_bytes < L.total) return fail(GGNN_E_WORKSPACE, "dense training workspace too small: %zu < %zu", ws_bytes, L.total);
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)stream, side = side_stream ? (hipStream_t)side_stream : (hipStream_t)stream;
    auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    const int rows = b * v, N = rows * steps;
    const size_t nd = (size_t)N * D;                                     // floats of one saved tensor
    const float* saved = f(L.saved);
    const float *h = saved, *x = saved + nd, *rh = saved + 5 * nd;       // saved[0], [1], [5] stacked over the timesteps: [N, D]
    float *dpc = f(L.dpc), *dpg = f(L.dpg), *dx = f(L.dx), *dM = f(L.dM);

    if (int rc = ggnn_dense_propagate_bwd_f32(d_final, A, bwd_packed, saved, b, v, E, D, steps, nullptr, dpc, dpg, dx, dM, stream)) return rc;

    // ---- the GRU's four variables, side stream: the products of backward.DensePropagateFn with the same arguments ----------------
    if (int rc = stream_order_after(side, st)) return rc;
    {
        int32_t row_off[2] = {0, N};
        int32_t ldx[2] = {D, D};
        const float* X[2] = {x, rh};
        if (int rc = ggnn_xty_acc_f32(X, 2, D, ldx, nullptr, dpc, D, g_Wc, g_bc, 1, 2 * D, D, 1, row_off, 1, base + L.xty, L.xty_bytes,
                                      (ggnn_stream_t)side)) return rc;
        X[1] = h;
        if (int rc = ggnn_xty_acc_f32(X, 2, D, ldx, nullptr, dpg, 2 * D, g_Wg, g_bg, 1, 2 * D, 2 * D, 1, row_off, 1, base + L.xty, L.xty_bytes,
                                      (ggnn_stream_t)side)) return rc;
    }
    // ---- edge weights and edge biases, main stream ---------------------------------------------------------------------------------
    if (int rc = ggnn_dense_edge_grad_f32(h, dM, nin, dx, N, rows, E, D, g_W, g_b, 1, base + L.eg, L.eg_bytes, stream)) return rc;
    return stream_order_after(st, side);          // the caller's next launches (optimizer, next forward) see every product
}
