// The layer / timestep driver of chem_tensorflow_sparse.py:131-218 in native code: ONE C-ABI call enqueues the
// whole forward propagation (all layers x timesteps: message transform -> gather/segment-sum -> GRU) on the
// stream.  The Python host layer would otherwise make ~3 ctypes calls and ~5 tensor allocations per timestep
// (24 + 40 per 8-step forward, ~1.2 ms of host time against ~1.6 ms of GPU time: the loop was close to
// host-bound on slow hosts).  No allocation, no sync: scratch comes from the caller.
//
// Per timestep it launches either 3 kernels (transform, gather/segment-sum, GRU) or -- with `fuse_gather`, packed
// GRU weights, a fused hidden size and no edge bias -- 2 kernels (transform, GRU with the segment sum gathered
// inside: ggnn_gru_packed_gather_f32).  With propagation attention (:147-149, 170-196; ggnn_sparse_propagate_attn_f32) the
// segment sum is ggnn_gather_segment_sum_attn_compact_f32 over the compacted rows: always 3 kernels.  Both entry points run the
// one driver below; without attention it launches what it always launched.
//
// The cell is a parameter of the driver: with an RnnCell (ggnn_sparse_propagate_rnn_f32; graph_rnn_cell = RNN, the R-GCN
// configuration) the node update is the BasicRNNCell -- ggnn_rnn_packed_gather_f32 (2 kernels per timestep; at hidden 128 / 192 / 256
// ggnn_rnn_panel_gather_f32 on panel images) for a layer with packed
// images, a supported (D, nx) and no edge bias, ggnn_gather_segment_sum_f32 + ggnn_rnn_f32 (3 kernels) otherwise -- always behind
// the compacted transform.  Without one the GRU entry points launch exactly what they launched before.
//
// With a CudnnCell (ggnn_sparse_propagate_cudnn_f32; graph_rnn_cell = CudnnCompatibleGRUCell, :105-108) the node update is that cell,
// always behind the compacted transform and ggnn_gather_segment_sum_f32 over the compact rows (edge bias included):
// ggnn_cudnn_gru_packed_f32 (one launch) for a layer with packed images and a supported (D, nx), ggnn_cudnn_gru_f32 (three) otherwise.
#include "ggnn_common.h"
#include <cstring>

namespace ggnn {
// ggnn_msg_compact.hip: ggnn_msg_transform_compact_f32 that also leaves 0 in *zero (may be NULL) -- stored by the transform launch itself
int msg_transform_compact_zero(const float* h, const float* W, const int32_t* pair_node, const int64_t* type_row_off, float* Hc,
                               void* ws, size_t ws_bytes, int V, int D, int T, int fmt, int32_t* zero, ggnn_stream_t stream);
}

static constexpr int kTileCounters = 1024;     // timesteps per call that get a dynamic tile counter (the rest split statically)

extern "C" size_t ggnn_sparse_propagate_workspace_bytes(int V, int D, int T, int64_t compact_rows) {
    if (V < 0 || D <= 0 || T <= 0) return 0;
    const size_t vd = (size_t)V * D * sizeof(float);
    const size_t hrows = compact_rows >= 0 ? (size_t)(compact_rows > 0 ? compact_rows : 1) * D * sizeof(float)
                                           : (size_t)V * T * D * sizeof(float);
    // transformed states + incoming + two ping-pong states + GRU scratch (un-fused sizes) + tile counters of the
    // fused GRU launches (one int32 per timestep) + 256-B alignment slack
    return hrows + 3 * vd + ggnn_gru_workspace_bytes(V, D) + kTileCounters * sizeof(int32_t) + 6 * 256;
}

static inline char* bump(char*& p, size_t bytes) {
    char* r = p;
    p += (bytes + 255) / 256 * 256;
    return r;
}

// the BasicRNNCell's per-layer weights (HOST arrays of num_layers DEVICE pointers) and the length of gather_row
struct RnnCell {
    const float* const* w;
    const float* const* b;
    const float* const* packed;
    int64_t M;
};

// the CudnnCompatibleGRUCell's per-layer weights (HOST arrays of num_layers DEVICE pointers); packed: ggnn_cudnn_gru_pack_weights_f32
struct CudnnCell {
    const float* const* wg;
    const float* const* bg;
    const float* const* wcx;
    const float* const* bcx;
    const float* const* wch;
    const float* const* bch;
    const float* const* packed;
};

extern "C" size_t ggnn_sparse_propagate_cudnn_workspace_bytes(int V, int D, int T, int64_t compact_rows) {
    const size_t base = ggnn_sparse_propagate_workspace_bytes(V, D, T, compact_rows);
    return base ? base + ggnn_cudnn_gru_workspace_bytes(V, D) + 256 : 0;
}

static int propagate(
        const RnnCell* rnn, const CudnnCell* cud, const float* h0, int V, int D, int T,
        const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node, const int64_t* type_row_off,
        const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
        const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
        const float* const* gru_packed, const int32_t* gru_fmt, const int32_t* edge_fmt, int act, int fuse_gather,
        float* const* layer_out, void* ws, size_t ws_bytes, const int32_t* slot_pair, const float* const* attn_factors,
        ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && D % 4 == 0 && T > 0, "bad sizes V=%d D=%d T=%d", V, D, T);
    GGNN_CHECK_ARG(num_layers > 0 && layer_timesteps && res_ptr && layer_out, "bad layer description");
    GGNN_CHECK_ARG(edge_w || edge_packed, "edge weights missing");
    if (rnn) GGNN_CHECK_ARG(rnn->b && (rnn->packed || rnn->w) && rnn->M >= 0, "RNN weights missing");
    else if (cud) GGNN_CHECK_ARG(cud->bg && cud->bcx && cud->bch && (cud->packed || (cud->wg && cud->wcx && cud->wch)), "Cudnn GRU weights missing");
    else GGNN_CHECK_ARG(bg && bc && (gru_packed || (Wg && Wc)), "GRU weights missing");
    const bool compact = pair_node != nullptr && type_row_off != nullptr;
    GGNN_CHECK_ARG(!rnn || compact, "the RNN cell runs on the compacted transform only (pair_node, type_row_off)");
    GGNN_CHECK_ARG(!cud || compact, "the CudnnCompatibleGRUCell runs on the compacted transform only (pair_node, type_row_off)");
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h0 && row_ptr && ws, "null pointer");
    GGNN_CHECK_ARG(!attn_factors || compact, "propagation attention needs the compacted transform (pair_node, type_row_off)");
    const int64_t rows = compact ? type_row_off[T] : -1;
    const size_t ws_need = cud ? ggnn_sparse_propagate_cudnn_workspace_bytes(V, D, T, rows) : ggnn_sparse_propagate_workspace_bytes(V, D, T, rows);
    if (ws_bytes < ws_need)
        return ggnn::fail(GGNN_E_WORKSPACE, "propagate workspace too small: %zu < %zu", ws_bytes, ws_need);
    const size_t vd = (size_t)V * D * sizeof(float);
    char* p = reinterpret_cast<char*>((reinterpret_cast<size_t>(ws) + 255) / 256 * 256);
    float* H = reinterpret_cast<float*>(bump(p, compact ? (size_t)(rows > 0 ? rows : 1) * D * sizeof(float)
                                                       : (size_t)V * T * D * sizeof(float)));
    float* incoming = reinterpret_cast<float*>(bump(p, vd));
    float* ping[2] = {reinterpret_cast<float*>(bump(p, vd)), nullptr};
    ping[1] = reinterpret_cast<float*>(bump(p, vd));
    int32_t* counters = reinterpret_cast<int32_t*>(bump(p, kTileCounters * sizeof(int32_t)));
    void* gru_ws = p;
    const size_t gru_ws_bytes = ggnn_gru_workspace_bytes(V, D);
    p += (gru_ws_bytes + 255) / 256 * 256;
    void* cud_ws = p;                              // (CudnnCell only: the composed cell's r*h | u | r | hc)
    const size_t cud_ws_bytes = ggnn_cudnn_gru_workspace_bytes(V, D);
    int step_no = 0;
    // The counters are zero before their GRU launches.  The compacted transform of a timestep precedes that timestep's GRU on the
    // stream and zeroes its counter itself (ggnn::msg_transform_compact_zero: one thread's store, no fill launch in front of the
    // forward); the routes with another transform kernel (dense, column panels) or none (no rows) fill them all here.
    const bool zero_in_transform = compact && rows > 0 && ggnn_gru_is_fused(D) == 1;
    if (!zero_in_transform) {
        int total_steps = 0;
        for (int l = 0; l < num_layers; ++l) total_steps += layer_timesteps[l] > 0 ? layer_timesteps[l] : 0;
        if (total_steps > kTileCounters) total_steps = kTileCounters;
        if (total_steps > 0) GGNN_CHECK_HIP(hipMemsetAsync(counters, 0, (size_t)total_steps * sizeof(int32_t), (hipStream_t)stream));
    }

    const float* states[64];                       // node_states_per_layer (:118-119, :152)
    GGNN_CHECK_ARG(num_layers < 63, "too many layers");
    states[0] = h0;
    for (int l = 0; l < num_layers; ++l) {
        const int nres = res_ptr[l + 1] - res_ptr[l];
        // any number of residual inputs in the reference (:139-145); here up to 6 (the generic GEMM's 8 K segments = 6 + messages
        // + h); the fused single-launch GRU kernels take 2, layers with more run the two-launch generic GRU
        GGNN_CHECK_ARG(nres >= 0 && nres <= 6, "layer %d has %d residual inputs (max 6)", l, nres);
        const float* xs[7];
        for (int i = 0; i < nres; ++i) {
            const int src = res_idx[res_ptr[l] + i];
            GGNN_CHECK_ARG(src >= 0 && src <= l, "layer %d: residual index %d refers to a later layer", l, src);
            xs[i] = states[src];                   // :140-145
        }
        xs[nres] = incoming;                       // :211-212 residual states first, aggregated messages last
        const int nx = nres + 1;
        GGNN_CHECK_ARG(layer_out[l], "layer_out[%d] is null", l);
        const float* cur = states[l];              // :152
        const int steps = layer_timesteps[l];
        const float* bias_l = edge_bias ? edge_bias[l] : nullptr;
        const bool packed_gru = !rnn && !cud && gru_packed && gru_packed[l] && ggnn_gru_is_fused(D) && nx <= 3;
        const int fmt_l = gru_fmt ? gru_fmt[l] : GGNN_GRU_FMT_BF16X3;      // the format gru_packed[l] was packed in
        // fuse_gather = the largest number of concatenated GRU inputs (residuals + messages) for which the segment sum
        // is gathered inside the GRU kernel; 0 = never.
        const float* factors_l = attn_factors ? attn_factors[l] : nullptr;
        GGNN_CHECK_ARG(!attn_factors || factors_l, "attn_factors[%d] is null", l);
        const bool gather_in_gru = !rnn && !cud && !attn_factors && fuse_gather > 0 && nx <= fuse_gather && packed_gru && ggnn_gru_is_fused(D) == 1 && bias_l == nullptr &&
                                   (unsigned long long)V * T * D < (1ULL << 30);      // (its 32-bit byte offsets)
        // (the two supported sets are disjoint: rnn->packed[l] holds the images of whichever cell takes (D, nx))
        const bool panel_rnn = rnn && ggnn_rnn_panel_supported(D, nx);
        const bool gather_in_rnn = rnn && fuse_gather > 0 && nx <= fuse_gather && rnn->packed && rnn->packed[l] &&
                                   (panel_rnn || ggnn_rnn_fused_supported(D, nx)) && bias_l == nullptr &&
                                   (unsigned long long)V * D < (1ULL << 30) && (unsigned long long)(rows > 0 ? rows : 1) * D < (1ULL << 30);
        if (rnn) GGNN_CHECK_ARG(rnn->b[l] && (gather_in_rnn || (rnn->w && rnn->w[l])), "layer %d needs raw RNN weights (no fused cell for it)", l);
        const bool packed_cud = cud && cud->packed && cud->packed[l] && ggnn_cudnn_gru_fused_supported(D, nx) &&
                                (unsigned long long)V * D < (1ULL << 30);
        if (cud) GGNN_CHECK_ARG(cud->bg[l] && cud->bcx[l] && cud->bch[l] &&
                                (packed_cud || (cud->wg && cud->wcx && cud->wch && cud->wg[l] && cud->wcx[l] && cud->wch[l])),
                                "layer %d needs raw Cudnn GRU weights (no fused cell for it)", l);
        for (int s = 0; s < steps; ++s) {          // :153
            int rc;
            static const bool dyn_tiles = [] { const char* e = getenv("GGNN_DYN_TILES"); return !e || atoi(e) != 0; }();
            int32_t* counter = (dyn_tiles && step_no < kTileCounters) ? counters + step_no : nullptr;
            ++step_no;
            if (compact) {
                const bool packed = edge_packed && edge_packed[l];
                rc = ggnn::msg_transform_compact_zero(cur, packed ? nullptr : edge_w[l], pair_node, type_row_off, H,
                                                      packed ? const_cast<float*>(edge_packed[l]) : gru_ws,
                                                      packed ? ggnn_msg_transform_compact_workspace_bytes(D, T) : gru_ws_bytes,
                                                      V, D, T, (packed && edge_fmt) ? edge_fmt[l] : GGNN_GRU_FMT_BF16X3,
                                                      zero_in_transform ? counter : nullptr, stream);
            } else {
                GGNN_CHECK_ARG(edge_w && edge_w[l], "dense transform needs raw edge weights");
                rc = ggnn_msg_transform_f32(cur, D, edge_w[l], H, V, D, T, stream);
            }
            if (rc) return rc;
            float* out = (s + 1 == steps) ? layer_out[l] : ping[s & 1];
            if (gather_in_rnn && panel_rnn) {
                rc = ggnn_rnn_panel_gather_f32(xs, nx, cur, rnn->packed[l], rnn->b[l], out, H, rows > 0 ? rows : 1, row_ptr, gather_row,
                                               rnn->M, nin, T, use_avg, nullptr, V, D, act, stream);
            } else if (gather_in_rnn) {
                rc = ggnn_rnn_packed_gather_f32(xs, nx, cur, rnn->packed[l], rnn->b[l], out, H, rows > 0 ? rows : 1, row_ptr, gather_row,
                                                rnn->M, nin, T, use_avg, nullptr, V, D, act, stream);
            } else if (rnn) {
                rc = ggnn_gather_segment_sum_f32(H, row_ptr, gather_row, nin, bias_l, use_avg, incoming, V, D, T, stream);
                if (rc) return rc;
                rc = ggnn_rnn_f32(xs, nx, cur, rnn->w[l], rnn->b[l], out, V, D, act, stream);
            } else if (cud) {
                rc = ggnn_gather_segment_sum_f32(H, row_ptr, gather_row, nin, bias_l, use_avg, incoming, V, D, T, stream);
                if (rc) return rc;
                if (packed_cud)
                    rc = ggnn_cudnn_gru_packed_f32(xs, nx, cur, cud->packed[l], cud->bg[l], cud->bcx[l], cud->bch[l], out, nullptr,
                                                   nullptr, nullptr, nullptr, V, D, stream);
                else
                    rc = ggnn_cudnn_gru_f32(xs, nx, cur, cud->wg[l], cud->bg[l], cud->wcx[l], cud->bcx[l], cud->wch[l], cud->bch[l], out,
                                            cud_ws, cud_ws_bytes, V, D, stream);
            } else if (gather_in_gru) {
                rc = ggnn_gru_packed_gather_f32(xs, nx, cur, gru_packed[l], bg[l], bc[l], out, H, row_ptr, gather_row, nin, T,
                                                use_avg, V, D, act, fmt_l, counter, stream);
            } else {
                rc = factors_l ? ggnn_gather_segment_sum_attn_compact_f32(H, cur, row_ptr, slot_pair, gather_row, factors_l, nin, bias_l,
                                                                          use_avg, incoming, V, D, T, stream)
                               : ggnn_gather_segment_sum_f32(H, row_ptr, gather_row, nin, bias_l, use_avg, incoming, V, D, T, stream);
                if (rc) return rc;
                if (packed_gru)
                    rc = ggnn_gru_packed_f32(xs, nx, cur, gru_packed[l], bg[l], bc[l], out, nullptr, nullptr, nullptr, V, D, act,
                                             fmt_l, counter, stream);
                else {
                    GGNN_CHECK_ARG(Wg && Wc && Wg[l] && Wc[l], "layer %d needs raw GRU weights (no packed images for it)", l);
                    rc = ggnn_gru_f32(xs, nx, cur, Wg[l], bg[l], Wc[l], bc[l], out, gru_ws, gru_ws_bytes, nullptr, nullptr,
                                      nullptr, V, D, act, stream);
                }
            }
            if (rc) return rc;
            cur = out;
        }
        if (steps == 0) {                          // a layer without timesteps forwards its input state
            GGNN_CHECK_HIP(hipMemcpyAsync(layer_out[l], cur, vd, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        }
        states[l + 1] = layer_out[l];
    }
    return GGNN_OK;
}

extern "C" int ggnn_sparse_propagate_f32(
        const float* h0, int V, int D, int T,
        const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node, const int64_t* type_row_off,
        const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
        const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
        const float* const* gru_packed, const int32_t* gru_fmt, const int32_t* edge_fmt, int act, int fuse_gather,
        float* const* layer_out, void* ws, size_t ws_bytes, ggnn_stream_t stream) {
    return propagate(nullptr, nullptr, h0, V, D, T, row_ptr, gather_row, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                     res_idx, edge_w, edge_packed, edge_bias, Wg, bg, Wc, bc, gru_packed, gru_fmt, edge_fmt, act, fuse_gather,
                     layer_out, ws, ws_bytes, nullptr, nullptr, stream);
}

extern "C" int ggnn_sparse_propagate_attn_f32(
        const float* h0, int V, int D, int T,
        const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node, const int64_t* type_row_off,
        const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
        const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
        const float* const* gru_packed, const int32_t* gru_fmt, const int32_t* edge_fmt, int act, int fuse_gather,
        float* const* layer_out, void* ws, size_t ws_bytes, const int32_t* slot_pair, const float* const* attn_factors,
        ggnn_stream_t stream) {
    GGNN_CHECK_ARG(attn_factors, "attn_factors is null");
    if (D > 256) return ggnn::fail(GGNN_E_UNSUPPORTED, "propagation attention supports hidden sizes up to 256 (got %d)", D);
    return propagate(nullptr, nullptr, h0, V, D, T, row_ptr, gather_row, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                     res_idx, edge_w, edge_packed, edge_bias, Wg, bg, Wc, bc, gru_packed, gru_fmt, edge_fmt, act, fuse_gather,
                     layer_out, ws, ws_bytes, slot_pair, attn_factors, stream);
}

extern "C" int ggnn_sparse_propagate_rnn_f32(
        const float* h0, int V, int D, int T,
        const int32_t* row_ptr, const int32_t* gather_row, int64_t M, const int32_t* pair_node, const int64_t* type_row_off,
        const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
        const float* const* rnn_w, const float* const* rnn_b, const float* const* rnn_packed,
        const int32_t* edge_fmt, int act, int fuse_gather, float* const* layer_out, void* ws, size_t ws_bytes,
        ggnn_stream_t stream) {
    GGNN_CHECK_ARG(pair_node && type_row_off, "the RNN cell runs on the compacted transform only (pair_node, type_row_off)");
    GGNN_CHECK_ARG(act == GGNN_ACT_TANH || act == GGNN_ACT_RELU, "unknown activation %d", act);
    const RnnCell cell{rnn_w, rnn_b, rnn_packed, M};
    return propagate(&cell, nullptr, h0, V, D, T, row_ptr, gather_row, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                     res_idx, edge_w, edge_packed, edge_bias, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, edge_fmt, act,
                     fuse_gather, layer_out, ws, ws_bytes, nullptr, nullptr, stream);
}

extern "C" int ggnn_sparse_propagate_cudnn_f32(
        const float* h0, int V, int D, int T,
        const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node, const int64_t* type_row_off,
        const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
        const float* const* wg, const float* const* bg, const float* const* wcx, const float* const* bcx,
        const float* const* wch, const float* const* bch, const float* const* cell_packed,
        const int32_t* edge_fmt, float* const* layer_out, void* ws, size_t ws_bytes, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(pair_node && type_row_off, "the CudnnCompatibleGRUCell runs on the compacted transform only (pair_node, type_row_off)");
    const CudnnCell cell{wg, bg, wcx, bcx, wch, bch, cell_packed};
    return propagate(nullptr, &cell, h0, V, D, T, row_ptr, gather_row, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps,
                     res_ptr, res_idx, edge_w, edge_packed, edge_bias, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, edge_fmt,
                     GGNN_ACT_TANH, 0, layer_out, ws, ws_bytes, nullptr, nullptr, stream);
}
