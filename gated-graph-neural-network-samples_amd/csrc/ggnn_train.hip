// The optimisation step of the default sparse model (chem_tensorflow.py:183-191 over chem_tensorflow_sparse.py:117-218) as native
// launch sequences: ggnn_sparse_train_forward_f32 enqueues the whole training forward (compacted message transform + fused GRU
// with the segment sum gathered inside, r / u / c / incoming and every timestep's state kept), ggnn_sparse_train_backward_f32 the
// whole backward pass (fused GRU backward, transpose segment sums, compacted transform on W^T, every weight-gradient product on
// a side stream, accumulated straight into the optimizer's gradient buffers).  Between the two the host runs the readout + loss
// (ggnn_readout_loss_{fwd,bwd}_f32) and, under data parallelism, the all-reduce of the mask counts.
//
// Why: the same sequence driven from Python through torch.autograd is ~250 ctypes calls, tensor allocations and autograd nodes per
// step -- 4.4 ms of host time for ~6 ms of GPU time, and with a producer thread packing the next batch (which needs the interpreter
// lock) fresh-batch epochs ran at 6.9-7.3 ms per step instead of 6.1.  Here a step is two calls; nothing is allocated (one
// caller-provided workspace, laid out by train_layout below), nothing synchronises.
//
// With propagation attention (:147-149, 170-196) on the compacted route (params['compact_attention'] == 'native') the same two
// sequences run as ggnn_sparse_attn_train_forward_f32 / ggnn_sparse_attn_train_backward_f32: the segment sum is
// ggnn_gather_segment_sum_attn_compact_f32 in front of ggnn_gru_packed_f32 (three launches per timestep instead of two), and in
// the backward the unweighted transpose gather into dHc gives way to: the compact rows recomputed, ggnn_attn_bwd_target_compact_f32
// (softmax backward per target: coef_a / coef_s / dfac per message, target-side dh), ggnn_range_sum_f32 of dfac added to the layer's
// attention-factor gradient, and ggnn_attn_bwd_source_compact_f32 (dHc and the source-side dh in one pass).  Everything else --
// layout, layer plan, merged products, the node sum deferred into the next GRU backward -- is shared: the drivers below take the
// attention arguments as an optional struct and launch what they always launched without it.
//
// At the column-panel hidden sizes (128 / 192 / 256) the default model runs the same two sequences as
// ggnn_sparse_train_panel_forward_f32 / ggnn_sparse_train_panel_backward_f32 -- a second ROUTE through the drivers below (TrainRoute),
// not a copy of them.  There is no gather-fused forward GRU at these sizes, so a timestep is what the attention form already
// launches: transform, a stand-alone segment sum (ggnn_gather_segment_sum_f32 into that timestep's `incoming`), ggnn_gru_packed_f32
// saving r / u / c in the layer's operand format.  The backward's GRU launches are the panel kernel's (ggnn_gru_bwd_panel.hip); its
// weight-gradient products are too wide for ggnn_xty_acc_f32 (dpg has 2D = up to 512 columns), so on the side stream they run per X
// segment on the row-split kernel's accumulate form (ggnn_gemm_tn_acc_f32 straight into the caller's gradient views, the bias
// gradients as column sums added to theirs; timestep by timestep unless GGNN_TRAIN_MERGE_PRODUCTS is set: merge_products below),
// and the row-gathered edge-weight product goes through 128-column views of h and dHc whose blocks one small launch adds into the
// [T, D, D] destination.  The images come from ggnn_sparse_train_panel_prepare_f32 (ggnn_train_panel.hip).
//
// With the BasicRNNCell (graph_rnn_cell = RNN, :109-110) on the compacted route (params['compact_rnn'] == 'native') the same two
// sequences run as ggnn_sparse_rnn_train_forward_f32 / ggnn_sparse_rnn_train_backward_f32: the drivers take the cell as an optional
// struct (RnnForward / RnnBackward) and launch what they always launched without it.  A timestep of the forward is the compacted
// transform + ggnn_rnn_packed_gather_f32 keeping `incoming`; of the backward ggnn_rnn_bwd_fused_f32 (its gather form when a node sum
// is pending) and ONE weight-gradient product, dW += [x.. | incoming | h]^T dP with the bias gradient, where the GRU has two.  The
// layout drops r / u / c / r*h / dpg; dpc holds dP.  The images come per layer from the single-kind packers (no one-launch prepare).
//
// Cross-stream hazards: everything a side-stream product reads (dpc, dpg, r*h, incoming, states, dHc) has its own buffer per
// timestep, so the main stream never waits for the side stream inside a step; the call ends with the main stream waiting for the
// side stream's last product, which orders the next step's forward (it reuses the workspace) behind them.
#include "ggnn_split.hpp"
#include "ggnn_philox.hpp"
#include <mutex>

namespace ggnn {
namespace {

constexpr int kMaxLayers = 62;
constexpr int kMaxNx = 3;

constexpr int kEdgeBlock = 128;        // columns of each operand the row-gathered ggnn_xty_acc_f32 takes

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// Which kernels the two sequences run on.  panel == false: the whole-block sizes (32 / 64 / 100), the launches they always made.
// panel == true: the column-panel sizes (128 / 192 / 256), see the header comment.
struct TrainRoute {
    bool panel;
    bool takes(int D) const {
        return panel ? (D == 128 || D == 192 || D == 256) && ggnn_gru_is_fused(D) == 2 && ggnn_gru_bwd_is_fused(D) && ggnn_msg_transform_compact_supported(D)
                     : ggnn_gru_is_fused(D) == 1 && ggnn_gru_bwd_is_fused(D) && ggnn_msg_transform_compact_supported(D);
    }
};

struct TrainLayout {
    size_t Hc, state, r, u, c, inc, counters;           // forward
    size_t dpc, rh, dh, dpg, dx, dHc, Z, xty;            // backward
    size_t coef, md;                                     // attention: coef_a | coef_s | dfac, md bytes each (one set: main stream only)
    size_t tn, eblk, colsum, bsum;                       // panel route, side stream only: gemm_tn partials, edge-gradient blocks, column sums
    size_t tn_bytes, colsum_bytes, xty_bytes;
    size_t vd, rd, total;
    int steps;
};

// M > 0: the layout of the attention sequences (M messages); M == 0: the default model's, unchanged; panel: the default model's at the
// column-panel sizes (everything the side stream's products need beyond the per-timestep buffers follows them); rnn: the BasicRNNCell's
// -- no r / u / c / r*h / dpg, and dpc holds dP = dL/d(pre-activation), the one dY of the cell's weight-gradient product
TrainLayout train_layout(int V, int D, int T, int64_t R, int steps, int64_t M = 0, bool panel = false, bool rnn = false) {
    TrainLayout L{};
    L.steps = steps;
    // per-timestep buffers follow each other WITHOUT padding (V*D*4 is a multiple of 16): the buffers of consecutive timesteps then
    // form one [S*V, D] matrix, which lets the weight-gradient products of a layer's timesteps run as ONE product over S*V rows
    L.vd = (size_t)V * D * sizeof(float);
    L.rd = al256((size_t)(R > 0 ? R : 1) * D * sizeof(float));
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += al256(bytes); return at; };
    L.Hc = take(L.rd);
    L.state = take(L.vd * (steps + 1));                  // slot 0: a copy of h0; slot k+1: the state after timestep k
    const size_t gates = rnn ? 0 : L.vd * steps;         // (a buffer of 0 bytes takes no room)
    L.r = take(gates); L.u = take(gates); L.c = take(gates);
    L.inc = take(L.vd * steps);
    L.counters = take((size_t)steps * sizeof(int32_t));
    L.dpc = take(L.vd * steps); L.rh = take(gates); L.dh = take(L.vd * steps); L.dpg = take(2 * gates);
    L.dx = take(L.vd * steps * kMaxNx);
    L.dHc = take(L.rd * steps); L.Z = take(L.rd);
    L.md = al256((size_t)M * sizeof(float));
    if (M > 0) L.coef = take(3 * L.md);
    if (panel) {
        // one set each: the side stream runs its products in order.  The widest row-split product is [S*V, D]^T [S*V, 2D]
        L.tn_bytes = ggnn_gemm_tn_workspace_bytes(V * (steps > 1 ? steps : 1), D, 2 * D);
        L.tn = take(L.tn_bytes);
        L.eblk = take((size_t)T * D * D * sizeof(float));
        L.colsum_bytes = ggnn_colsum_workspace_bytes(2 * D);
        L.colsum = take(L.colsum_bytes);
        L.bsum = take((size_t)2 * D * sizeof(float));
        L.xty_bytes = ggnn_xty_workspace_bytes(V > R ? V : (int)R, kEdgeBlock, kEdgeBlock, T);
    } else {
        L.xty_bytes = ggnn_xty_workspace_bytes((V > R ? V : (int)R) * (steps > 1 ? steps : 1), 4 * D, rnn ? D : 2 * D, T);
    }
    L.xty = take(L.xty_bytes);
    L.total = p + 256;
    (void)T;
    return L;
}

// events that order the side stream behind the main stream's producers (created once per device; recording an event that an
// earlier hipStreamWaitEvent already captured is fine: a wait refers to the record that preceded it)
struct EventPool {
    hipEvent_t ev[64];
    int next = 0;
    bool ready = false;
};
std::mutex g_pool_mutex;
EventPool g_pools[16];

int next_event(hipEvent_t* out) {
    int dev = 0;
    GGNN_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    EventPool& p = g_pools[dev & 15];
    if (!p.ready) {
        for (int i = 0; i < 64; ++i) GGNN_CHECK_HIP(hipEventCreateWithFlags(&p.ev[i], hipEventDisableTiming));
        p.ready = true;
    }
    *out = p.ev[p.next];
    p.next = (p.next + 1) & 63;
    return GGNN_OK;
}

int order_after(hipStream_t waiter, hipStream_t producer) {
    if (waiter == producer) return GGNN_OK;
    hipEvent_t e;
    if (int rc = next_event(&e)) return rc;
    GGNN_CHECK_HIP(hipEventRecord(e, producer));
    GGNN_CHECK_HIP(hipStreamWaitEvent(waiter, e, 0));
    return GGNN_OK;
}

__global__ void add_inplace_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 a = reinterpret_cast<f32x4*>(dst)[i];
    const f32x4 b = reinterpret_cast<const f32x4*>(src)[i];
    a += b;
    reinterpret_cast<f32x4*>(dst)[i] = a;
}

int add_inplace(float* dst, const float* src, long long n, hipStream_t st) {
    const long long n4 = n / 4;
    if (n4 == 0) return GGNN_OK;
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, dst, src, n4);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

// dst[t][k][n] += blocks of the panel route's edge-weight gradient: block (bk, bn) holds [T][kw][nw] (kw = min(128, D - 128 bk), nw
// likewise) and the blocks follow each other in (bk, bn) order -- what ggnn_xty_acc_f32 wrote for the 128-column views of h and dHc
__global__ void add_edge_blocks_kernel(float* __restrict__ dst, const float* __restrict__ blk, int T, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * D * D) return;
    const int n = i % D, k = (i / D) % D, t = i / (D * D);
    const int bk = k / kEdgeBlock, bn = n / kEdgeBlock;
    const int kw = min(kEdgeBlock, D - bk * kEdgeBlock), nw = min(kEdgeBlock, D - bn * kEdgeBlock);
    // floats in front of block (bk, bn): whole block rows (T * 128 * D each), then the blocks to its left in its row (T * kw * 128 each)
    const size_t off = (size_t)T * kEdgeBlock * D * bk + (size_t)T * kw * kEdgeBlock * bn;
    dst[i] += blk[off + ((size_t)t * kw + (k - bk * kEdgeBlock)) * nw + (n - bn * kEdgeBlock)];
}

// ---- a step's weight images in ONE launch ------------------------------------------------------------------------------------------
// Every optimisation step changes every weight, so every step rebuilds every stage image: per layer the T edge-weight images and
// the T images of their transposes (both of the weight-dropout-MASKED weights, the mask applied on the fly: ggnn_philox.hpp), the
// 3(nx+1) images of the fused GRU and the 3(nx+1) of its backward -- ~120 images of 48 KiB for the default model.  Driven layer by
// layer from the host that was 30 launches of 4 us each at the head of the step (mask, transpose copy, four pack kernels per layer).
constexpr int kPrepMaxLayers = 16;
struct PrepArgs {
    const float* edge_w[kPrepMaxLayers]; const float* Wg[kPrepMaxLayers]; const float* Wc[kPrepMaxLayers];
    float* edge_img[kPrepMaxLayers]; float* edge_img_t[kPrepMaxLayers]; float* gru_img[kPrepMaxLayers]; float* gru_bwd_img[kPrepMaxLayers];
    unsigned long long seed[kPrepMaxLayers];
    int nx[kPrepMaxLayers];
    int gru_fmt[kPrepMaxLayers];       // operand format of layer l's GRU FORWARD images (kSplitF16x2 / kSplitBf16x3)
    int T; float keep;
};

// SF: every image in split form (ggnn_split.hpp).  The GRU FORWARD's images of layer l are in the operand format a.gru_fmt[l] (the
// caller's per-layer choice, see include/ggnn_hip.h "Operand formats"); the edge-weight images -- whose transposes multiply
// gradients of any magnitude -- and the GRU backward's are always in the exact bf16 x 3 format.
template <int D, bool SF>
__global__ __launch_bounds__(256) void train_prepare_kernel(PrepArgs a) {
    using C = StageCfg<D>;
    const int l = blockIdx.z, i = blockIdx.y;
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    const int T = a.T, ng = 3 * (a.nx[l] + 1);
    if (i < 2 * T) {
        // edge-weight image of type t (i < T), or of its transpose (the backward's Z = dHc W_t^T); masked like ggnn_dropout_f32 masks
        // the [T*D, D] variable: row key = t*D + (row of W_t), column = column of W_t
        const bool tr = i >= T;
        const int t = tr ? i - T : i;
        const float* W = a.edge_w[l] + (size_t)t * D * D;
        const float keep = a.keep;
        const unsigned long long seed = a.seed[l];
        auto value = [&](int k, int n) -> float {                         // image[k][n] = W_t[k][n], or W_t[n][k]
            if (n >= D) return 0.f;
            const int r = tr ? n : k, c = tr ? k : n;
            float v = W[(size_t)r * D + c];
            if (keep < 1.0f) v = dropout_apply(v, keep, seed, (unsigned long long)(t * D + r), c);
            return v;
        };
        float* img = (tr ? a.edge_img_t[l] : a.edge_img[l]) + (size_t)t * ImgCfg<D, SF>::IMG;
        if constexpr (SF) {
            pack_split_image<D>(value, img, first, stride);
        } else {
            for (int j = first; j < C::IMG; j += stride) {
                float v = 0.f;
                if (j < C::MAIN) {
                    const int e = j & 3, n = (j >> 2) % C::BN, k = 4 * ((j >> 2) / C::BN) + e;
                    v = value(k, n);
                } else if (j < C::MAIN + C::REM) {
                    const int jj = j - C::MAIN;
                    v = value(16 * C::NC + jj / C::BN, jj % C::BN);
                }
                img[j] = v;
            }
        }
    } else if (i < 2 * T + ng) {
        const int ci = i - 2 * T;
        if constexpr (SF) {
            if (a.gru_fmt[l] == kSplitF16x2)         // (block-uniform)
                gru_fwd_image_pack_split<D, kSplitF16x2>(a.Wg[l], a.Wc[l], a.nx[l], ci, a.gru_img[l] + (size_t)ci * ImgCfg<D, true, kSplitF16x2>::IMG, first, stride);
            else
                gru_fwd_image_pack_split<D, kSplitBf16x3>(a.Wg[l], a.Wc[l], a.nx[l], ci, a.gru_img[l] + (size_t)ci * ImgCfg<D, true>::IMG, first, stride);
        } else gru_fwd_image_pack<D>(a.Wg[l], a.Wc[l], a.nx[l], ci, a.gru_img[l] + (size_t)ci * ImgCfg<D, false>::IMG, first, stride);
    } else if (i < 2 * T + 2 * ng) {
        const int bi = i - 2 * T - ng;
        float* img = a.gru_bwd_img[l] + (size_t)bi * ImgCfg<D, SF>::IMG;
        if constexpr (SF) gru_bwd_image_pack_split<D>(a.Wg[l], a.Wc[l], a.nx[l], bi, img, first, stride);
        else gru_bwd_image_pack<D>(a.Wg[l], a.Wc[l], a.nx[l], bi, img, first, stride);
    }
}

// GGNN_TRAIN_MERGE_PRODUCTS=0: the GRU weight-gradient products timestep by timestep also for layers without residual inputs.
// The panel route merges only when the variable is SET (and not 0): timestep by timestep its row-split products are the autograd
// step's own, in the same order -- the gradients of the two steps then differ by the order of the layer-input sums only -- while
// one product over S*V rows splits the rows differently.  Measured at h = 192, two merged timesteps: gradients 2.7e-7 of the
// largest entry apart, which Adam's first steps (d update / d g <= lr / (eps / sqrt(1 - beta2)) = 3162) turn into weights 2.2e-5
// apart after three steps, beyond the 2e-5 the step is held to against the autograd step.
bool merge_products(bool panel) {
    static const int v = [] { const char* e = getenv("GGNN_TRAIN_MERGE_PRODUCTS"); return !e ? -1 : (atoi(e) != 0 ? 1 : 0); }();
    return panel ? v == 1 : v != 0;
}

// what the attention form of the two sequences needs beyond the default model's arguments
struct AttnForward {
    const int32_t* slot_pair;              // by-target slot -> src*T + type (gather_row_c is then the slot -> compact row table)
    const float* const* factors;           // per layer: edge_type_attention_weights [T]
    int64_t M;
};
struct AttnBackward {
    const int32_t *row_ptr, *slot_pair, *slot_row, *msg_perm;        // the by-target index of the forward
    const int64_t* msg_type_off;                                     // host [T+1]: message ids of type t (dfac is by message id)
    const int32_t *src_node_ptr, *src_dst, *src_msg, *src_row;       // by-(source, type) slots: ggnn_attn_bwd_source_compact_f32
    const float* const* edge_packed;                                 // forward images: the compact rows are recomputed
    const float* const* factors;
    float* const* g_attn;                                            // per layer: gradient view of the attention factors [T]
    int64_t M;
};

// the BasicRNNCell form (graph_rnn_cell = RNN on the compacted route, params['compact_rnn'] == 'native'): the cell's arguments in
// place of the GRU's.  A timestep of the forward is the compacted transform + ggnn_rnn_packed_gather_f32 (save_incoming), of the
// backward ggnn_rnn_bwd_fused[_gather]_f32 + ONE weight-gradient product dW += [x.. | incoming | h]^T dP with the bias gradient.
struct RnnForward {
    const float* const* packed;            // per layer: ggnn_rnn_pack_weights_f32's images
    const float* const* b;                 // per layer: bias [D]
    int64_t M;                             // messages: the length of gather_row_c
};
struct RnnBackward {
    const float* const* bwd_packed;        // per layer: ggnn_rnn_bwd_pack_weights_f32's images
    float* const* g_W;                     // per layer: gradient views of W [(nx+1)D, D] and b [D]
    float* const* g_b;
};

struct LayerPlan { int first_step, steps, nres; int res[kMaxNx]; };

// every layer of the plan is one the fused RNN cell takes (checked before anything is enqueued)
int rnn_layers_supported(int D, int num_layers, const LayerPlan* plan) {
    if (!ggnn_msg_transform_compact_supported(D))
        return fail(GGNN_E_UNSUPPORTED, "native training step, RNN cell: hidden size %d has no compacted transform", D);
    for (int l = 0; l < num_layers; ++l)
        if (!ggnn_rnn_fused_supported(D, plan[l].nres + 1))
            return fail(GGNN_E_UNSUPPORTED, "native training step, RNN cell: layer %d (D=%d, nx=%d) is outside ggnn_rnn_fused_supported", l, D,
                        plan[l].nres + 1);
    return GGNN_OK;
}

int plan_layers(int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx, LayerPlan* plan,
                int* total_steps) {
    GGNN_CHECK_ARG(num_layers > 0 && num_layers <= kMaxLayers && layer_timesteps && res_ptr, "bad layer description");
    int steps = 0;
    for (int l = 0; l < num_layers; ++l) {
        LayerPlan& P = plan[l];
        P.first_step = steps; P.steps = layer_timesteps[l];
        GGNN_CHECK_ARG(P.steps >= 1, "layer %d has %d timesteps: the native training step needs at least one per layer", l, P.steps);
        P.nres = res_ptr[l + 1] - res_ptr[l];
        GGNN_CHECK_ARG(P.nres >= 0 && P.nres + 1 <= kMaxNx, "layer %d has %d residual inputs (the fused kernels take %d)", l, P.nres, kMaxNx - 1);
        for (int i = 0; i < P.nres; ++i) {
            P.res[i] = res_idx[res_ptr[l] + i];
            GGNN_CHECK_ARG(P.res[i] >= 0 && P.res[i] <= l, "layer %d: residual index %d refers to a later layer", l, P.res[i]);
        }
        steps += P.steps;
    }
    *total_steps = steps;
    return GGNN_OK;
}

}  // namespace

// the same event pool for the other native launch sequences (ggnn_dense_train.hip)
int stream_order_after(hipStream_t waiter, hipStream_t producer) { return order_after(waiter, producer); }

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_sparse_train_prepare_f32(int num_layers, int T, int D, const int32_t* nx, const float* const* edge_w, float keep_prob,
                                             const uint64_t* seeds, const float* const* Wg, const float* const* Wc,
                                             const int32_t* gru_fmt, float* const* edge_packed, float* const* edge_packed_t,
                                             float* const* gru_packed, float* const* gru_bwd_packed, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(num_layers > 0 && num_layers <= kPrepMaxLayers, "num_layers %d outside 1..%d", num_layers, kPrepMaxLayers);
    GGNN_CHECK_ARG(T > 0 && T <= 64 && nx && edge_w && Wg && Wc && edge_packed && edge_packed_t && gru_packed && gru_bwd_packed, "bad arguments");
    GGNN_CHECK_ARG(keep_prob > 0.0f && keep_prob <= 1.0f && (keep_prob >= 1.0f || seeds), "keep_prob %g outside (0, 1] or seeds missing", (double)keep_prob);
    if (ggnn_gru_is_fused(D) != 1 || !ggnn_gru_bwd_is_fused(D) || !ggnn_msg_transform_compact_supported(D))
        return fail(GGNN_E_UNSUPPORTED, "no whole-block stage images for hidden size %d", D);
    PrepArgs a{};
    a.T = T; a.keep = keep_prob;
    int max_images = 0;
    for (int l = 0; l < num_layers; ++l) {
        GGNN_CHECK_ARG(nx[l] >= 1 && nx[l] <= kMaxNx, "layer %d: nx %d outside 1..%d", l, nx[l], kMaxNx);
        GGNN_CHECK_ARG(edge_w[l] && Wg[l] && Wc[l] && edge_packed[l] && edge_packed_t[l] && gru_packed[l] && gru_bwd_packed[l], "layer %d: null pointer", l);
        a.edge_w[l] = edge_w[l]; a.Wg[l] = Wg[l]; a.Wc[l] = Wc[l];
        a.edge_img[l] = edge_packed[l]; a.edge_img_t[l] = edge_packed_t[l]; a.gru_img[l] = gru_packed[l]; a.gru_bwd_img[l] = gru_bwd_packed[l];
        a.seed[l] = seeds ? seeds[l] : 0ULL; a.nx[l] = nx[l];
        a.gru_fmt[l] = gru_launch_fmt(gru_fmt ? gru_fmt[l] : kSplitBf16x3);
        const int images = 2 * T + 6 * (nx[l] + 1);
        if (images > max_images) max_images = images;
    }
    const dim3 grid(8, max_images, num_layers);
    hipStream_t st = (hipStream_t)stream;
    const bool sf = split_matrix_path();
#define GGNN_PREP(DD) if (sf) hipLaunchKernelGGL((train_prepare_kernel<DD, true>), grid, dim3(256), 0, st, a); \
                      else hipLaunchKernelGGL((train_prepare_kernel<DD, false>), grid, dim3(256), 0, st, a);
    switch (D) {
        case 100: GGNN_PREP(100) break;
        case 64: GGNN_PREP(64) break;
        default: GGNN_PREP(32) break;
    }
#undef GGNN_PREP
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

extern "C" size_t ggnn_sparse_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps) {
    if (V < 0 || D <= 0 || T <= 0 || total_steps <= 0) return 0;
    return train_layout(V, D, T, compact_rows, total_steps).total;
}

extern "C" size_t ggnn_sparse_attn_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps, int64_t M) {
    if (V < 0 || D <= 0 || T <= 0 || total_steps <= 0 || compact_rows < 0 || M <= 0 || M >= (1LL << 31)) return 0;
    return train_layout(V, D, T, compact_rows, total_steps, M).total;
}

static int train_forward(
        const float* h0, int V, int D, int T, const int32_t* row_ptr, const int32_t* gather_row_c, const int32_t* pair_node,
        const int64_t* type_row_off, const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
        const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed, const float* const* bg,
        const float* const* bc, const float* const* gru_packed, const int32_t* gru_fmt, int act, void* ws, size_t ws_bytes,
        int64_t* final_state_offset, const AttnForward* at, const RnnForward* rn, const TrainRoute& route, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V > 0 && D > 0 && D % 4 == 0 && T > 0, "bad sizes V=%d D=%d T=%d", V, D, T);
    GGNN_CHECK_ARG(h0 && row_ptr && gather_row_c && pair_node && type_row_off && ws && final_state_offset, "null pointer");
    GGNN_CHECK_ARG(edge_packed && (rn ? (rn->packed && rn->b && !at && !route.panel) : (bg && bc && gru_packed)), "weights missing");
    GGNN_CHECK_ARG((reinterpret_cast<size_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
    if (route.panel) {
        if (!route.takes(D)) return fail(GGNN_E_UNSUPPORTED, "native training step, panel route: hidden size %d is not 128 / 192 / 256", D);
        GGNN_CHECK_ARG(!at, "the panel route has no attention form");
        GGNN_CHECK_ARG(!use_avg || nin, "nin is required for mean aggregation");
    } else if (!rn && (ggnn_gru_is_fused(D) != 1 || !ggnn_msg_transform_compact_supported(D)))
        return fail(GGNN_E_UNSUPPORTED, "native training step: hidden size %d has no gather-fused GRU / compacted transform", D);
    LayerPlan plan[kMaxLayers];
    int steps = 0;
    if (int rc = plan_layers(num_layers, layer_timesteps, res_ptr, res_idx, plan, &steps)) return rc;
    if (rn) { if (int rc = rnn_layers_supported(D, num_layers, plan)) return rc; }
    const int64_t R = type_row_off[T];
    GGNN_CHECK_ARG(R > 0, "no messages in the batch");
    GGNN_CHECK_ARG(!rn || ((!use_avg || nin) && rn->M > 0 && rn->M < (1LL << 31)), "RNN cell: nin missing for mean aggregation, or bad message count");
    GGNN_CHECK_ARG(!at || (at->slot_pair && at->factors && at->M > 0 && at->M < (1LL << 31) && (!use_avg || nin)), "attention arguments missing");
    if (route.panel) {            // (the limits of the launches below, checked before anything is enqueued)
        GGNN_CHECK_ARG(T <= 64 && R < (1LL << 31), "bad sizes T=%d, %lld compact rows", T, (long long)R);
        if ((unsigned long long)V * 2 * D >= (1ULL << 30) || (unsigned long long)R * D >= (1ULL << 30) || (long long)V * steps >= (1LL << 31))
            return fail(GGNN_E_UNSUPPORTED, "native training step, panel route: V*2D and rows*D must be < 2^30 (V=%d, D=%d, rows=%lld)", V, D, (long long)R);
    }
    const TrainLayout L = train_layout(V, D, T, R, steps, at ? at->M : 0, route.panel, rn != nullptr);
    if (ws_bytes < L.total) return fail(GGNN_E_WORKSPACE, "training workspace too small: %zu < %zu", ws_bytes, L.total);
    if (rn) {
        if ((unsigned long long)V * D >= (1ULL << 30) || (unsigned long long)R * D >= (1ULL << 30))
            return fail(GGNN_E_UNSUPPORTED, "native training step, RNN cell: V*D and rows*D must be < 2^30 (V=%d, D=%d, rows=%lld)", V, D, (long long)R);
        for (int l = 0; l < num_layers; ++l) GGNN_CHECK_ARG(edge_packed[l] && rn->packed[l] && rn->b[l], "layer %d: weights missing", l);
    }
    char* base = static_cast<char*>(ws);
    float* Hc = reinterpret_cast<float*>(base + L.Hc);
    int32_t* counters = reinterpret_cast<int32_t*>(base + L.counters);
    hipStream_t st = (hipStream_t)stream;
    if (!rn) GGNN_CHECK_HIP(hipMemsetAsync(counters, 0, (size_t)steps * sizeof(int32_t), st));     // (the GRU's tile counters)
    auto buf = [&](size_t off, int step) { return reinterpret_cast<float*>(base + off + (size_t)step * L.vd); };
    const float* states[kMaxLayers + 1];
    states[0] = h0;
    // (the backward's merged products read the input state of every timestep from the state array: slot 0 holds h0)
    GGNN_CHECK_HIP(hipMemcpyAsync(buf(L.state, 0), h0, L.vd, hipMemcpyDeviceToDevice, st));
    const size_t edge_img_bytes = ggnn_msg_transform_compact_workspace_bytes(D, T);
    for (int l = 0; l < num_layers; ++l) {
        const LayerPlan& P = plan[l];
        const float* xs[kMaxNx];
        for (int i = 0; i < P.nres; ++i) xs[i] = states[P.res[i]];              // :140-145
        const int nx = P.nres + 1;
        const float* cur = states[l];                                           // :152
        GGNN_CHECK_ARG(rn || (edge_packed[l] && bg[l] && bc[l] && gru_packed[l]), "layer %d: weights missing", l);
        GGNN_CHECK_ARG(!at || at->factors[l], "layer %d: attention factors missing", l);
        for (int s = 0; s < P.steps; ++s) {                                     // :153
            const int k = P.first_step + s;
            if (int rc = ggnn_msg_transform_compact_f32(cur, nullptr, pair_node, type_row_off, Hc, const_cast<float*>(edge_packed[l]),
                                                        edge_img_bytes, V, D, T, GGNN_GRU_FMT_BF16X3, stream)) return rc;
            float* out = buf(L.state, k + 1);
            if (rn) {
                // :198-216 with the BasicRNNCell: the segment sum gathered inside the cell, `incoming` kept for dW -- the launch
                // of the autograd route's training forward (variants.compact_rnn_forward)
                if (int rc = ggnn_rnn_packed_gather_f32(xs, nx, cur, rn->packed[l], rn->b[l], out, Hc, R, row_ptr, gather_row_c, rn->M,
                                                        use_avg ? nin : nullptr, T, use_avg ? 1 : 0, buf(L.inc, k), V, D, act, stream)) return rc;
            } else if (at) {
                // :170-196 the attention-weighted sum into this timestep's `incoming`, then the GRU on it (every product exact:
                // the two-piece f16 range proof does not cover attention-weighted sums)
                if (int rc = ggnn_gather_segment_sum_attn_compact_f32(Hc, cur, row_ptr, at->slot_pair, gather_row_c, at->factors[l], nin,
                                                                      nullptr, use_avg ? 1 : 0, buf(L.inc, k), V, D, T, stream)) return rc;
                xs[nx - 1] = buf(L.inc, k);
                if (int rc = ggnn_gru_packed_f32(xs, nx, cur, gru_packed[l], bg[l], bc[l], out, buf(L.r, k), buf(L.u, k), buf(L.c, k), V, D,
                                                 act, GGNN_GRU_FMT_BF16X3, counters + k, stream)) return rc;
            } else if (route.panel) {
                // :160-168, 206-209 the stand-alone segment sum (with the mean epilogue) into this timestep's `incoming`, then the panel
                // GRU on it in the layer's operand format
                if (int rc = ggnn_gather_segment_sum_f32(Hc, row_ptr, gather_row_c, use_avg ? nin : nullptr, nullptr, use_avg ? 1 : 0,
                                                         buf(L.inc, k), V, D, T, stream)) return rc;
                xs[nx - 1] = buf(L.inc, k);
                if (int rc = ggnn_gru_packed_f32(xs, nx, cur, gru_packed[l], bg[l], bc[l], out, buf(L.r, k), buf(L.u, k), buf(L.c, k), V, D,
                                                 act, gru_fmt ? gru_fmt[l] : GGNN_GRU_FMT_BF16X3, nullptr, stream)) return rc;
            } else if (int rc = ggnn_gru_packed_gather_train_f32(xs, nx, cur, gru_packed[l], bg[l], bc[l], out, Hc, row_ptr, gather_row_c,
                                                          use_avg ? nin : nullptr, T, use_avg ? 1 : 0, buf(L.r, k), buf(L.u, k),
                                                          buf(L.c, k), buf(L.inc, k), V, D, act,
                                                          gru_fmt ? gru_fmt[l] : GGNN_GRU_FMT_BF16X3, counters + k, stream)) return rc;
            cur = out;
        }
        states[l + 1] = cur;
    }
    *final_state_offset = (int64_t)(reinterpret_cast<const char*>(states[num_layers]) - base);
    return GGNN_OK;
}

static int train_backward(
        const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const int32_t* rows_rp, const int32_t* rows_gather, const int32_t* rows_heads,
        const int32_t* node_rp, const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
        const float* const* edge_packed_t, const float* const* gru_bwd_packed, int act,
        float* const* g_edge, float* const* g_Wg, float* const* g_bg, float* const* g_Wc, float* const* g_bc,
        float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes, const AttnBackward* at, const RnnBackward* rn,
        const TrainRoute& route, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    GGNN_CHECK_ARG(V > 0 && D > 0 && D % 4 == 0 && T > 0 && T <= 64, "bad sizes V=%d D=%d T=%d", V, D, T);
    GGNN_CHECK_ARG(h0 && pair_node && type_row_off && (at || (rows_rp && rows_gather)) && node_rp && node_order && identity_rows && d_final && ws,
                   "null pointer");
    GGNN_CHECK_ARG(!at || (at->row_ptr && at->slot_pair && at->slot_row && at->msg_perm && at->msg_type_off && at->src_node_ptr && at->src_dst &&
                           at->src_msg && at->src_row && at->edge_packed && at->factors && at->g_attn && at->M > 0 && at->M < (1LL << 31)),
                   "attention arguments missing");
    GGNN_CHECK_ARG(edge_packed_t && g_edge && d_state_ws && (rn ? (rn->bwd_packed && rn->g_W && rn->g_b && !at && !route.panel)
                                                                 : (gru_bwd_packed && g_Wg && g_bg && g_Wc && g_bc)),
                   "weights / gradient buffers missing");
    GGNN_CHECK_ARG(!use_avg || nin, "nin is required for mean aggregation");
    GGNN_CHECK_ARG((reinterpret_cast<size_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
    if (!rn && !route.takes(D))
        return fail(GGNN_E_UNSUPPORTED, route.panel ? "native training step, panel route: hidden size %d is not 128 / 192 / 256"
                                                    : "native training step: no whole-block fused GRU backward for hidden size %d", D);
    GGNN_CHECK_ARG(!route.panel || !at, "the panel route has no attention form");
    LayerPlan plan[kMaxLayers];
    int steps = 0;
    if (int rc = plan_layers(num_layers, layer_timesteps, res_ptr, res_idx, plan, &steps)) return rc;
    if (rn) { if (int rc = rnn_layers_supported(D, num_layers, plan)) return rc; }
    const int64_t R64 = type_row_off[T];
    GGNN_CHECK_ARG(R64 > 0 && R64 < (1LL << 31), "bad compact row count");
    const int R = (int)R64;
    if (route.panel) {            // (the limits of the launches below, checked before anything is enqueued)
        if ((unsigned long long)V * 2 * D >= (1ULL << 30) || (unsigned long long)R * D >= (1ULL << 30) || (long long)V * steps >= (1LL << 31))
            return fail(GGNN_E_UNSUPPORTED, "native training step, panel route: V*2D and rows*D must be < 2^30 (V=%d, D=%d, rows=%d)", V, D, R);
    }
    const TrainLayout L = train_layout(V, D, T, R, steps, at ? at->M : 0, route.panel, rn != nullptr);
    if (ws_bytes < L.total) return fail(GGNN_E_WORKSPACE, "training workspace too small: %zu < %zu", ws_bytes, L.total);
    if (rn) {                     // (the limits of the cell's launches, checked before anything is enqueued)
        if ((unsigned long long)V * D >= (1ULL << 30) || (unsigned long long)R * D >= (1ULL << 30))
            return fail(GGNN_E_UNSUPPORTED, "native training step, RNN cell: V*D and rows*D must be < 2^30 (V=%d, D=%d, rows=%d)", V, D, R);
        for (int l = 0; l < num_layers; ++l)
            GGNN_CHECK_ARG(edge_packed_t[l] && rn->bwd_packed[l] && g_edge[l] && rn->g_W[l] && rn->g_b[l], "layer %d: pointers missing", l);
    }
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)stream, side = side_stream ? (hipStream_t)side_stream : (hipStream_t)stream;
    auto buf = [&](size_t off, int step) { return reinterpret_cast<float*>(base + off + (size_t)step * L.vd); };
    float* Z = reinterpret_cast<float*>(base + L.Z);
    void* xty_ws = base + L.xty;
    const size_t xty_ws_bytes = L.xty_bytes;
    const size_t edge_img_bytes = ggnn_msg_transform_compact_workspace_bytes(D, T);
    const long long nvd = (long long)V * D;
    int32_t row_off_v[2] = {0, V};
    int32_t row_off_t[65];
    for (int t = 0; t <= T; ++t) row_off_t[t] = (int32_t)type_row_off[t];

    // forward states by layer (the forward pass's buffers) and the gradients flowing into them
    const float* states[kMaxLayers + 1];
    states[0] = buf(L.state, 0);                          // (the forward's copy of h0)
    for (int l = 0; l < num_layers; ++l) states[l + 1] = buf(L.state, plan[l].first_step + plan[l].steps);
    (void)h0;
    float* dstate[kMaxLayers + 1];
    bool has[kMaxLayers + 1];
    for (int l = 0; l < num_layers; ++l) { dstate[l] = d_state_ws[l]; has[l] = false; GGNN_CHECK_ARG(dstate[l], "d_state_ws[%d] is null", l); }
    dstate[num_layers] = d_final; has[num_layers] = true;

    // the first side-stream product of the step is ordered behind everything queued on the main stream so far (the zeroed gradients)
    if (int rc = order_after(side, st)) return rc;

    // The per-node sum that closes a timestep's transform backward (dh[v] += sum_t Z[row(v,t)]) is taken by its CONSUMER: the fused
    // GRU backward of the timestep processed next reads g[v] + the rows of Z its node's slot-head record names
    // (ggnn_gru_bwd_fused_gather_f32) -- one launch and one pass over [V,D] less per timestep.  Needs the head records and at most
    // four rows per node (T <= 4: a node has one compact row per edge type it sends on); GGNN_TRAIN_FUSE_NODE_SUM=0: stand-alone sums.
    static const bool fuse_env = [] { const char* e = getenv("GGNN_TRAIN_FUSE_NODE_SUM"); return !e || atoi(e) != 0; }();
    const bool fuse_node_sum = fuse_env && node_heads != nullptr && T <= 4;
    bool z_pending = false;                         // Z holds rows that the next GRU backward still has to add to its g

    for (int l = num_layers - 1; l >= 0; --l) {
        const LayerPlan& P = plan[l];
        const int nx = P.nres + 1;
        GGNN_CHECK_ARG(has[l + 1], "no gradient reaches the output of layer %d", l);
        GGNN_CHECK_ARG(rn || (edge_packed_t[l] && gru_bwd_packed[l] && g_edge[l] && g_Wg[l] && g_bg[l] && g_Wc[l] && g_bc[l]), "layer %d: pointers missing", l);
        GGNN_CHECK_ARG(!at || (at->edge_packed[l] && at->factors[l] && at->g_attn[l]), "layer %d: attention pointers missing", l);
        const float* g = dstate[l + 1];
        for (int s = P.steps - 1; s >= 0; --s) {
            const int k = P.first_step + s;
            const float* h_in = buf(L.state, k);              // input state of timestep k (slot k; slot 0 = h0)
            // where this timestep's gradients go: straight into an empty accumulator, else into a temporary that is added afterwards
            float* dh_dst = buf(L.dh, k);
            bool dh_direct = false;
            if (s == 0 && !has[l]) { dh_dst = dstate[l]; dh_direct = true; }
            float* dxp[kMaxNx];
            bool dx_direct[kMaxNx];
            for (int i = 0; i < P.nres; ++i) {
                const int src = P.res[i];
                dx_direct[i] = !has[src] && !(s == 0 && src == l && dh_direct);
                // (two residual inputs of one layer may name the same state: only the first of them can write it directly)
                for (int j = 0; j < i; ++j) if (P.res[j] == src) dx_direct[i] = false;
                dxp[i] = dx_direct[i] ? dstate[src] : reinterpret_cast<float*>(base + L.dx + ((size_t)k * kMaxNx + i) * L.vd);
            }
            float* dinc = reinterpret_cast<float*>(base + L.dx + ((size_t)k * kMaxNx + (nx - 1)) * L.vd);
            dxp[nx - 1] = dinc;
            float* dpc = buf(L.dpc, k); float* rh = buf(L.rh, k);
            float* dpg = reinterpret_cast<float*>(base + L.dpg + (size_t)k * 2 * L.vd);
            if (rn) {
                // the whole BasicRNNCell backward of the timestep in one launch; dpc holds dP.  A pending node sum is taken on load
                if (z_pending) {
                    if (int rc = ggnn_rnn_bwd_fused_gather_f32(g, Z, node_heads, R, buf(L.state, k + 1), rn->bwd_packed[l], dpc, dxp, dh_dst,
                                                               nin, T, use_avg ? 1 : 0, nx, V, D, act, stream)) return rc;
                    z_pending = false;
                } else {
                    if (int rc = ggnn_rnn_bwd_fused_f32(g, buf(L.state, k + 1), rn->bwd_packed[l], dpc, dxp, dh_dst, nin, T, use_avg ? 1 : 0,
                                                        nx, V, D, act, stream)) return rc;
                }
            } else if (z_pending) {
                if (int rc = ggnn_gru_bwd_fused_gather_f32(g, Z, node_heads, h_in, buf(L.r, k), buf(L.u, k), buf(L.c, k),
                                                           const_cast<float*>(gru_bwd_packed[l]), dpc, dpg, rh, dh_dst, dxp, nin, T,
                                                           use_avg ? 1 : 0, nx, V, D, act, stream)) return rc;
                z_pending = false;
            } else {
                if (int rc = ggnn_gru_bwd_fused_f32(g, h_in, buf(L.r, k), buf(L.u, k), buf(L.c, k), nullptr, nullptr,
                                                    const_cast<float*>(gru_bwd_packed[l]), dpc, dpg, rh, dh_dst, dxp, nin, T, use_avg ? 1 : 0,
                                                    nx, V, D, act, stream)) return rc;
            }
            for (int i = 0; i < P.nres; ++i) if (dx_direct[i]) has[P.res[i]] = true;
            if (dh_direct) has[l] = true;

            // ---- GRU weight gradients, side stream: dWc += [x.. | incoming | r*h]^T dpc, dWg += [x.. | incoming | h]^T dpg
            // (RNN cell: the one product dW += [x.. | incoming | h]^T dP, the bias gradient from its ones row)
            // A layer WITHOUT residual inputs runs them once for all its timesteps: incoming, r*h, dpc, dpg and the input states of
            // consecutive timesteps are consecutive [V,D] ([V,2D]) buffers, i.e. one matrix of S*V rows each -- one product
            // instead of S, and its fixed part (prologue, partial store, reduction launch: ~20 us of ~100) paid once.
            const bool merged = P.nres == 0 && P.steps > 1 && merge_products(route.panel);
            if (route.panel) {
                // per X segment on the row-split kernel's accumulate form, straight into the segment's rows of the gradient views;
                // the bias gradients as column sums added to theirs
                if (!merged || s == 0) {
                    if (int rc = order_after(side, st)) return rc;
                    const int k0 = merged ? P.first_step : k;
                    const int rows = merged ? V * P.steps : V;
                    const float* X[kMaxNx + 1];
                    for (int i = 0; i < P.nres; ++i) X[i] = states[P.res[i]];          // (merged: none)
                    X[nx - 1] = buf(L.inc, k0);
                    const float* dpc0 = buf(L.dpc, k0);
                    const float* dpg0 = reinterpret_cast<const float*>(base + L.dpg + (size_t)k0 * 2 * L.vd);
                    void* tn_ws = base + L.tn;
                    float* bsum = reinterpret_cast<float*>(base + L.bsum);
                    X[nx] = buf(L.rh, k0);
                    for (int i = 0; i <= nx; ++i)
                        if (int rc = ggnn_gemm_tn_acc_f32(X[i], D, dpc0, D, g_Wc[l] + (size_t)i * D * D, D, 1, rows, D, D, tn_ws, L.tn_bytes, side)) return rc;
                    if (int rc = ggnn_colsum_f32(dpc0, D, rows, D, bsum, base + L.colsum, L.colsum_bytes, side)) return rc;
                    if (int rc = add_inplace(g_bc[l], bsum, D, side)) return rc;
                    X[nx] = buf(L.state, k0);
                    for (int i = 0; i <= nx; ++i)
                        if (int rc = ggnn_gemm_tn_acc_f32(X[i], D, dpg0, 2 * D, g_Wg[l] + (size_t)i * D * 2 * D, 2 * D, 1, rows, D, 2 * D, tn_ws, L.tn_bytes, side)) return rc;
                    if (int rc = ggnn_colsum_f32(dpg0, 2 * D, rows, 2 * D, bsum, base + L.colsum, L.colsum_bytes, side)) return rc;
                    if (int rc = add_inplace(g_bg[l], bsum, 2 * D, side)) return rc;
                }
            } else if (merged) {
                if (s == 0) {                               // (the layer's first timestep is the last one processed)
                    if (int rc = order_after(side, st)) return rc;
                    const int k0 = P.first_step;
                    int32_t row_off_m[2] = {0, V * P.steps};
                    const float* X[2] = {buf(L.inc, k0), rn ? buf(L.state, k0) : buf(L.rh, k0)}; int32_t ldx[2] = {D, D};
                    if (int rc = ggnn_xty_acc_f32(X, 2, D, ldx, nullptr, buf(L.dpc, k0), D, rn ? rn->g_W[l] : g_Wc[l], rn ? rn->g_b[l] : g_bc[l], 1,
                                                  2 * D, D, 1, row_off_m, 1, xty_ws, xty_ws_bytes, side)) return rc;
                    X[1] = buf(L.state, k0);
                    if (!rn) {                              // (the RNN cell has the one product)
                        if (int rc = ggnn_xty_acc_f32(X, 2, D, ldx, nullptr, reinterpret_cast<float*>(base + L.dpg + (size_t)k0 * 2 * L.vd), 2 * D,
                                                      g_Wg[l], g_bg[l], 1, 2 * D, 2 * D, 1, row_off_m, 1, xty_ws, xty_ws_bytes, side)) return rc;
                    }
                }
            } else {
                if (int rc = order_after(side, st)) return rc;
                const float* X[4]; int32_t ldx[4];
                for (int i = 0; i < P.nres; ++i) { X[i] = states[P.res[i]]; ldx[i] = D; }
                X[nx - 1] = buf(L.inc, k); ldx[nx - 1] = D;
                X[nx] = rn ? h_in : rh; ldx[nx] = D;
                if (int rc = ggnn_xty_acc_f32(X, nx + 1, D, ldx, nullptr, dpc, D, rn ? rn->g_W[l] : g_Wc[l], rn ? rn->g_b[l] : g_bc[l], 1,
                                              (nx + 1) * D, D, 1, row_off_v, 1, xty_ws, xty_ws_bytes, side)) return rc;
                X[nx] = h_in;
                if (!rn) {
                    if (int rc = ggnn_xty_acc_f32(X, nx + 1, D, ldx, nullptr, dpg, 2 * D, g_Wg[l], g_bg[l], 1, (nx + 1) * D, 2 * D, 1, row_off_v, 1,
                                                  xty_ws, xty_ws_bytes, side)) return rc;
                }
            }

            // ---- back through the segment sum and the compacted transform (main stream)
            float* dHc = reinterpret_cast<float*>(base + L.dHc + (size_t)k * L.rd);
            // The gradient of the step's INPUT state: not needed for the very first timestep (h0 is data: nothing upstream of it is
            // trained, and nobody reads d_state_ws[0]) -- its transform and node sum are not run at all.
            const bool first_step = l == 0 && s == 0;
            if (at) {
                // :170-196 under autodiff.  The compact rows are recomputed (one transform launch; saving them per step would cost
                // steps * R * D floats of workspace and as many bytes written in the forward as are read back here), then the
                // softmax backward per target node and both transpose gathers of the source side in one launch.
                float* Hc = reinterpret_cast<float*>(base + L.Hc);
                float* coef_a = reinterpret_cast<float*>(base + L.coef);
                float* coef_s = reinterpret_cast<float*>(base + L.coef + L.md);
                float* dfac = reinterpret_cast<float*>(base + L.coef + 2 * L.md);
                if (int rc = ggnn_msg_transform_compact_f32(h_in, nullptr, pair_node, type_row_off, Hc, const_cast<float*>(at->edge_packed[l]),
                                                            edge_img_bytes, V, D, T, GGNN_GRU_FMT_BF16X3, stream)) return rc;
                if (int rc = ggnn_attn_bwd_target_compact_f32(Hc, h_in, dinc, at->row_ptr, at->slot_pair, at->slot_row, at->msg_perm,
                                                              at->factors[l], coef_a, coef_s, dfac, dh_dst, 1, V, D, T, stream)) return rc;
                if (int rc = range_sum(dfac, at->msg_type_off, T, at->g_attn[l], 1, st)) return rc;
                if (int rc = ggnn_attn_bwd_source_compact_f32(dinc, h_in, at->src_node_ptr, at->src_dst, at->src_msg, at->src_row, coef_a,
                                                              coef_s, dHc, first_step ? nullptr : dh_dst, V, D, stream)) return rc;
            } else if (rows_heads) {
                if (int rc = ggnn_gather_segment_sum_heads_f32(dinc, rows_rp, rows_gather, rows_heads, nullptr, nullptr, 0, dHc, R, D, 1, 0, stream)) return rc;
            } else {
                if (int rc = ggnn_gather_segment_sum_f32(dinc, rows_rp, rows_gather, nullptr, nullptr, 0, dHc, R, D, 1, stream)) return rc;
            }
            if (!first_step) {
                if (int rc = ggnn_msg_transform_compact_f32(dHc, nullptr, identity_rows, type_row_off, Z, const_cast<float*>(edge_packed_t[l]),
                                                            edge_img_bytes, R, D, T, GGNN_GRU_FMT_BF16X3, stream)) return rc;
                if (fuse_node_sum) {
                    z_pending = true;                   // (the next timestep's GRU backward adds the rows while it loads g)
                } else if (node_heads) {
                    if (int rc = ggnn_gather_segment_sum_heads_f32(Z, node_rp, node_order, node_heads, nullptr, nullptr, 0, dh_dst, V, D, 1, 1, stream)) return rc;
                } else {
                    if (int rc = ggnn_gather_segment_sum_acc_f32(Z, node_rp, node_order, dh_dst, V, D, stream)) return rc;
                }
            }
            // ---- edge-weight gradients, side stream (needs dHc: ordered behind the transform launch above, which also read it)
            if (int rc = order_after(side, st)) return rc;
            if (D <= kEdgeBlock) {
                const float* X[1] = {h_in}; int32_t ldx[1] = {D};
                if (int rc = ggnn_xty_acc_f32(X, 1, D, ldx, pair_node, dHc, D, g_edge[l], nullptr, 1, D, D, 0, row_off_t, T, xty_ws, xty_ws_bytes,
                                              side)) return rc;
            } else {
                // (panel route, D = 192 / 256) the row-gathered kernel takes <= 128 columns of each operand: 128-column views of h
                // (pointer offset, ldx = D) and of dHc, the blocks into the workspace, one launch adds them into [T, D, D]
                float* blk = reinterpret_cast<float*>(base + L.eblk);
                float* out = blk;
                int32_t ldx[1] = {D};
                for (int kb = 0; kb < D; kb += kEdgeBlock) {
                    const int kw = D - kb < kEdgeBlock ? D - kb : kEdgeBlock;
                    for (int nb = 0; nb < D; nb += kEdgeBlock) {
                        const int nw = D - nb < kEdgeBlock ? D - nb : kEdgeBlock;
                        const float* X[1] = {h_in + kb};
                        if (int rc = ggnn_xty_acc_f32(X, 1, kw, ldx, pair_node, dHc + nb, D, out, nullptr, 0, kw, nw, 0, row_off_t, T, xty_ws,
                                                      xty_ws_bytes, side)) return rc;
                        out += (size_t)T * kw * nw;
                    }
                }
                const int n = T * D * D;
                hipLaunchKernelGGL(add_edge_blocks_kernel, dim3((n + 255) / 256), dim3(256), 0, side, g_edge[l], (const float*)blk, T, D);
                GGNN_CHECK_HIP(hipGetLastError());
            }
            // ---- accumulate what went to temporaries
            for (int i = 0; i < P.nres; ++i) {          // (sums into the gradient of h0 are not needed either)
                if (!dx_direct[i] && P.res[i] != 0) { if (int rc = add_inplace(dstate[P.res[i]], dxp[i], nvd, st)) return rc; }
            }
            if (s == 0 && !dh_direct && l != 0) { if (int rc = add_inplace(dstate[l], dh_dst, nvd, st)) return rc; }
            g = dh_dst;
        }
    }
    // every deferred node sum was consumed by the GRU (RNN cell) backward of the timestep before it (the only step that defers without a
    // consumer would be the very first one, which runs no transform): a pending one here means a gradient was dropped
    GGNN_CHECK_ARG(!z_pending, "internal: a deferred node sum of the transform backward was never added (fuse_node_sum invariant)");
    return order_after(st, side);          // the caller's next launches (optimizer, next forward) see every product
}

extern "C" int ggnn_sparse_train_forward_f32(
        const float* h0, int V, int D, int T, const int32_t* row_ptr, const int32_t* gather_row_c, const int32_t* pair_node,
        const int64_t* type_row_off, const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
        const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed, const float* const* bg,
        const float* const* bc, const float* const* gru_packed, const int32_t* gru_fmt, int act, void* ws, size_t ws_bytes,
        int64_t* final_state_offset, ggnn_stream_t stream) {
    return train_forward(h0, V, D, T, row_ptr, gather_row_c, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                         res_idx, edge_packed, bg, bc, gru_packed, gru_fmt, act, ws, ws_bytes, final_state_offset, nullptr, nullptr,
                         TrainRoute{false}, stream);
}

extern "C" int ggnn_sparse_train_backward_f32(
        const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const int32_t* rows_rp, const int32_t* rows_gather, const int32_t* rows_heads,
        const int32_t* node_rp, const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
        const float* const* edge_packed_t, const float* const* gru_bwd_packed, int act,
        float* const* g_edge, float* const* g_Wg, float* const* g_bg, float* const* g_Wc, float* const* g_bc,
        float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    return train_backward(h0, V, D, T, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr, res_idx, rows_rp,
                          rows_gather, rows_heads, node_rp, node_order, node_heads, identity_rows, edge_packed_t, gru_bwd_packed, act,
                          g_edge, g_Wg, g_bg, g_Wc, g_bc, d_final, d_state_ws, ws, ws_bytes, nullptr, nullptr, TrainRoute{false}, stream, side_stream);
}

// ---- the default model's two sequences at the column-panel sizes 128 / 192 / 256 (see the header comment) ---------------------------
extern "C" size_t ggnn_sparse_train_panel_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps) {
    if (V <= 0 || T <= 0 || T > 64 || total_steps <= 0 || compact_rows < 0 || compact_rows >= (1LL << 31) || !TrainRoute{true}.takes(D)) return 0;
    if ((long long)V * total_steps >= (1LL << 31)) return 0;
    return train_layout(V, D, T, compact_rows, total_steps, 0, true).total;
}

extern "C" int ggnn_sparse_train_panel_forward_f32(
        const float* h0, int V, int D, int T, const int32_t* row_ptr, const int32_t* gather_row_c, const int32_t* pair_node,
        const int64_t* type_row_off, const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
        const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed, const float* const* bg,
        const float* const* bc, const float* const* gru_packed, const int32_t* gru_fmt, int act, void* ws, size_t ws_bytes,
        int64_t* final_state_offset, ggnn_stream_t stream) {
    return train_forward(h0, V, D, T, row_ptr, gather_row_c, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                         res_idx, edge_packed, bg, bc, gru_packed, gru_fmt, act, ws, ws_bytes, final_state_offset, nullptr, nullptr,
                         TrainRoute{true}, stream);
}

extern "C" int ggnn_sparse_train_panel_backward_f32(
        const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const int32_t* rows_rp, const int32_t* rows_gather, const int32_t* rows_heads,
        const int32_t* node_rp, const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
        const float* const* edge_packed_t, const float* const* gru_bwd_packed, int act,
        float* const* g_edge, float* const* g_Wg, float* const* g_bg, float* const* g_Wc, float* const* g_bc,
        float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    return train_backward(h0, V, D, T, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr, res_idx, rows_rp,
                          rows_gather, rows_heads, node_rp, node_order, node_heads, identity_rows, edge_packed_t, gru_bwd_packed, act,
                          g_edge, g_Wg, g_bg, g_Wc, g_bc, d_final, d_state_ws, ws, ws_bytes, nullptr, nullptr, TrainRoute{true}, stream, side_stream);
}

// ---- the same two sequences with propagation attention on the compacted route (see the header comment) -----------------------------
extern "C" int ggnn_sparse_attn_train_forward_f32(
        const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr, const int32_t* slot_pair, const int32_t* slot_row,
        const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg, int num_layers,
        const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed,
        const float* const* attn_factors, const float* const* bg, const float* const* bc, const float* const* gru_packed, int act,
        void* ws, size_t ws_bytes, int64_t* final_state_offset, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(slot_pair && slot_row && attn_factors, "null pointer (attention index / factors)");
    GGNN_CHECK_ARG(M > 0 && M < (1LL << 31), "bad message count %lld", (long long)M);
    const AttnForward at{slot_pair, attn_factors, M};
    return train_forward(h0, V, D, T, row_ptr, slot_row, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                         res_idx, edge_packed, bg, bc, gru_packed, nullptr, act, ws, ws_bytes, final_state_offset, &at, nullptr, TrainRoute{false}, stream);
}

extern "C" int ggnn_sparse_attn_train_backward_f32(
        const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr, const int32_t* slot_pair, const int32_t* slot_row,
        const int32_t* msg_perm, const int64_t* msg_type_off, const int32_t* pair_node, const int64_t* type_row_off, const float* nin,
        int use_avg, int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const int32_t* src_node_ptr, const int32_t* src_dst, const int32_t* src_msg, const int32_t* src_row,
        const int32_t* node_rp, const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
        const float* const* edge_packed, const float* const* edge_packed_t, const float* const* gru_bwd_packed,
        const float* const* attn_factors, int act, float* const* g_edge, float* const* g_attn, float* const* g_Wg, float* const* g_bg,
        float* const* g_Wc, float* const* g_bc, float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes,
        ggnn_stream_t stream, ggnn_stream_t side_stream) {
    GGNN_CHECK_ARG(row_ptr && slot_pair && slot_row && msg_perm && msg_type_off && src_node_ptr && src_dst && src_msg && src_row &&
                   edge_packed && attn_factors && g_attn, "null pointer (attention index / factors / gradient views)");
    GGNN_CHECK_ARG(M > 0 && M < (1LL << 31), "bad message count %lld", (long long)M);
    if (D > 0 && (ggnn_gru_is_fused(D) != 1 || !ggnn_msg_transform_compact_supported(D)))          // (what the forward call takes)
        return fail(GGNN_E_UNSUPPORTED, "native training step: hidden size %d has no gather-fused GRU / compacted transform", D);
    const AttnBackward at{row_ptr, slot_pair, slot_row, msg_perm, msg_type_off, src_node_ptr, src_dst, src_msg, src_row,
                          edge_packed, attn_factors, g_attn, M};
    return train_backward(h0, V, D, T, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr, res_idx, nullptr,
                          nullptr, nullptr, node_rp, node_order, node_heads, identity_rows, edge_packed_t, gru_bwd_packed, act, g_edge,
                          g_Wg, g_bg, g_Wc, g_bc, d_final, d_state_ws, ws, ws_bytes, &at, nullptr, TrainRoute{false}, stream, side_stream);
}

// ---- the same two sequences for the BasicRNNCell on the compacted route (graph_rnn_cell = RNN; see RnnForward / RnnBackward) ---------
extern "C" size_t ggnn_sparse_rnn_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps) {
    if (V <= 0 || T <= 0 || T > 64 || total_steps <= 0 || compact_rows < 0 || compact_rows >= (1LL << 31)) return 0;
    if (!ggnn_rnn_fused_supported(D, 1) || !ggnn_msg_transform_compact_supported(D)) return 0;
    return train_layout(V, D, T, compact_rows, total_steps, 0, false, true).total;
}

extern "C" int ggnn_sparse_rnn_train_forward_f32(
        const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr, const int32_t* gather_row_c, const int32_t* pair_node,
        const int64_t* type_row_off, const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
        const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed, const float* const* rnn_b,
        const float* const* rnn_packed, int act, void* ws, size_t ws_bytes, int64_t* final_state_offset, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(rnn_b && rnn_packed, "null pointer (cell weights)");
    const RnnForward rn{rnn_packed, rnn_b, M};
    return train_forward(h0, V, D, T, row_ptr, gather_row_c, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr,
                         res_idx, edge_packed, nullptr, nullptr, nullptr, nullptr, act, ws, ws_bytes, final_state_offset, nullptr, &rn,
                         TrainRoute{false}, stream);
}

extern "C" int ggnn_sparse_rnn_train_backward_f32(
        const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg,
        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
        const int32_t* rows_rp, const int32_t* rows_gather, const int32_t* rows_heads,
        const int32_t* node_rp, const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
        const float* const* edge_packed_t, const float* const* rnn_bwd_packed, int act,
        float* const* g_edge, float* const* g_W, float* const* g_b,
        float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream) {
    GGNN_CHECK_ARG(rnn_bwd_packed && g_W && g_b, "null pointer (cell weights / gradient views)");
    const RnnBackward rn{rnn_bwd_packed, g_W, g_b};
    return train_backward(h0, V, D, T, pair_node, type_row_off, nin, use_avg, num_layers, layer_timesteps, res_ptr, res_idx, rows_rp,
                          rows_gather, rows_heads, node_rp, node_order, node_heads, identity_rows, edge_packed_t, nullptr, act,
                          g_edge, nullptr, nullptr, nullptr, nullptr, d_final, d_state_ws, ws, ws_bytes, nullptr, &rn, TrainRoute{false},
                          stream, side_stream);
}
