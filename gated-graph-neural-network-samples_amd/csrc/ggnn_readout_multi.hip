// Multi-task fused readout + masked loss, forward and backward: the arithmetic of ggnn_readout.hip
// (chem_tensorflow_sparse.py:220-231 gated_regression, chem_tensorflow.py:158-170 masked loss / MAE) for the K entries of task_ids
// (chem_tensorflow.py:150-170 loops over them) in ONE pass over the node states:
//     gate[v,k] = sigmoid([hT[v] | h0[v]] . Wg_k + bg_k),   val[v,k] = hT[v] . Wt_k + bt_k
//     out[k,g]  = sum over the nodes v of graph g of gate[v,k] val[v,k] (node_mask[v])
//     stats[k]  = (sum_g 0.5 diff^2, sum_g |diff|, sum_g m)   with diff = (out[k,g] - target[k,g]) m,  m = mask[k,g]
// hT and h0 are read once by the forward and once by the backward whatever K is, and d_hT is written once.  The K weight vectors
// ([2D] gate, [D] transform) of a call are staged once per workgroup in LDS as one [K][3D] image; all arithmetic is plain f32 on the
// VALU (the products are [V,3D] x [3D,K] and its two transposes: about 1 GF per pass at V = 1e5, K = 16).
// Deterministic and atomics-free like the per-task kernels: graph_nodes_list non-decreasing, every cross-lane, cross-block and
// cross-task sum in a fixed order.  Every per-task quantity (out, stats, the weight and bias gradients) is summed in an order that
// does not depend on K: task k of a K = 13 call and of a K = 5 call give the same bits.
//
//   forward   node kernel : 16 lanes per node hold the node's hT / h0 columns (float4 per lane and slot) in registers and walk
//                           the K tasks over the LDS weights; after the butterfly reduction every lane has the two sums, lane k
//                           keeps task k's, applies bias and sigmoid and writes node_gv[v] = (gate[v,0..K) | val[v,0..K))
//             graph kernel: thread (graph, task): out[k,g] in node order; per-block partials of the three sums of every task
//                           (a fixed pairwise tree over the block's 64 graphs)
//             stats kernel: one block per task: the block partials in a fixed order
//   backward  node kernel : a workgroup walks tiles of 16 nodes.  Per tile: (1) thread (node, task) forms
//                           dO = d_out[k,g] + d_num_k m^2 (out-y) + d_abs_k m sign(diff), dval = dO gate, dpre = dO val gate (1-gate)
//                           into LDS, and the tile's hT / h0 rows (prefetched into registers during the previous tile) go to LDS;
//                           (2) d_hT[v] (+)= sum_k dpre[v,k] Wg_k[:D] + dval[v,k] Wt_k, tasks in order;
//                           (3) the [K, 3D+2] weight-gradient accumulators are tiled over the 256 threads: thread (task k, column
//                           group c) owns the float4 columns c, c+16, .. of [dpre hT | dpre h0 | dval hT] of task k in registers and
//                           adds the tile's nodes in node order.  Block partials go to the workspace.
//             final kernel: the block partials in 8 fixed chains per (task, column) -> the K destinations of every gradient
#include "ggnn_common.h"

namespace ggnn {

constexpr int kRmMaxTasks = 16;                 // = lanes per node of the forward: lane k keeps task k
constexpr int kRmLanes = 16;
constexpr int kRmFwdBlocks = 1024;              // forward node kernel: four 4-wave blocks per CU
constexpr int kRmBwdBlocks = 512;               // backward node kernel: partials are nb x K x (3D+4) floats
constexpr int kRmTile = 16;                     // nodes per backward tile
constexpr int kRmGraphs = 64;                   // graphs per block of the graph kernel

// kernel-argument images of the host arrays of K device pointers (indexed by a wave-uniform task only)
struct RmWeights { const float* gate_W[kRmMaxTasks]; const float* gate_b[kRmMaxTasks];
                   const float* transform_W[kRmMaxTasks]; const float* transform_b[kRmMaxTasks]; };
struct RmGrads { float* gate_W[kRmMaxTasks]; float* gate_b[kRmMaxTasks]; float* transform_W[kRmMaxTasks]; float* transform_b[kRmMaxTasks]; };

// [K][3D] LDS image: row k = gate_W[k] (2D) | transform_W[k] (D)
__device__ __forceinline__ void rm_stage_weights(float* __restrict__ wl, const RmWeights& w, int D, int K) {
    const int D4 = D >> 2;
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ gw = w.gate_W[k];
        const float* __restrict__ tw = w.transform_W[k];
        for (int i = threadIdx.x; i < 3 * D4; i += 256) {
            const f32x4 x = i < 2 * D4 ? *reinterpret_cast<const f32x4*>(gw + 4 * i) : *reinterpret_cast<const f32x4*>(tw + 4 * (i - 2 * D4));
            *reinterpret_cast<f32x4*>(wl + (size_t)k * 3 * D + 4 * i) = x;
        }
    }
}

// S = float4 column slots per lane: D <= 64 -> 1, D <= 128 -> 2, D <= 256 -> 4
template <int S>
__global__ __launch_bounds__(256) void rm_node_kernel(const float* __restrict__ hT, const float* __restrict__ h0, const RmWeights w,
                                                      float* __restrict__ node_gv, int V, int D, int K) {
    constexpr int LPN = kRmLanes, NPB = 256 / LPN;
    extern __shared__ float rm_lds[];                               // [K][3D] weights | [K] gate_b | [K] transform_b
    float* wl = rm_lds;
    float* bl = rm_lds + (size_t)K * 3 * D;
    rm_stage_weights(wl, w, D, K);
    for (int k = 0; k < K; ++k) {                                   // (k uniform: the pointer arrays are read by scalar loads)
        if (threadIdx.x == 2 * k) bl[k] = w.gate_b[k][0];
        if (threadIdx.x == 2 * k + 1) bl[kRmMaxTasks + k] = w.transform_b[k][0];
    }
    __syncthreads();
    const int l = threadIdx.x % LPN, grp = threadIdx.x / LPN;
    const int D4 = D >> 2;
    const int stride = gridDim.x * NPB;
    f32x4 a[S], b[S];
    auto load = [&](int base, f32x4* pa, f32x4* pb) {
        int v = base + grp;
        v = v < V ? v : V - 1;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int c4 = l + s * LPN;
            const bool on = c4 < D4;
            pa[s] = on ? *reinterpret_cast<const f32x4*>(hT + (size_t)v * D + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
            pb[s] = on ? *reinterpret_cast<const f32x4*>(h0 + (size_t)v * D + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    load(blockIdx.x * NPB, a, b);
    for (int base = blockIdx.x * NPB; base < V; base += stride) {   // uniform trip count: the shuffles below see whole waves
        f32x4 na[S], nb[S];
        load(base + stride < V ? base + stride : base, na, nb);     // next node's rows, in flight during this node's K tasks
        const int v = base + grp;
        float mysg = 0.f, myst = 0.f;
        for (int k = 0; k < K; ++k) {
            const float* wk = wl + (size_t)k * 3 * D;
            float sg = 0.f, st = 0.f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int c4 = l + s * LPN;
                if (c4 < D4) {
                    const f32x4 wa = *reinterpret_cast<const f32x4*>(wk + 4 * c4);
                    const f32x4 wb = *reinterpret_cast<const f32x4*>(wk + D + 4 * c4);
                    const f32x4 wt = *reinterpret_cast<const f32x4*>(wk + 2 * D + 4 * c4);
                    const f32x4 x = a[s], y = b[s];
                    sg += x.x * wa.x + x.y * wa.y + x.z * wa.z + x.w * wa.w + y.x * wb.x + y.y * wb.y + y.z * wb.z + y.w * wb.w;
                    st += x.x * wt.x + x.y * wt.y + x.z * wt.z + x.w * wt.w;
                }
            }
#pragma unroll
            for (int off = LPN / 2; off > 0; off >>= 1) {
                sg += __shfl_xor(sg, off, LPN);
                st += __shfl_xor(st, off, LPN);
            }
            if (l == k) { mysg = sg; myst = st; }
        }
        if (v < V && l < K) {
            const size_t o = (size_t)v * 2 * K;
            node_gv[o + l] = 1.0f / (1.0f + expf(-(mysg + bl[l])));
            node_gv[o + K + l] = myst + bl[kRmMaxTasks + l];
        }
#pragma unroll
        for (int s = 0; s < S; ++s) { a[s] = na[s]; b[s] = nb[s]; }
    }
}

// first node of graph g in the non-decreasing graph_nodes_list, clamped to [0, V] (graph_ptr == NULL: binary search)
__device__ __forceinline__ int rm_graph_begin(const int* __restrict__ graph_of, const int* __restrict__ graph_ptr, int g, int V) {
    if (graph_ptr) {
        const int p = graph_ptr[g];
        return p < 0 ? 0 : (p > V ? V : p);
    }
    int lo = 0, hi = V;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (graph_of[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// thread (task k = tid % 16, graph slot tid / 16 + 16 j): a block owns 64 consecutive graphs whatever K is
__global__ __launch_bounds__(256) void rm_graph_kernel(const float* __restrict__ node_gv, const int* __restrict__ graph_of,
                                                       const int* __restrict__ graph_ptr, const float* __restrict__ node_mask,
                                                       const float* __restrict__ target, const float* __restrict__ mask,
                                                       float* __restrict__ out, float* __restrict__ partials, int V, int G, int K) {
    __shared__ float red[3][16][kRmMaxTasks];
    const int k = threadIdx.x % kRmMaxTasks, gi = threadIdx.x / kRmMaxTasks;
    float num[kRmGraphs / 16], ab[kRmGraphs / 16], ms[kRmGraphs / 16];
#pragma unroll
    for (int j = 0; j < kRmGraphs / 16; ++j) {
        const int g = blockIdx.x * kRmGraphs + gi + 16 * j;
        num[j] = ab[j] = ms[j] = 0.f;
        if (g < G && k < K) {
            const int beg = rm_graph_begin(graph_of, graph_ptr, g, V), end = rm_graph_begin(graph_of, graph_ptr, g + 1, V);
            float s = 0.f;
            for (int v = beg; v < end; ++v) {
                const float gt = node_gv[(size_t)v * 2 * K + k], vl = node_gv[(size_t)v * 2 * K + K + k];
                s += node_mask ? gt * vl * node_mask[v] : gt * vl;
            }
            const size_t o = (size_t)k * G + g;
            out[o] = s;
            if (target) {
                const float m = mask ? mask[o] : 1.0f;
                const float diff = (s - target[o]) * m;             // chem_tensorflow.py:161,164
                num[j] = 0.5f * diff * diff; ab[j] = fabsf(diff); ms[j] = m;
            }
        }
    }
    if (!partials) return;
    // the block's 64 graphs of task k in a fixed pairwise tree: the thread's four, then the 16 graph slots through LDS
    static_assert(kRmGraphs == 64, "the tree below sums four graphs per thread");
    red[0][gi][k] = (num[0] + num[1]) + (num[2] + num[3]);
    red[1][gi][k] = (ab[0] + ab[1]) + (ab[2] + ab[3]);
    red[2][gi][k] = (ms[0] + ms[1]) + (ms[2] + ms[3]);
    __syncthreads();
    for (int off = 8; off > 0; off >>= 1) {
        if (gi < off) {
            red[0][gi][k] += red[0][gi + off][k];
            red[1][gi][k] += red[1][gi + off][k];
            red[2][gi][k] += red[2][gi + off][k];
        }
        __syncthreads();
    }
    if (gi < 3 && k < K) partials[((size_t)blockIdx.x * kRmMaxTasks + k) * 3 + gi] = red[gi][0][k];
}

// block k: thread t sums the block partials b == t (mod 64) in order, then a fixed tree over the 64 chains
__global__ __launch_bounds__(64) void rm_stats_kernel(const float* __restrict__ partials, int nblocks, float* __restrict__ stats) {
    __shared__ float red[3][64];
    const int k = blockIdx.x, t = threadIdx.x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int b = t; b < nblocks; b += 64) {
        const float* p = partials + ((size_t)b * kRmMaxTasks + k) * 3;
        s0 += p[0]; s1 += p[1]; s2 += p[2];
    }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (t < off) { red[0][t] += red[0][t + off]; red[1][t] += red[1][t + off]; red[2][t] += red[2][t + off]; }
        __syncthreads();
    }
    if (t < 3) stats[k * 3 + t] = red[t][0];
}

// J = float4 accumulator slots per thread (3 D/4 columns over 16 column groups): D <= 64 -> 3, D <= 128 -> 6, D <= 256 -> 12
template <int J>
__global__ __launch_bounds__(256) void rm_bwd_node_kernel(
        const float* __restrict__ hT, const float* __restrict__ h0, const int* __restrict__ graph_of,
        const float* __restrict__ node_mask, const RmWeights w, const float* __restrict__ node_gv, const float* __restrict__ out,
        const float* __restrict__ target, const float* __restrict__ mask, const float* __restrict__ d_out,
        const float* __restrict__ d_stats, float* __restrict__ d_hT, int accumulate, float* __restrict__ partials,
        int V, int D, int K, int G) {
    constexpr int NT = kRmTile, R = J / 3;                          // R float4 per thread and array cover a [16, D] tile
    extern __shared__ float rm_lds[];
    const int D4 = D >> 2, Q = 3 * D4;
    float* wl = rm_lds;                                             // [K][3D]
    float* xs = wl + (size_t)K * 3 * D;                             // [NT][D] hT tile, then [NT][D] h0 tile
    float* cf = xs + 2 * NT * D;                                    // [NT][2][16]: dpre | dval of (node, task)
    rm_stage_weights(wl, w, D, K);
    const int k = threadIdx.x % kRmMaxTasks, cg = threadIdx.x / kRmMaxTasks;
    const float d_num = (d_stats && k < K) ? d_stats[2 * k] : 0.f, d_abs = (d_stats && k < K) ? d_stats[2 * k + 1] : 0.f;
    // accumulator slot j = float4 column q = cg + 16 j of [dpre hT | dpre h0 | dval hT]: its source in xs and its coefficient
    int src[J];
    bool by_pre[J];
    f32x4 acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int q = cg + 16 * j;
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        by_pre[j] = q < 2 * D4;
        src[j] = q < D4 ? 4 * q : (q < 2 * D4 ? NT * D + 4 * (q - D4) : (q < Q ? 4 * (q - 2 * D4) : 0));   // (q >= Q: an unused slot)
    }
    float accp = 0.f, accv = 0.f;                                   // bias sums of task k (column group 0 only)
    const int ntiles = (V + NT - 1) / NT;
    f32x4 ra[R], rb[R];
    auto load = [&](int tile) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = threadIdx.x + 256 * r;                  // float4 idx of the tile = (node idx / D4, column idx % D4)
            const int n = idx / D4;
            const bool on = idx < NT * D4 && tile * NT + n < V;
            const size_t o = (size_t)tile * NT * D + 4 * (size_t)idx;
            ra[r] = on ? *reinterpret_cast<const f32x4*>(hT + o) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[r] = on ? *reinterpret_cast<const f32x4*>(h0 + o) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if ((int)blockIdx.x < ntiles) load(blockIdx.x);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // (1) the tile's rows and coefficients into LDS
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = threadIdx.x + 256 * r;
            if (idx < NT * D4) {
                *reinterpret_cast<f32x4*>(xs + 4 * idx) = ra[r];
                *reinterpret_cast<f32x4*>(xs + NT * D + 4 * idx) = rb[r];
            }
        }
        {
            const int v = tile * NT + cg;
            float dpre = 0.f, dval = 0.f;
            if (v < V && k < K) {
                const int g = graph_of[v];
                float dO = 0.f;
                if ((unsigned)g < (unsigned)G) {
                    const size_t o = (size_t)k * G + g;
                    if (d_out) dO = d_out[o];
                    if (target) {
                        const float m = mask ? mask[o] : 1.0f;
                        const float diff = (out[o] - target[o]) * m;
                        dO += d_num * diff * m + d_abs * m * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));
                    }
                }
                if (node_mask) dO *= node_mask[v];
                const float gt = node_gv[(size_t)v * 2 * K + k], vl = node_gv[(size_t)v * 2 * K + K + k];
                dval = dO * gt; dpre = dO * vl * gt * (1.0f - gt);
            }
            cf[(cg * 2 + 0) * kRmMaxTasks + k] = dpre;
            cf[(cg * 2 + 1) * kRmMaxTasks + k] = dval;
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load(tile + gridDim.x);  // next tile's rows, in flight during (2) and (3)
        // (2) d_hT of the tile: thread (node, float4 column), tasks in order
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int idx = threadIdx.x + 256 * r;
            const int n = idx / D4, c4 = idx - n * D4;
            if (idx < NT * D4 && tile * NT + n < V) {
                f32x4 dh = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int kk = 0; kk < K; ++kk) {
                    const float p = cf[(n * 2 + 0) * kRmMaxTasks + kk], dv = cf[(n * 2 + 1) * kRmMaxTasks + kk];
                    const f32x4 wa = *reinterpret_cast<const f32x4*>(wl + (size_t)kk * 3 * D + 4 * c4);
                    const f32x4 wt = *reinterpret_cast<const f32x4*>(wl + (size_t)kk * 3 * D + 2 * D + 4 * c4);
                    dh += p * wa + dv * wt;
                }
                const size_t o = (size_t)tile * NT * D + 4 * (size_t)idx;
                if (accumulate) dh += *reinterpret_cast<const f32x4*>(d_hT + o);
                *reinterpret_cast<f32x4*>(d_hT + o) = dh;
            }
        }
        // (3) weight-gradient accumulators: the tile's nodes in node order (rows past V are zero coefficients and zero rows)
        const int nn = V - tile * NT < NT ? V - tile * NT : NT;
        for (int n = 0; n < nn; ++n) {
            const float p = cf[(n * 2 + 0) * kRmMaxTasks + k], dv = cf[(n * 2 + 1) * kRmMaxTasks + k];
            const float* row = xs + n * D;
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] += (by_pre[j] ? p : dv) * *reinterpret_cast<const f32x4*>(row + src[j]);
            accp += p; accv += dv;
        }
        __syncthreads();
    }
    if (k < K) {
        float* mine = partials + ((size_t)blockIdx.x * K + k) * (3 * D + 4);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = cg + 16 * j;
            if (q < Q) *reinterpret_cast<f32x4*>(mine + 4 * q) = acc[j];
        }
        if (cg == 0) { mine[3 * D] = accp; mine[3 * D + 1] = accv; }
    }
}

// grid (columns / 32, K).  A block = 32 columns x 8 chains of one task, as readout_bwd_final_kernel: chain q sums the block
// partials b == q (mod 8) of its column in order, the chains are combined pairwise.
__global__ __launch_bounds__(256) void rm_bwd_final_kernel(const float* __restrict__ partials, int nblocks, int D, int K, const RmGrads d) {
    __shared__ float red[8][32];
    const int W = 3 * D + 2, WL = 3 * D + 4;
    const int k = blockIdx.y;
    const int c = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + c;
    float acc = 0.f;
    if (i < W) {
        const float* p = partials + (size_t)k * WL + i;
        const size_t bs = (size_t)K * WL;
        int b = q;
        for (; b + 24 < nblocks; b += 32) {
            const float v0 = p[(size_t)b * bs], v1 = p[(size_t)(b + 8) * bs], v2 = p[(size_t)(b + 16) * bs], v3 = p[(size_t)(b + 24) * bs];
            acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; b < nblocks; b += 8) acc += p[(size_t)b * bs];
    }
    red[q][c] = acc;
    __syncthreads();
    if (q != 0 || i >= W) return;
    const float s = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + ((red[4][c] + red[5][c]) + (red[6][c] + red[7][c]));
    if (i < 2 * D) d.gate_W[k][i] = s;
    else if (i < 3 * D) d.transform_W[k][i - 2 * D] = s;
    else if (i == 3 * D) d.gate_b[k][0] = s;
    else d.transform_b[k][0] = s;
}

static inline int rm_fwd_blocks(int V) { const int nb = (V + 15) / 16; return nb < kRmFwdBlocks ? nb : kRmFwdBlocks; }
static inline int rm_bwd_blocks(int V) { const int nb = (V + kRmTile - 1) / kRmTile; return nb < kRmBwdBlocks ? nb : kRmBwdBlocks; }
// dynamic LDS of a launch; the kernels' limit is raised ONCE per instantiation and device, so it is raised to the instantiation's
// maximum (K = kRmMaxTasks at the widest D it serves), never to the size of the call that happens to come first
constexpr size_t rm_fwd_lds(int D, int K) { return ((size_t)K * 3 * D + 2 * kRmMaxTasks) * sizeof(float); }
constexpr size_t rm_bwd_lds(int D, int K) { return ((size_t)K * 3 * D + 2 * (size_t)kRmTile * D + 2 * kRmTile * kRmMaxTasks) * sizeof(float); }
constexpr int rm_bwd_max_width(int J) { return J == 3 ? 64 : (J == 6 ? 128 : 256); }
static inline float* rm_align(void* ws) { return reinterpret_cast<float*>((reinterpret_cast<size_t>(ws) + 255) / 256 * 256); }

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_readout_multi_supported(int D, int K) {
    return (D >= 4 && D <= 256 && D % 4 == 0 && K >= 1 && K <= kRmMaxTasks) ? 1 : 0;
}

extern "C" size_t ggnn_readout_multi_workspace_bytes(int V, int D, int K, int num_graphs) {
    if (V < 0 || D <= 0 || K <= 0 || num_graphs < 0) return 0;
    const size_t fwd = (size_t)((num_graphs + kRmGraphs - 1) / kRmGraphs) * kRmMaxTasks * 3 * sizeof(float);
    const size_t bwd = (size_t)rm_bwd_blocks(V) * K * (3 * (size_t)D + 4) * sizeof(float);
    return (fwd > bwd ? fwd : bwd) + 256;
}

extern "C" int ggnn_readout_multi_fwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const int32_t* graph_ptr,
                                          const float* node_mask, const float* const* gate_W, const float* const* gate_b,
                                          const float* const* transform_W, const float* const* transform_b, const float* target,
                                          const float* mask, float* out, float* node_gv, float* stats, void* ws, size_t ws_bytes,
                                          int V, int D, int K, int num_graphs, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && K > 0 && num_graphs >= 0, "bad sizes V=%d D=%d K=%d G=%d", V, D, K, num_graphs);
    if (!ggnn_readout_multi_supported(D, K))
        return fail(GGNN_E_UNSUPPORTED, "multi-task readout: hidden size %d with %d tasks (multiples of 4 up to 256, 1..%d tasks)", D, K, kRmMaxTasks);
    GGNN_CHECK_ARG(!stats || (target && ws), "stats need target values and a workspace");
    RmWeights w{};
    if (num_graphs > 0) {
        GGNN_CHECK_ARG(out, "null pointer");
        if (V > 0) {
            GGNN_CHECK_ARG(hT && h0 && graph_nodes_list && gate_W && gate_b && transform_W && transform_b && node_gv, "null pointer");
            GGNN_CHECK_ARG(aligned16(hT) && aligned16(h0), "pointers must be 16-byte aligned");
            for (int k = 0; k < K; ++k) {
                GGNN_CHECK_ARG(gate_W[k] && gate_b[k] && transform_W[k] && transform_b[k], "null weight pointer of task %d", k);
                GGNN_CHECK_ARG(aligned16(gate_W[k]) && aligned16(transform_W[k]), "weights of task %d must be 16-byte aligned", k);
                w.gate_W[k] = gate_W[k]; w.gate_b[k] = gate_b[k]; w.transform_W[k] = transform_W[k]; w.transform_b[k] = transform_b[k];
            }
        }
        if (stats && ws_bytes < ggnn_readout_multi_workspace_bytes(V, D, K, num_graphs))
            return fail(GGNN_E_WORKSPACE, "multi-task readout workspace too small");
    }
    hipStream_t st = (hipStream_t)stream;
    if (stats) GGNN_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)K * 3 * sizeof(float), st));
    if (num_graphs == 0) return GGNN_OK;
    if (V > 0) {
        const size_t lds = rm_fwd_lds(D, K);
        const int nb = rm_fwd_blocks(V);
        if (D <= 64) hipLaunchKernelGGL(rm_node_kernel<1>, dim3(nb), dim3(256), lds, st, hT, h0, w, node_gv, V, D, K);
        else if (D <= 128) hipLaunchKernelGGL(rm_node_kernel<2>, dim3(nb), dim3(256), lds, st, hT, h0, w, node_gv, V, D, K);
        else {
            static std::atomic<unsigned long long> lds_ok{0};
            constexpr size_t max_lds = rm_fwd_lds(256, kRmMaxTasks);
            if (lds > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&rm_node_kernel<4>, max_lds, lds_ok));
            hipLaunchKernelGGL(rm_node_kernel<4>, dim3(nb), dim3(256), lds, st, hT, h0, w, node_gv, V, D, K);
        }
        GGNN_CHECK_HIP(hipGetLastError());
    }
    const int nbg = (num_graphs + kRmGraphs - 1) / kRmGraphs;
    float* partials = stats ? rm_align(ws) : nullptr;
    hipLaunchKernelGGL(rm_graph_kernel, dim3(nbg), dim3(256), 0, st, (const float*)node_gv, graph_nodes_list, graph_ptr, node_mask, target,
                       mask, out, partials, V, num_graphs, K);
    GGNN_CHECK_HIP(hipGetLastError());
    if (stats) {
        hipLaunchKernelGGL(rm_stats_kernel, dim3(K), dim3(64), 0, st, (const float*)partials, nbg, stats);
        GGNN_CHECK_HIP(hipGetLastError());
    }
    return GGNN_OK;
}

extern "C" int ggnn_readout_multi_bwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const float* node_mask,
                                          const float* const* gate_W, const float* const* transform_W, const float* node_gv,
                                          const float* out, const float* target, const float* mask, const float* d_out,
                                          const float* d_stats, float* d_hT, int accumulate, float* const* d_gate_W,
                                          float* const* d_gate_b, float* const* d_transform_W, float* const* d_transform_b, void* ws,
                                          size_t ws_bytes, int V, int D, int K, int num_graphs, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && K > 0 && num_graphs >= 0, "bad sizes V=%d D=%d K=%d G=%d", V, D, K, num_graphs);
    if (!ggnn_readout_multi_supported(D, K))
        return fail(GGNN_E_UNSUPPORTED, "multi-task readout: hidden size %d with %d tasks (multiples of 4 up to 256, 1..%d tasks)", D, K, kRmMaxTasks);
    GGNN_CHECK_ARG(d_gate_W && d_gate_b && d_transform_W && d_transform_b && ws, "null pointer");
    RmGrads d{};
    for (int k = 0; k < K; ++k) {
        GGNN_CHECK_ARG(d_gate_W[k] && d_gate_b[k] && d_transform_W[k] && d_transform_b[k], "null gradient pointer of task %d", k);
        d.gate_W[k] = d_gate_W[k]; d.gate_b[k] = d_gate_b[k]; d.transform_W[k] = d_transform_W[k]; d.transform_b[k] = d_transform_b[k];
    }
    RmWeights w{};
    const bool work = V > 0 && num_graphs > 0;
    if (work) {
        GGNN_CHECK_ARG(hT && h0 && graph_nodes_list && gate_W && transform_W && node_gv && out && d_hT, "null pointer");
        GGNN_CHECK_ARG(!d_stats || target, "d_stats needs target values");
        GGNN_CHECK_ARG(aligned16(hT) && aligned16(h0) && aligned16(d_hT), "pointers must be 16-byte aligned");
        for (int k = 0; k < K; ++k) {
            GGNN_CHECK_ARG(gate_W[k] && transform_W[k], "null weight pointer of task %d", k);
            GGNN_CHECK_ARG(aligned16(gate_W[k]) && aligned16(transform_W[k]), "weights of task %d must be 16-byte aligned", k);
            w.gate_W[k] = gate_W[k]; w.transform_W[k] = transform_W[k];
        }
    }
    if (ws_bytes < ggnn_readout_multi_workspace_bytes(V, D, K, num_graphs)) return fail(GGNN_E_WORKSPACE, "multi-task readout workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* partials = rm_align(ws);
    int nb = 0;
    if (work) {
        nb = rm_bwd_blocks(V);
        const size_t lds = rm_bwd_lds(D, K);
#define GGNN_RM_BWD(J)                                                                                                                 \
        do {                                                                                                                           \
            static std::atomic<unsigned long long> lds_ok{0};                           /* one mask per instantiation */               \
            constexpr size_t max_lds = rm_bwd_lds(rm_bwd_max_width(J), kRmMaxTasks);                                                  \
            if (lds > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&rm_bwd_node_kernel<J>, max_lds, lds_ok));                           \
            hipLaunchKernelGGL(rm_bwd_node_kernel<J>, dim3(nb), dim3(256), lds, st, hT, h0, graph_nodes_list, node_mask, w, node_gv, out, \
                               target, mask, d_out, d_stats, d_hT, accumulate, partials, V, D, K, num_graphs);                          \
        } while (0)
        if (D <= 64) GGNN_RM_BWD(3);
        else if (D <= 128) GGNN_RM_BWD(6);
        else GGNN_RM_BWD(12);
#undef GGNN_RM_BWD
        GGNN_CHECK_HIP(hipGetLastError());
    }
    else if (V > 0 && d_hT && !accumulate) {                        // no graphs: every node's gradient is zero
        GGNN_CHECK_HIP(hipMemsetAsync(d_hT, 0, sizeof(float) * (size_t)V * D, st));
    }
    hipLaunchKernelGGL(rm_bwd_final_kernel, dim3((3 * D + 2 + 31) / 32, K), dim3(256), 0, st, (const float*)partials, nb, D, K, d);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
