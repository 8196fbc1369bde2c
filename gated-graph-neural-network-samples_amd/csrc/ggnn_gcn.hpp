// What the GCN layer kernels share (ggnn_gcn.hip: hidden sizes 32 / 64 / 100; ggnn_gcn_panel.hip: 128 / 192 / 256): the weighted
// accumulation of a gathered row into the aggregate fragment, the epilogue out = dropout(relu(P + b)) and the ReLU gate of the
// layer-backward forms.
#pragma once
#include "ggnn_split.hpp"
#include "ggnn_philox.hpp"

namespace ggnn {

template <int D>
__device__ __forceinline__ void frag_fma(Frag<D>& a, float w, const Frag<D>& t) {
#pragma unroll
    for (int c = 0; c < StageCfg<D>::NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) a.v[c][e] = __builtin_fmaf(w, t.v[c][e], a.v[c][e]);
#pragma unroll
    for (int q = 0; q < StageCfg<D>::NR; ++q) a.r[q] = __builtin_fmaf(w, t.r[q], a.r[q]);
}

struct GcnEpilogue {
    const float* bias;          // [D] or null
    int relu;
    const int64_t* row_key;     // [V] or null: row_key_base + row
    int64_t row_key_base;
    uint32_t k0, k1;            // dropout seed
    float keep;                 // >= 1: no dropout
};

// tf.nn.dropout's factor for the 4 columns 4q .. 4q+3 of a row: the expression of ggnn_dropout_f32, term for term
__device__ __forceinline__ f32x4 gcn_epilogue(f32x4 v, int row, int col, const GcnEpilogue& ep) {
    if (ep.bias) v += *reinterpret_cast<const f32x4*>(ep.bias + col);
    if (ep.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
    }
    if (ep.keep < 1.0f) {
        const uint64_t key = (uint64_t)(ep.row_key ? ep.row_key[row] : ep.row_key_base + row);
        uint32_t u[4];
        philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)(col >> 2), 0u, ep.k0, ep.k1, u);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / ep.keep * floorf(ep.keep + (float)(u[e] >> 8) * (1.0f / 16777216.0f));
    }
    return v;
}

// d v / d P of out = dropout(relu(P)) given out: ggnn_act_bwd_f32's ReLU select, term for term
__device__ __forceinline__ f32x4 gcn_relu_gate(f32x4 v, f32x4 gate) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gate[e] > 0.f ? v[e] : 0.f;
    return v;
}

inline size_t align256g(size_t x) { return (x + 255) / 256 * 256; }

inline bool gcn_epilogue_args(const float* bias, float keep_prob) {
    return (keep_prob > 0.0f && keep_prob <= 1.0f) && (!bias || aligned16(bias));
}

}  // namespace ggnn
