// Propagation attention (chem_tensorflow_sparse.py:147-149, 170-196) over the rows of the COMPACTED message transform.
//
// The score of a message, <h[src], h[tgt]> * factor[type], does not depend on the transformed rows, so attention needs no
// dense [V, T*D] transform: the message of slot e is Hc[slot_row[e]] (Hc [R,D] = ggnn_msg_transform_compact_f32's output,
// slot_row = the remapped gather rows), slot_pair[e] = src*T + type still names the source node and the factor.
//
// Same layout and arithmetic as the dense-row kernels of ggnn_scatter.hip (one sub-wave of 16 / 32 / 64 lanes per target,
// max-shifted scores, expf, ONE division of the accumulated row by (S + 1e-7), then bias and mean; the backward treats the
// shift as a constant), with one difference in the traffic: the first kHeld slots of a target are loaded once -- their
// indices with one coalesced read, their h[src] and Hc rows all in flight together -- and their scores stay in registers
// between the passes.  Only the slots beyond kHeld recompute, pass by pass, as the dense-row kernels do for every slot
// (molecule batches never have more than kHeld messages into a node).  Per message the forward reads one h[src] row and one
// Hc row (dense-row kernel: two h[src] rows and one H row), the backward one of each (dense-row kernel: four and two).
// VALU only, no atomics, slot order = the reference's accumulation order: deterministic.
// attn_bwd_source_compact_kernel (the native training step's) closes the backward on the source side: see its comment.
#include "ggnn_common.h"

namespace ggnn {

constexpr int kHeld = 8;            // slots per target whose rows and scores are held in registers (<= the smallest sub-wave)
constexpr float kLowest = -3.402823466e+38f;

template <int LPR>
__device__ __forceinline__ float subwave_dot(f32x4 a, f32x4 b) {
    float part = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, LPR);
    return part;
}

__device__ __forceinline__ f32x4 row4(const float* __restrict__ base, int row, int D, int c4) {
    return *reinterpret_cast<const f32x4*>(base + (size_t)row * D + 4 * c4);
}

// The first kHeld slots of one target: indices, rows, and the raw dot products <h[src], h[tgt]>.
// Every lane of the block runs this (no divergence around the shuffles); slots >= n hold zeros and index 0.
template <int LPR>
struct HeldSlots {
    int g[kHeld];                   // src*T + type
    f32x4 hs[kHeld];                // h[src] columns of this lane
    f32x4 hc[kHeld];                // Hc[slot_row] columns of this lane
    float f[kHeld];                 // factor[type]
    float p[kHeld];                 // <h[src], h[tgt]>

    __device__ __forceinline__ void load(const float* __restrict__ Hc, const float* __restrict__ h,
                                         const int* __restrict__ slot_pair, const int* __restrict__ slot_row,
                                         const float* __restrict__ factors, f32x4 hv, int beg, int n, int l, bool col_ok, int c4,
                                         int D, int T) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        int gl = 0, rl = 0;
        if (l < kHeld && l < n) { gl = slot_pair[beg + l]; rl = slot_row[beg + l]; }
        int r[kHeld];
#pragma unroll
        for (int k = 0; k < kHeld; ++k) { g[k] = __shfl(gl, k, LPR); r[k] = __shfl(rl, k, LPR); }
#pragma unroll
        for (int k = 0; k < kHeld; ++k) {
            const bool on = col_ok && k < n;
            const int src = g[k] / T;
            hs[k] = on ? row4(h, src, D, c4) : zero;
            hc[k] = on ? row4(Hc, r[k], D, c4) : zero;
            f[k] = factors[g[k] - src * T];
        }
#pragma unroll
        for (int k = 0; k < kHeld; ++k) p[k] = subwave_dot<LPR>(hs[k], hv);
    }
};

template <int LPR>
__global__ __launch_bounds__(256) void attn_compact_kernel(
        const float* __restrict__ Hc, const float* __restrict__ h, const int* __restrict__ row_ptr,
        const int* __restrict__ slot_pair, const int* __restrict__ slot_row, const float* __restrict__ factors,
        const float* __restrict__ nin, const float* __restrict__ bias, int use_avg, float* __restrict__ out, int V, int D, int T) {
    constexpr int NODES = 256 / LPR;
    const int l = threadIdx.x % LPR;
    int v = blockIdx.x * NODES + threadIdx.x / LPR;
    const bool live = v < V;
    v = live ? v : V - 1;                                    // dead sub-waves stay in every shuffle, with no slots
    const int beg = row_ptr[v], end = live ? row_ptr[v + 1] : beg;
    const int n = end - beg;
    const int D4 = D >> 2;                                   // D4 <= LPR (checked by the launcher)
    const bool col_ok = l < D4;
    const int c4 = col_ok ? l : 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 hv = col_ok ? row4(h, v, D, c4) : zero;

    HeldSlots<LPR> s;
    s.load(Hc, h, slot_pair, slot_row, factors, hv, beg, n, l, col_ok, c4, D, T);
    auto score = [&](int g) {                                // slots beyond kHeld: recomputed in both passes
        const int src = g / T;
        return subwave_dot<LPR>(col_ok ? row4(h, src, D, c4) : zero, hv) * factors[g - src * T];
    };
    float sc[kHeld];
    float m = kLowest;
#pragma unroll
    for (int k = 0; k < kHeld; ++k) {
        sc[k] = s.p[k] * s.f[k];
        m = k < n ? fmaxf(m, sc[k]) : m;
    }
    for (int e = beg + kHeld; e < end; ++e) m = fmaxf(m, score(slot_pair[e]));
    f32x4 acc = zero;
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < kHeld; ++k) {
        if (k < n) {
            const float w = expf(sc[k] - m);
            S += w;
            acc += w * s.hc[k];
        }
    }
    for (int e = beg + kHeld; e < end; ++e) {
        const float w = expf(score(slot_pair[e]) - m);
        S += w;
        if (col_ok) acc += w * row4(Hc, slot_row[e], D, c4);
    }
    if (col_ok && live) {
        acc = acc / (S + 1e-7f);                             // :194
        float deg = 0.f;
        if ((use_avg || bias) && nin)
            for (int t = 0; t < T; ++t) deg += nin[(size_t)v * T + t];
        if (bias) {
            f32x4 b = zero;
            for (int t = 0; t < T; ++t) b += nin[(size_t)v * T + t] * row4(bias, t, D, c4);
            acc += b;
        }
        if (use_avg) acc = acc / (deg + 1e-7f);
        *reinterpret_cast<f32x4*>(out + (size_t)v * D + 4 * c4) = acc;
    }
}

// Backward per target (the formulas of attn_bwd_target_kernel, ggnn_scatter.hip):  p_e = <h[src_e], h[v]>, s_e = p_e f[t_e],
//   a_e = exp(s_e - max) / (sum_k exp(s_k - max) + 1e-7),  da_e = <Hc[slot_row[e]], d[v]>,  ds_e = a_e (da_e - sum_k a_k da_k)
//   dh[v] (+)= sum_e ds_e f[t_e] h[src_e];   by message id:  coef_a = a_e,  coef_s = ds_e f[t_e],  dfac = ds_e p_e.
template <int LPR>
__global__ __launch_bounds__(256) void attn_bwd_target_compact_kernel(
        const float* __restrict__ Hc, const float* __restrict__ h, const float* __restrict__ d, const int* __restrict__ row_ptr,
        const int* __restrict__ slot_pair, const int* __restrict__ slot_row, const int* __restrict__ msg_perm,
        const float* __restrict__ factors, float* __restrict__ coef_a, float* __restrict__ coef_s, float* __restrict__ dfac,
        float* __restrict__ dh, int accumulate, int V, int D, int T) {
    constexpr int NODES = 256 / LPR;
    const int l = threadIdx.x % LPR;
    int v = blockIdx.x * NODES + threadIdx.x / LPR;
    const bool live = v < V;
    v = live ? v : V - 1;
    const int beg = row_ptr[v], end = live ? row_ptr[v + 1] : beg;
    const int n = end - beg;
    const int D4 = D >> 2;
    const bool col_ok = l < D4;
    const int c4 = col_ok ? l : 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 hv = col_ok ? row4(h, v, D, c4) : zero;
    const f32x4 dv = col_ok ? row4(d, v, D, c4) : zero;

    HeldSlots<LPR> s;
    s.load(Hc, h, slot_pair, slot_row, factors, hv, beg, n, l, col_ok, c4, D, T);
    float da[kHeld];
#pragma unroll
    for (int k = 0; k < kHeld; ++k) da[k] = subwave_dot<LPR>(s.hc[k], dv);
    auto hsrc = [&](int g) { return col_ok ? row4(h, g / T, D, c4) : zero; };
    auto hrow = [&](int e) { return col_ok ? row4(Hc, slot_row[e], D, c4) : zero; };

    float m = kLowest;
#pragma unroll
    for (int k = 0; k < kHeld; ++k) m = k < n ? fmaxf(m, s.p[k] * s.f[k]) : m;
    for (int e = beg + kHeld; e < end; ++e) { const int g = slot_pair[e]; m = fmaxf(m, subwave_dot<LPR>(hsrc(g), hv) * factors[g % T]); }
    float S = 0.f;
    float w[kHeld];
#pragma unroll
    for (int k = 0; k < kHeld; ++k) {
        w[k] = k < n ? expf(s.p[k] * s.f[k] - m) : 0.f;
        S += w[k];
    }
    for (int e = beg + kHeld; e < end; ++e) { const int g = slot_pair[e]; S += expf(subwave_dot<LPR>(hsrc(g), hv) * factors[g % T] - m); }
    const float inv = 1.0f / (S + 1e-7f);
    float t1 = 0.f;
#pragma unroll
    for (int k = 0; k < kHeld; ++k) t1 += (w[k] * inv) * da[k];
    for (int e = beg + kHeld; e < end; ++e) {
        const int g = slot_pair[e];
        const float a = expf(subwave_dot<LPR>(hsrc(g), hv) * factors[g % T] - m) * inv;
        t1 += a * subwave_dot<LPR>(hrow(e), dv);
    }
    f32x4 acc = zero;
    const int my_mid = (l < kHeld && l < n) ? msg_perm[beg + l] : 0;      // lane k writes the coefficients of held slot k
#pragma unroll
    for (int k = 0; k < kHeld; ++k) {
        const float a = w[k] * inv;
        const float ds = a * (da[k] - t1);
        acc += (ds * s.f[k]) * s.hs[k];
        if (l == k && k < n) { coef_a[my_mid] = a; coef_s[my_mid] = ds * s.f[k]; dfac[my_mid] = ds * s.p[k]; }
    }
    for (int e = beg + kHeld; e < end; ++e) {
        const int g = slot_pair[e];
        const f32x4 hs = hsrc(g);
        const float f = factors[g % T];
        const float p = subwave_dot<LPR>(hs, hv);
        const float a = expf(p * f - m) * inv;
        const float ds = a * (subwave_dot<LPR>(hrow(e), dv) - t1);
        acc += (ds * f) * hs;
        if (l == 0) {
            const int mid = msg_perm[e];
            coef_a[mid] = a; coef_s[mid] = ds * f; dfac[mid] = ds * p;
        }
    }
    if (col_ok && live) {
        float* o = dh + (size_t)v * D + 4 * c4;
        if (accumulate) acc += *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = acc;
    }
}

// Source side of the backward, both transpose gathers in ONE pass over the messages LEAVING a node (by-(source, type) slots:
// a node's slots are consecutive, the slots of one (node, type) pair -- one compact row -- consecutive inside them):
//   dHc[slot_row[e]] = sum over the pair's slots of coef_a[msg_e] * d[dst_e]        (the weighted transpose of the forward gather)
//   dh[u]           += sum over the node's slots of coef_s[msg_e] * h[dst_e]        (the source-side state gradient)
// Bit for bit the two ggnn_weighted_segment_sum_f32 launches it replaces (same slot order, same acc += w * row, the old contents of
// dh added last).  Those walk every slot index -> weight -> row with nothing in flight; here the first kHeldSrc slots' indices come
// with one coalesced read each, their coefficients with one gathered read, and all their rows are in flight together.
// kHeldSrc = 4, not kHeld: two rows per slot are held and a molecule's atom sends ~2 messages (at most 4 bonds).  With 8 held slots
// the kernel took 110 VGPRs (4 waves/SIMD) and ran at 51.1 us against the two launches' 47.0 us (V = 99 989, M = 197 656, D = 100);
// with 4 it takes 62 (8 waves/SIMD) and runs at 40.9 us against 47.3 us (tools/attention_bench.py --leg source).
constexpr int kHeldSrc = 4;         // slots per source node whose rows are held in registers
template <int LPR>
__global__ __launch_bounds__(256) void attn_bwd_source_compact_kernel(
        const float* __restrict__ d, const float* __restrict__ h, const int* __restrict__ node_ptr, const int* __restrict__ slot_dst,
        const int* __restrict__ slot_msg, const int* __restrict__ slot_row, const float* __restrict__ coef_a,
        const float* __restrict__ coef_s, float* __restrict__ dHc, float* __restrict__ dh, int V, int D) {
    constexpr int NODES = 256 / LPR;
    const int l = threadIdx.x % LPR;
    int u = blockIdx.x * NODES + threadIdx.x / LPR;
    const bool live = u < V;
    u = live ? u : V - 1;                                    // dead sub-waves stay in every shuffle, with no slots
    const int beg = node_ptr[u], end = live ? node_ptr[u + 1] : beg;
    const int n = end - beg;
    const int D4 = D >> 2;                                   // D4 <= LPR (checked by the launcher)
    const bool col_ok = l < D4;
    const int c4 = col_ok ? l : 0;
    const bool with_dh = dh != nullptr;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // lane k holds the indices and coefficients of held slot k; lane kHeldSrc the row of the slot after them (kHeldSrc < LPR)
    int dl = 0, rl = -1;
    float al = 0.f, sl = 0.f;
    if (l <= kHeldSrc && l < n) rl = slot_row[beg + l];
    if (l < kHeldSrc && l < n) {
        dl = slot_dst[beg + l];
        const int mid = slot_msg[beg + l];
        al = coef_a[mid];
        sl = with_dh ? coef_s[mid] : 0.f;
    }
    int row[kHeldSrc + 1];
    float ca[kHeldSrc], cs[kHeldSrc];
    f32x4 dr[kHeldSrc], hr[kHeldSrc];
#pragma unroll
    for (int k = 0; k <= kHeldSrc; ++k) row[k] = __shfl(rl, k, LPR);       // (-1 past the node's last slot)
#pragma unroll
    for (int k = 0; k < kHeldSrc; ++k) {
        const int dst = __shfl(dl, k, LPR);
        ca[k] = __shfl(al, k, LPR);
        cs[k] = __shfl(sl, k, LPR);
        const bool on = col_ok && k < n;
        dr[k] = on ? row4(d, dst, D, c4) : zero;
        hr[k] = on && with_dh ? row4(h, dst, D, c4) : zero;
    }
    f32x4 acc_a = zero, acc_s = zero;
#pragma unroll
    for (int k = 0; k < kHeldSrc; ++k) {
        if (k < n) {
            acc_a += ca[k] * dr[k];
            acc_s += cs[k] * hr[k];
            if (row[k + 1] != row[k]) {                      // the pair's last slot
                if (col_ok) *reinterpret_cast<f32x4*>(dHc + (size_t)row[k] * D + 4 * c4) = acc_a;
                acc_a = zero;
            }
        }
    }
    for (int e = beg + kHeldSrc; e < end; ++e) {                // beyond the held slots: slot by slot
        const int dst = slot_dst[e], mid = slot_msg[e], r = slot_row[e];
        const int r_next = e + 1 < end ? slot_row[e + 1] : -1;
        if (col_ok) {
            acc_a += coef_a[mid] * row4(d, dst, D, c4);
            if (with_dh) acc_s += coef_s[mid] * row4(h, dst, D, c4);
            if (r_next != r) {
                *reinterpret_cast<f32x4*>(dHc + (size_t)r * D + 4 * c4) = acc_a;
                acc_a = zero;
            }
        }
    }
    if (col_ok && live && with_dh) {
        float* o = dh + (size_t)u * D + 4 * c4;
        acc_s += *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = acc_s;
    }
}

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_gather_segment_sum_attn_compact_f32(const float* Hc, const float* h, const int32_t* row_ptr,
                                                        const int32_t* slot_pair, const int32_t* slot_row,
                                                        const float* type_factors, const float* nin, const float* bias,
                                                        int use_avg, float* out, int V, int D, int T, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && D % 4 == 0 && T > 0, "bad sizes V=%d D=%d T=%d", V, D, T);
    if (D > 256) return fail(GGNN_E_UNSUPPORTED, "propagation attention supports hidden sizes up to 256 (got %d)", D);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(Hc && h && row_ptr && type_factors && out, "null pointer");
    GGNN_CHECK_ARG(!(bias || use_avg) || nin, "nin is required with bias or mean aggregation");
    GGNN_CHECK_ARG(aligned16(Hc) && aligned16(h) && aligned16(out) && (!bias || aligned16(bias)), "pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int D4 = D / 4;
#define GGNN_ATTN_COMPACT(LPR, NODES)                                                                                          \
    hipLaunchKernelGGL(attn_compact_kernel<LPR>, dim3((V + NODES - 1) / NODES), dim3(256), 0, st, Hc, h, row_ptr, slot_pair,   \
                       slot_row, type_factors, nin, bias, use_avg, out, V, D, T)
    if (D4 <= 16) GGNN_ATTN_COMPACT(16, 16);
    else if (D4 <= 32) GGNN_ATTN_COMPACT(32, 8);
    else GGNN_ATTN_COMPACT(64, 4);
#undef GGNN_ATTN_COMPACT
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

extern "C" int ggnn_attn_bwd_target_compact_f32(const float* Hc, const float* h, const float* d_att, const int32_t* row_ptr,
                                                const int32_t* slot_pair, const int32_t* slot_row, const int32_t* msg_perm,
                                                const float* type_factors, float* coef_a, float* coef_s, float* dfac, float* dh,
                                                int accumulate, int V, int D, int T, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && D % 4 == 0 && T > 0, "bad sizes V=%d D=%d T=%d", V, D, T);
    if (D > 256) return fail(GGNN_E_UNSUPPORTED, "propagation attention supports hidden sizes up to 256 (got %d)", D);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(Hc && h && d_att && row_ptr && type_factors && dh, "null pointer");
    GGNN_CHECK_ARG(aligned16(Hc) && aligned16(h) && aligned16(d_att) && aligned16(dh), "pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int D4 = D / 4;
#define GGNN_ATTN_BWD_COMPACT(LPR, NODES)                                                                                      \
    hipLaunchKernelGGL(attn_bwd_target_compact_kernel<LPR>, dim3((V + NODES - 1) / NODES), dim3(256), 0, st, Hc, h, d_att,     \
                       row_ptr, slot_pair, slot_row, msg_perm, type_factors, coef_a, coef_s, dfac, dh, accumulate, V, D, T)
    if (D4 <= 16) GGNN_ATTN_BWD_COMPACT(16, 16);
    else if (D4 <= 32) GGNN_ATTN_BWD_COMPACT(32, 8);
    else GGNN_ATTN_BWD_COMPACT(64, 4);
#undef GGNN_ATTN_BWD_COMPACT
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

extern "C" int ggnn_attn_bwd_source_compact_f32(const float* d_att, const float* h, const int32_t* node_ptr, const int32_t* slot_dst,
                                                const int32_t* slot_msg, const int32_t* slot_row, const float* coef_a,
                                                const float* coef_s, float* dHc, float* dh, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && D % 4 == 0, "bad sizes V=%d D=%d", V, D);
    if (D > 256) return fail(GGNN_E_UNSUPPORTED, "propagation attention supports hidden sizes up to 256 (got %d)", D);
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(d_att && node_ptr && slot_dst && slot_msg && slot_row && coef_a && dHc, "null pointer");
    GGNN_CHECK_ARG(!dh || (h && coef_s), "h and coef_s are required with dh");
    GGNN_CHECK_ARG(aligned16(d_att) && aligned16(dHc) && (!dh || (aligned16(h) && aligned16(dh))), "pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int D4 = D / 4;
#define GGNN_ATTN_BWD_SOURCE(LPR, NODES)                                                                                       \
    hipLaunchKernelGGL(attn_bwd_source_compact_kernel<LPR>, dim3((V + NODES - 1) / NODES), dim3(256), 0, st, d_att, h,         \
                       node_ptr, slot_dst, slot_msg, slot_row, coef_a, coef_s, dHc, dh, V, D)
    if (D4 <= 16) GGNN_ATTN_BWD_SOURCE(16, 16);
    else if (D4 <= 32) GGNN_ATTN_BWD_SOURCE(32, 8);
    else GGNN_ATTN_BWD_SOURCE(64, 4);
#undef GGNN_ATTN_BWD_SOURCE
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
