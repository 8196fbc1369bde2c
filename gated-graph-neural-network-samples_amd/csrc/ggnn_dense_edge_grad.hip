// Edge-weight and edge-bias gradients of the graph-resident dense training step (what TF autodiff derives from
// chem_tensorflow_dense.py:103-112 through compute_gradients, chem_tensorflow.py:184), on the rows stacked over the timesteps:
//     dW[e][k][n] = sum_rows h[row][k] * dM[row][e*D + n]                       [E, D, D]  (the variable's own layout)
//     db[e][n]    = sum_rows nin[row % rows_per_step][e] * dx[row][n]           [E, D]
// in ONE product launch plus one reduce launch, deterministic (fixed-order sums, no atomics), every product on the f32 MFMA
// (v_mfma_f32_16x16x4_f32: exact-format arithmetic, as every backward product of this library).
//
// What it replaces: ggnn_gemm_tn_f32 twice (h^T dM with ~384 row splits of ~80 rows -> 61 MB of partials summed by 40 000 threads
// with 384 dependent loads each; nin^T dx with K = E = 4 on one wave in four), a nin.repeat(steps, 1) copy and the
// [D, E, D] -> [E, D, D] permute copy.
//
// Decomposition: a workgroup (4 waves) owns ONE edge type e -- the [D, D] block dW[e] -- and one of S row ranges, S chosen so that
// E * S ~ one workgroup per CU (N = 29 696, E = 4: S = 64 ranges of 480 rows -> 9.3 MB of partials instead of 61).  The rows go
// through LDS in double-buffered 32-row slabs (h, dM_e; global -> registers before the slab's MFMAs, registers -> LDS after them,
// one barrier per slab).  Wave w owns the 16-row tiles k = w, w + 4 of dW[e] times all D/16 column tiles.
// The edge biases ride along as one extra A tile: the 16-wide operand is the slab's nin rows (E <= 8 columns, zero-padded), the B
// operand dx.  Workgroup e takes the dx column tiles nt = e, e + E, .. so dx is read once over the E workgroups of a row range; the
// MFMAs go to the wave with the fewest dW tiles.
// The workgroups of one row range read the same h rows: the block index is remapped so that they share an XCD (and its L2) --
// a speed choice only, nothing depends on placement.
// The reduce launch adds the S partials of every output: 64 outputs x 4 quarter-ranges of the splits per workgroup, each quarter
// summed in order, the quarters as (q0 + q1) + (q2 + q3); `accumulate` adds the destination's contents last (one f32 add).
#include "ggnn_common.h"
#include "ggnn_dense_graph.hpp"

namespace ggnn {
namespace {

constexpr int kEgWaves = 4;
constexpr int kEgThreads = kEgWaves * 64;
constexpr int kEgSlab = 32;              // rows per LDS slab (8 MFMA steps)

template <int D>
struct EgCfg {
    static constexpr int NT = (D + 15) / 16;                     // 16-column tiles of a [., D] operand (= 16-row tiles of dW[e])
    static constexpr int KTW = (NT + kEgWaves - 1) / kEgWaves;   // dW row tiles per wave
    static constexpr int P = 16 * NT + 4;                        // LDS pitch of the h / dM slabs (floats)
    static constexpr int NTB = (NT + 1) / 2;                     // dx column tiles per workgroup, at most (E >= 2)
    static constexpr int PX = 16 * NTB + 4;                      // LDS pitch of the dx slab
    static constexpr int F4 = kEgSlab * (P / 4);                 // float4s of one h (or dM) slab
    static constexpr int F4X = kEgSlab * (PX / 4);
    static constexpr int IT = (F4 + kEgThreads - 1) / kEgThreads;
    static constexpr int ITX = (F4X + kEgThreads - 1) / kEgThreads;
    static constexpr int BUF = 2 * kEgSlab * P;                  // floats of one buffer without the bias operands
    static constexpr int BUFB = BUF + kEgSlab * PX + kEgSlab * 8;
};

struct EgArgs {
    const float* h; const float* dM; const float* nin; const float* dx;
    float* part;
    int N, rows_per_step, E, rows_per_split, S;
};

template <int D, bool HAS_B>
__global__ __launch_bounds__(kEgThreads) void dense_edge_grad_kernel(EgArgs a) {
    using C = EgCfg<D>;
    constexpr int NT = C::NT, KTW = C::KTW, P = C::P, NTB = C::NTB, PX = C::PX;
    constexpr int BUFSZ = HAS_B ? C::BUFB : C::BUF;
    extern __shared__ __attribute__((aligned(16))) float lds[];            // [2][h slab | dM slab | dx slab | nin slab]

    // block -> (row range, edge type): the E workgroups of a row range get consecutive slots of one XCD (block b runs on XCD b % 8)
    const int total = a.E * a.S;
    const int per_xcd = gridDim.x / kNumXcd;
    const int w = (blockIdx.x % kNumXcd) * per_xcd + blockIdx.x / kNumXcd;
    if (w >= total) return;
    const int e = w % a.E, split = w / a.E;
    const int E = a.E;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int r_beg = split * a.rows_per_split;
    const int r_end = min(a.N, r_beg + a.rows_per_split);
    const size_t ldm = (size_t)E * D;

    f32x4 acc[KTW][NT];
    f32x4 accb[NTB];
#pragma unroll
    for (int j = 0; j < KTW; ++j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[j][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NTB; ++j) accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- a slab's operands: global -> registers (issued before the MFMAs of the slab in flight), registers -> LDS (after them) ----
    f32x4 ph[C::IT], pm[C::IT], px[C::ITX];
    float pn = 0.f;
    auto fetch = [&](int r0) {
#pragma unroll
        for (int j = 0; j < C::IT; ++j) {
            const int i = tid + j * kEgThreads;
            const int rr = i / (P / 4), c4 = i % (P / 4);
            const int row = r0 + rr;
            const bool ok = i < C::F4 && row < r_end && 4 * c4 < D;      // (zero beyond the rows of the range and the D columns)
            ph[j] = ok ? *reinterpret_cast<const f32x4*>(a.h + (size_t)row * D + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
            pm[j] = ok ? *reinterpret_cast<const f32x4*>(a.dM + (size_t)row * ldm + (size_t)e * D + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (HAS_B) {
#pragma unroll
            for (int j = 0; j < C::ITX; ++j) {
                const int i = tid + j * kEgThreads;
                const int rr = i / (PX / 4), c4 = i % (PX / 4);
                const int row = r0 + rr;
                const int nt = e + (c4 / 4) * E;                         // slab tile c4 / 4 holds dx column tile e + (c4 / 4) E
                const int n = 16 * nt + 4 * (c4 % 4);
                const bool ok = i < C::F4X && row < r_end && c4 / 4 < NTB && nt < NT && n < D;
                px[j] = ok ? *reinterpret_cast<const f32x4*>(a.dx + (size_t)row * D + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const int rr = tid >> 3, c = tid & 7, row = r0 + rr;         // kEgSlab * 8 == kEgThreads: one in-degree per thread
            pn = (row < r_end && c < E) ? a.nin[(size_t)(row % a.rows_per_step) * E + c] : 0.f;
        }
    };
    auto commit = [&](int buf) {
        float* hs = lds + buf * BUFSZ;
        float* ms = hs + kEgSlab * P;
#pragma unroll
        for (int j = 0; j < C::IT; ++j) {
            const int i = tid + j * kEgThreads;
            if (i < C::F4) {
                const int rr = i / (P / 4), c4 = i % (P / 4);
                *reinterpret_cast<f32x4*>(hs + rr * P + 4 * c4) = ph[j];
                *reinterpret_cast<f32x4*>(ms + rr * P + 4 * c4) = pm[j];
            }
        }
        if constexpr (HAS_B) {
            float* xs = ms + kEgSlab * P;
            float* ns = xs + kEgSlab * PX;
#pragma unroll
            for (int j = 0; j < C::ITX; ++j) {
                const int i = tid + j * kEgThreads;
                if (i < C::F4X) {
                    const int rr = i / (PX / 4), c4 = i % (PX / 4);
                    *reinterpret_cast<f32x4*>(xs + rr * PX + 4 * c4) = px[j];
                }
            }
            ns[tid] = pn;
        }
    };

    int buf = 0;
    fetch(r_beg);
    commit(0);
    __syncthreads();
    for (int r0 = r_beg; r0 < r_end; r0 += kEgSlab) {
        const bool more = r0 + kEgSlab < r_end;
        if (more) fetch(r0 + kEgSlab);
        const float* hs = lds + buf * BUFSZ;
        const float* ms = hs + kEgSlab * P;
#pragma unroll
        for (int s = 0; s < kEgSlab / 4; ++s) {
            const int row = 4 * s + kq;
            // lane (li, kq): A operand = h[row][16 kt + li], B operand = dM_e[row][16 nt + li]; the accumulator of tile (kt, nt)
            // holds dW[e][16 kt + 4 kq + j][16 nt + li], j = 0..3
            float b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = ms[row * P + 16 * nt + li];
#pragma unroll
            for (int j = 0; j < KTW; ++j) {
                const int kt = wave + j * kEgWaves;
                if (kt < NT) {                                              // (wave-uniform)
                    const float av = hs[row * P + 16 * kt + li];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[j][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[nt], acc[j][nt], 0, 0, 0);
                }
            }
            if constexpr (HAS_B) {
                if (wave == kEgWaves - 1) {                                 // the wave with the fewest dW tiles
                    const float* xs = ms + kEgSlab * P;
                    const float* ns = xs + kEgSlab * PX;
                    const float nv = ns[row * 8 + (li & 7)];
                    const float an = li < 8 ? nv : 0.f;                     // A operand: nin[row][li], E <= 8 columns zero-padded
#pragma unroll
                    for (int j = 0; j < NTB; ++j)
                        if (e + j * E < NT)
                            accb[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(an, xs[row * PX + 16 * j + li], accb[j], 0, 0, 0);
                }
            }
        }
        if (more) commit(buf ^ 1);
        __syncthreads();                                                    // slab[buf] consumed, slab[buf ^ 1] written
        buf ^= 1;
    }

    // ---- this range's partial: [E][D][D] followed by [E][D] per split; every element is written by exactly one workgroup ----------
    const size_t per_split = (size_t)E * D * D + (size_t)E * D;
    float* out = a.part + (size_t)split * per_split;
    float* outw = out + (size_t)e * D * D;
#pragma unroll
    for (int j = 0; j < KTW; ++j) {
        const int kt = wave + j * kEgWaves;
        if (kt < NT) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = 16 * nt + li;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = 16 * kt + 4 * kq + q;
                    if (k < D && n < D) outw[(size_t)k * D + n] = acc[j][nt][q];
                }
            }
        }
    }
    if constexpr (HAS_B) {
        if (wave == kEgWaves - 1) {
            float* outb = out + (size_t)E * D * D;
#pragma unroll
            for (int j = 0; j < NTB; ++j) {
                const int nt = e + j * E, n = 16 * nt + li;
                if (nt < NT && n < D) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int eb = 4 * kq + q;                          // accumulator row = edge type
                        if (eb < E) outb[(size_t)eb * D + n] = accb[j][q];
                    }
                }
            }
        }
    }
}

// dst[o] (+)= sum over the S partials: thread (q, i) adds quarter q of the splits of output 64 blockIdx + i, in order
__global__ __launch_bounds__(256) void dense_edge_grad_reduce_kernel(const float* __restrict__ part, size_t per_split, int S, int nw, int nout,
                                                                     float* __restrict__ dW, float* __restrict__ db, int accumulate) {
    __shared__ float sums[4][64];
    const int i = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int o = blockIdx.x * 64 + i;
    const int chunk = (S + 3) / 4;
    const int p_beg = q * chunk, p_end = min(S, p_beg + chunk);
    float s = 0.f;
    if (o < nout)
        for (int p = p_beg; p < p_end; ++p) s += part[(size_t)p * per_split + o];
    sums[q][i] = s;
    __syncthreads();
    if (q == 0 && o < nout) {
        const float v = (sums[0][i] + sums[1][i]) + (sums[2][i] + sums[3][i]);
        float* dst = o < nw ? dW + o : db + (o - nw);
        *dst = accumulate ? *dst + v : v;
    }
}

bool edge_grad_shape_ok(int E, int D) { return (D == 32 || D == 64 || D == 100) && (E == 2 || E == 4 || E == 6 || E == 8); }

// upper bound of the number of row ranges: E * S ~ one workgroup per CU, at least two slabs per range (non-decreasing in N: the
// workspace is sized by it)
int edge_grad_max_splits(int N, int E) {
    int s = (num_cus() + E - 1) / E;
    const int max_s = (N + 2 * kEgSlab - 1) / (2 * kEgSlab);
    if (s > max_s) s = max_s;
    return s < 1 ? 1 : s;
}

// -> rows per range (a multiple of the slab) and the number of ranges S <= edge_grad_max_splits
void edge_grad_splits(int N, int E, int* rows_per_split, int* S) {
    const int s = edge_grad_max_splits(N, E);
    int rows = (N + s - 1) / s;
    rows = (rows + kEgSlab - 1) / kEgSlab * kEgSlab;
    if (rows < kEgSlab) rows = kEgSlab;
    *rows_per_split = rows;
    *S = N > 0 ? (N + rows - 1) / rows : 1;                          // (every range holds at least one row)
}

template <int D, bool HAS_B>
int launch_edge_grad(const EgArgs& a, hipStream_t st) {
    using C = EgCfg<D>;
    const size_t ldsb = (size_t)2 * (HAS_B ? C::BUFB : C::BUF) * sizeof(float);
    static std::atomic<unsigned long long> lds_ok{0};
    if (ldsb > 64 * 1024) GGNN_CHECK_HIP((allow_dynamic_lds(&dense_edge_grad_kernel<D, HAS_B>, ldsb, lds_ok)));
    const int blocks = (a.E * a.S + kNumXcd - 1) / kNumXcd * kNumXcd;
    hipLaunchKernelGGL((dense_edge_grad_kernel<D, HAS_B>), dim3(blocks), dim3(kEgThreads), ldsb, st, a);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" size_t ggnn_dense_edge_grad_workspace_bytes(int N, int E, int D) {
    if (N <= 0 || !edge_grad_shape_ok(E, D)) return 256;
    return (size_t)edge_grad_max_splits(N, E) * ((size_t)E * D * D + (size_t)E * D) * sizeof(float) + 256;
}

extern "C" int ggnn_dense_edge_grad_f32(const float* h, const float* dM, const float* nin, const float* dx, int N, int rows_per_step,
                                        int E, int D, float* dW, float* db, int accumulate, void* ws, size_t ws_bytes,
                                        ggnn_stream_t stream) {
    GGNN_CHECK_ARG(N >= 0, "bad size N=%d", N);
    if (!edge_grad_shape_ok(E, D))
        return fail(GGNN_E_UNSUPPORTED, "dense edge gradients: unsupported shape E=%d D=%d (hidden size 32/64/100, E in {2,4,6,8})", E, D);
    GGNN_CHECK_ARG(dW && aligned16(dW), "null or misaligned pointer (dW)");
    GGNN_CHECK_ARG(!nin || (db && aligned16(db) && rows_per_step >= 1), "edge biases: nin needs db (16-byte aligned) and rows_per_step >= 1 (got %d)",
                   rows_per_step);
    hipStream_t st = (hipStream_t)stream;
    const size_t nw = (size_t)E * D * D, nb = nin ? (size_t)E * D : 0;
    if (N == 0) {                                                       // an empty sum: zeros, or nothing to add
        if (!accumulate) {
            GGNN_CHECK_HIP(hipMemsetAsync(dW, 0, nw * sizeof(float), st));
            if (nb) GGNN_CHECK_HIP(hipMemsetAsync(db, 0, nb * sizeof(float), st));
        }
        return GGNN_OK;
    }
    GGNN_CHECK_ARG(h && dM && ws && aligned16(h) && aligned16(dM) && aligned16(ws) && (!nin || (dx && aligned16(dx))), "null or misaligned pointer");
    const size_t need = ggnn_dense_edge_grad_workspace_bytes(N, E, D);
    if (ws_bytes < need) return fail(GGNN_E_WORKSPACE, "dense edge gradients: workspace too small: %zu < %zu", ws_bytes, need);
    EgArgs a{h, dM, nin, dx, static_cast<float*>(ws), N, nin ? rows_per_step : 1, E, 0, 0};
    edge_grad_splits(N, E, &a.rows_per_split, &a.S);
    const int rc = dense_for_D(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        return nin ? launch_edge_grad<DD, true>(a, st) : launch_edge_grad<DD, false>(a, st); });
    if (rc) return rc;
    // without edge biases the partials' [E][D] tails are never written and never read: the reduce covers the [E][D][D] heads only
    const int nout = (int)(nw + nb);
    hipLaunchKernelGGL(dense_edge_grad_reduce_kernel, dim3((nout + 63) / 64), dim3(256), 0, st, (const float*)a.part,
                       nw + (size_t)E * D, a.S, (int)nw, nout, dW, db, accumulate ? 1 : 0);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
