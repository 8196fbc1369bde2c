// BasicRNNCell (chem_tensorflow_sparse.py:109-110, 198-216) with the segment sum gathered inside, in one launch:
//
//     incoming[v] = (sum over slots row_ptr[v] .. row_ptr[v+1] of Hrows[gather_row[slot]]) / (sum_t nin[v,t] + 1e-7)
//     h'          = act([x_0 | .. | x_{nx-2} | incoming | h] W + b)          W [(nx+1) D, D], act = tanh / ReLU
//
// The R-GCN configuration of the sparse GGNN (graph_rnn_cell = RNN) runs this once per timestep behind the compacted message
// transform: the separate segment-sum launch and the HBM round trip of `incoming` are gone, and W is not re-staged per call.
//
// Structure: that of the fused GCN layer (ggnn_gcn.hip).  A workgroup brings ALL nx + 1 weight blocks [D, D] into LDS once, as
// exact bf16x3 stage images (LDS-DMA), then each wave walks over 16-row tiles.  Per tile a lane builds its part of the gathered
// segment in registers -- sum from 0 in slot order, the degree as the sequential sum over t, a plain division: the arithmetic of
// ggnn_gather_segment_sum_f32 without bias, bit for bit -- and multiplies the segments one after the other into one accumulator
// set: incoming first, then the residual segments, then h.  The epilogue is EpiBiasAct's (bias, tanh_f or fmaxf) and a store.
// Training form: the gathered segment is also written to save_incoming [V, D] (an operand of dW); h' does not depend on it.
//
// The cell's backward (dP, dx / d_incoming / dh from g and h') is the second kernel of this file, on the same configuration: see
// "the backward of the cell in one launch" below.
//
// Exact format only: ReLU states have no bound, so the two-piece f16 format's operand range cannot be proven for this cell.
//
// LDS and occupancy.  An image is 8 KiB at D = 32, 24 KiB at D = 64, 72 KiB at D = 100, and all nx + 1 are resident, so the
// supported set is what fits the 160 KiB of a CU: D = 32 / 64 with nx = 1 .. 3 (16 .. 96 KiB) and D = 100 with nx = 1 (144 KiB).
// The kernel is bounded to 128 registers (4 waves per SIMD = 16 per CU).  Up to 80 KiB two workgroups of 8 waves share a CU;
// beyond (D = 64 / nx = 3, D = 100 / nx = 1) only one workgroup fits, and it is the wave count of THAT workgroup which sets the
// occupancy: it runs 16 waves.
//
// Addressing is defensive: rows >= V are neither read nor written (their lanes read row V - 1 and store nothing), row_ptr values
// are clamped to [0, M], and a gather_row outside [0, num_rows) adds nothing and is not dereferenced (the lane fetches row 0 and
// selects 0).  32-bit byte offsets: V * D and num_rows * D must stay below 2^30 (the entry point refuses larger calls).
#include "ggnn_split.hpp"
#include <algorithm>

namespace ggnn {
namespace {

template <int D>
using RnnImg = SplitCfg<D, kSplitBf16x3>;

constexpr int kRnnDmaWaves = 8;                        // the waves that issue the image DMA (an image is whole KiB per 8 waves)

// one workgroup per CU (more than 80 KiB of images): 16 waves; otherwise two workgroups of 8
template <int D, int NX>
struct RnnCfg {
    static constexpr int LDS = (NX + 1) * RnnImg<D>::IMG_BYTES;
    static constexpr bool FITS = LDS <= 160 * 1024;
    static constexpr int WG_PER_CU = LDS <= 80 * 1024 ? 2 : 1;
    static constexpr int NW = WG_PER_CU == 2 ? 8 : 16;
};

struct RnnFusedArgs {
    const float* x[2];                                 // residual segments (nx - 1 of them)
    const float* h;
    const float* packed;                               // nx + 1 images, IMG_BYTES apart
    const float* b;
    float* h_out;
    const float* H;                                    // [num_rows, D]
    const int* row_ptr;
    const int* gidx;
    const float* nin;
    float* save;                                       // null or [V, D]
    int num_rows, M, T, use_avg, V, act;
};

// f += ok ? t : 0   (slot order; an invalid slot adds nothing)
template <int D>
__device__ __forceinline__ void frag_add(Frag<D>& f, const Frag<D>& t, bool ok) {
#pragma unroll
    for (int c = 0; c < StageCfg<D>::NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) f.v[c][e] += ok ? t.v[c][e] : 0.f;
#pragma unroll
    for (int q = 0; q < StageCfg<D>::NR; ++q) f.r[q] += ok ? t.r[q] : 0.f;
}

template <int D>
__global__ void rnn_pack_kernel(const float* __restrict__ W, float* __restrict__ packed) {
    const int s = blockIdx.y;                          // K segment: rows s D .. of W
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    pack_split_image<D, kSplitBf16x3>(StageValue<D>{W, s * D, 0, D, -1, nullptr, 0, 0, -1}, packed + (size_t)s * RnnImg<D>::IMG, first, stride);
}

template <int D, int NX>
__global__ __launch_bounds__((RnnCfg<D, NX>::NW * 64), 4) /* <= 128 VGPRs */ void rnn_fused_kernel(RnnFusedArgs a) {
    using S = StageCfg<D>;
    using I = RnnImg<D>;
    constexpr int NT = S::NT, NW = RnnCfg<D, NX>::NW;
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V;
    const int n_tiles = (V + 15) / 16;
    const int stride = gridDim.x * NW;

    if (wave < kRnnDmaWaves) dma_image_asm<(NX + 1) * I::IMG_BYTES, kRnnDmaWaves>(a.packed, img, wave, lane);
    dma_wait();
    __syncthreads();                                        // the images have landed

    for (int idx = blockIdx.x * NW + wave; idx < n_tiles; idx += stride) {
        const int r = idx * 16 + li;
        const bool live = r < V;
        const int rc = live ? r : V - 1;                    // (a row of its own for every lane: nothing beyond V is read)
        int beg = 0, end = 0;
        if (live) {
            beg = min(max(a.row_ptr[r], 0), a.M);
            end = min(max(a.row_ptr[r + 1], beg), a.M);
        }
        Frag<D> hf;
        load_frag<D>(hf, a.h, rc, kq);                      // independent of the gather's dependent loads: in flight beside them

        Frag<D> g;
#pragma unroll
        for (int c = 0; c < S::NC; ++c) g.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < S::NR; ++q) g.r[q] = 0.f;
        // two gathered rows in flight per iteration; the sum stays in slot order
        int k = beg;
        for (; k + 1 < end; k += 2) {
            const int j0 = a.gidx[k], j1 = a.gidx[k + 1];
            const bool ok0 = (unsigned)j0 < (unsigned)a.num_rows, ok1 = (unsigned)j1 < (unsigned)a.num_rows;
            Frag<D> t0, t1;
            load_frag<D>(t0, a.H, ok0 ? j0 : 0, kq);
            load_frag<D>(t1, a.H, ok1 ? j1 : 0, kq);
            frag_add<D>(g, t0, ok0);
            frag_add<D>(g, t1, ok1);
        }
        if (k < end) {
            const int j0 = a.gidx[k];
            const bool ok0 = (unsigned)j0 < (unsigned)a.num_rows;
            Frag<D> t0;
            load_frag<D>(t0, a.H, ok0 ? j0 : 0, kq);
            frag_add<D>(g, t0, ok0);
        }
        if (a.use_avg) {                                    // :206-209, the expression of the stand-alone segment sum
            float deg = 0.f;
            for (int t = 0; t < a.T; ++t) deg += a.nin[(size_t)rc * a.T + t];
            const float den = deg + 1e-7f;
#pragma unroll
            for (int c = 0; c < S::NC; ++c) g.v[c] = g.v[c] / den;
#pragma unroll
            for (int q = 0; q < S::NR; ++q) g.r[q] = g.r[q] / den;
        }
        if (a.save && live) {
            const unsigned ob = ((unsigned)r * (unsigned)D + 4u * (unsigned)kq) * 4u;
#pragma unroll
            for (int c = 0; c < S::NC; ++c) st4_b(a.save, ob + 64u * c, g.v[c]);
#pragma unroll
            for (int q = 0; q < S::NR; ++q) a.save[(size_t)r * D + 16 * S::NC + 4 * q + kq] = g.r[q];
        }

        // [x_0 | .. | incoming | h] W: image s holds rows s D .. of W; incoming is segment NX - 1, h segment NX
        f32x4 acc[NT];
        SFrag<D> sf;
        split_frag<D, kSplitBf16x3>(sf, g);
        stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc, sf, g, img + (NX - 1) * I::IMG, li, kq);
#pragma unroll
        for (int s = 0; s + 1 < NX; ++s) {
            Frag<D> xf;
            load_frag<D>(xf, a.x[s], rc, kq);
            split_frag<D, kSplitBf16x3>(sf, xf);
            stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc, sf, xf, img + s * I::IMG, li, kq);
        }
        split_frag<D, kSplitBf16x3>(sf, hf);
        stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc, sf, hf, img + NX * I::IMG, li, kq);

        if (live) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c0 = nt * 16 + 4 * kq;
                if (c0 < D) {
                    f32x4 c = acc[nt] + ld4(a.b + c0);       // EpiBiasAct, term for term
                    if (a.act == GGNN_ACT_TANH) { c.x = tanh_f(c.x); c.y = tanh_f(c.y); c.z = tanh_f(c.z); c.w = tanh_f(c.w); }
                    else { c.x = fmaxf(c.x, 0.f); c.y = fmaxf(c.y, 0.f); c.z = fmaxf(c.z, 0.f); c.w = fmaxf(c.w, 0.f); }
                    st4_b(a.h_out, ((unsigned)r * (unsigned)D + c0) * 4u, c);
                }
            }
        }
    }
}

template <int D, int NX>
int rnn_launch(const RnnFusedArgs& a, hipStream_t st) {
    using C = RnnCfg<D, NX>;
    static_assert(C::FITS, "the resident images must fit a CU's LDS");
    static std::atomic<unsigned long long> lds_ok{0};
    if (C::LDS > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&rnn_fused_kernel<D, NX>, C::LDS, lds_ok));
    const long long n_tiles = (a.V + 15) / 16;
    const long long blocks = std::min<long long>((n_tiles + C::NW - 1) / C::NW, (long long)C::WG_PER_CU * num_cus());
    hipLaunchKernelGGL((rnn_fused_kernel<D, NX>), dim3((unsigned)blocks), dim3(C::NW * 64), C::LDS, st, a);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D>
int rnn_pack(const float* W, int nx, float* packed, hipStream_t st) {
    hipLaunchKernelGGL((rnn_pack_kernel<D>), dim3(16, (unsigned)(nx + 1)), dim3(256), 0, st, W, packed);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

// calls f(RnnCfg<D, nx>{}) for a supported (D, nx); false otherwise
template <class F>
bool rnn_with_cfg(int D, int nx, F&& f) {
    switch (D * 4 + nx) {
        case 32 * 4 + 1: f(RnnCfg<32, 1>{}); return true;
        case 32 * 4 + 2: f(RnnCfg<32, 2>{}); return true;
        case 32 * 4 + 3: f(RnnCfg<32, 3>{}); return true;
        case 64 * 4 + 1: f(RnnCfg<64, 1>{}); return true;
        case 64 * 4 + 2: f(RnnCfg<64, 2>{}); return true;
        case 64 * 4 + 3: f(RnnCfg<64, 3>{}); return true;
        case 100 * 4 + 1: f(RnnCfg<100, 1>{}); return true;
        default: return false;
    }
}

int rnn_dispatch(const RnnFusedArgs& a, int D, int nx, hipStream_t st) {
    switch (D * 4 + nx) {
        case 32 * 4 + 1: return rnn_launch<32, 1>(a, st);
        case 32 * 4 + 2: return rnn_launch<32, 2>(a, st);
        case 32 * 4 + 3: return rnn_launch<32, 3>(a, st);
        case 64 * 4 + 1: return rnn_launch<64, 1>(a, st);
        case 64 * 4 + 2: return rnn_launch<64, 2>(a, st);
        case 64 * 4 + 3: return rnn_launch<64, 3>(a, st);
        default: return rnn_launch<100, 1>(a, st);
    }
}


// ---- the backward of the cell in one launch ------------------------------------------------------------------------------------------
// From g = dL/dh' and the saved output out = h' (chem_tensorflow_sparse.py:109-110 under autodiff):
//
//     g_eff = g [+ the rows of Z named by the node's slot-head record]         (the deferred node sum of the transform backward)
//     dP    = g_eff * act'(out)                    tanh: 1 - out^2;  ReLU: out > 0        (ggnn_act_bwd_f32's expressions)
//     Q_s   = dP W_s^T                             s = 0 .. nx,  W_s = rows s D .. of W
//     dx[s] = Q_s (s < nx - 1);   dinc = Q_{nx-1} [/ (sum_t nin[v,t] + 1e-7)];   dh = Q_nx
//
// The mirror image of the forward kernel above: the nx + 1 TRANSPOSED blocks are resident in LDS as exact bf16x3 images, a wave
// walks 16-row tiles, dP is built once per tile in registers (and written: it is the dY of the weight-gradient product), split
// once, and its planes serve all nx + 1 products, each into a fresh accumulator set that is stored as soon as it is complete.
// The same RnnCfg, so the same supported set, LDS budget and occupancy rule; the same defensive addressing.
struct RnnBwdArgs {
    const float* g;
    const float* out;
    const float* packed;                               // nx + 1 images of W_s^T, IMG_BYTES apart
    const float* gz;                                   // null, or [num_rows, D]
    const int* gz_heads;                               // [V] int4 slot-head records
    const float* nin;
    float* dP;
    float* q[4];                                       // destination of Q_s: dx[0 .. nx-2], dinc, dh
    int num_rows, T, use_avg, V, act;
};

template <int D>
__global__ void rnn_bwd_pack_kernel(const float* __restrict__ W, float* __restrict__ packed) {
    const int s = blockIdx.y;                          // image s: B(k, n) = W[s D + n][k]
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    pack_split_image<D, kSplitBf16x3>(StageValueT<D>{W, s * D, 0, D}, packed + (size_t)s * RnnImg<D>::IMG, first, stride);
}

template <int D, int NX, bool GATHER>
__global__ __launch_bounds__((RnnCfg<D, NX>::NW * 64), 4) /* <= 128 VGPRs */ void rnn_bwd_fused_kernel(RnnBwdArgs a) {
    using S = StageCfg<D>;
    using I = RnnImg<D>;
    constexpr int NT = S::NT, NW = RnnCfg<D, NX>::NW;
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V;
    const int n_tiles = (V + 15) / 16;
    const int stride = gridDim.x * NW;

    if (wave < kRnnDmaWaves) dma_image_asm<(NX + 1) * I::IMG_BYTES, kRnnDmaWaves>(a.packed, img, wave, lane);
    dma_wait();
    __syncthreads();                                        // the images have landed

    for (int idx = blockIdx.x * NW + wave; idx < n_tiles; idx += stride) {
        const int r = idx * 16 + li;
        const bool live = r < V;
        const int rc = live ? r : V - 1;                    // (a row of its own for every lane: nothing beyond V is read)
        Frag<D> gf, of;
        if constexpr (GATHER) {
            // the sums of ggnn_gather_segment_sum_heads_f32(accumulate = 1), in its order: (((0 + z0) + z1) + z2 + z3) + g.  The
            // head record first: it starts the dependent chain record -> rows.  Two rows in flight; slots 2, 3 exist for few
            // nodes (three or more edge types): a second round that most tiles skip as a wave
            const int4 hd = *reinterpret_cast<const int4*>(a.gz_heads + 4 * (size_t)rc);
            load_frag<D>(gf, a.g, rc, kq);
            const bool ok0 = (unsigned)hd.x < (unsigned)a.num_rows, ok1 = (unsigned)hd.y < (unsigned)a.num_rows;
            const bool ok2 = (unsigned)hd.z < (unsigned)a.num_rows, ok3 = (unsigned)hd.w < (unsigned)a.num_rows;
            Frag<D> z0, z1, zs;
#pragma unroll
            for (int c = 0; c < S::NC; ++c) zs.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < S::NR; ++q) zs.r[q] = 0.f;
            // (a slot that names no row fetches row 0 and selects 0, like the forward's gather: nothing outside gz is dereferenced)
            load_frag<D>(z0, a.gz, ok0 ? hd.x : 0, kq);
            load_frag<D>(z1, a.gz, ok1 ? hd.y : 0, kq);
            frag_add<D>(zs, z0, ok0);
            frag_add<D>(zs, z1, ok1);
            if (ok2 || ok3) {
                load_frag<D>(z0, a.gz, ok2 ? hd.z : 0, kq);
                load_frag<D>(z1, a.gz, ok3 ? hd.w : 0, kq);
                frag_add<D>(zs, z0, ok2);
                frag_add<D>(zs, z1, ok3);
            }
#pragma unroll
            for (int c = 0; c < S::NC; ++c) gf.v[c] = zs.v[c] + gf.v[c];
#pragma unroll
            for (int q = 0; q < S::NR; ++q) gf.r[q] = zs.r[q] + gf.r[q];
            // (out only now: with it in flight beside g, the sum and two rows, D = 100 needs 168 B of scratch per lane)
            __builtin_amdgcn_sched_barrier(0);
            load_frag<D>(of, a.out, rc, kq);
        } else {
            load_frag<D>(gf, a.g, rc, kq);
            load_frag<D>(of, a.out, rc, kq);
        }

        // dP in place of g: act_bwd_kernel's expressions, term for term
        if (a.act == GGNN_ACT_TANH) {
#pragma unroll
            for (int c = 0; c < S::NC; ++c) gf.v[c] = gf.v[c] * (1.0f - of.v[c] * of.v[c]);
#pragma unroll
            for (int q = 0; q < S::NR; ++q) gf.r[q] = gf.r[q] * (1.0f - of.r[q] * of.r[q]);
        } else {
#pragma unroll
            for (int c = 0; c < S::NC; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) gf.v[c][e] = of.v[c][e] > 0.f ? gf.v[c][e] : 0.f;
#pragma unroll
            for (int q = 0; q < S::NR; ++q) gf.r[q] = of.r[q] > 0.f ? gf.r[q] : 0.f;
        }
        if (live) {
            const unsigned ob = ((unsigned)r * (unsigned)D + 4u * (unsigned)kq) * 4u;
#pragma unroll
            for (int c = 0; c < S::NC; ++c) st4_b(a.dP, ob + 64u * c, gf.v[c]);
#pragma unroll
            for (int q = 0; q < S::NR; ++q) a.dP[(size_t)r * D + 16 * S::NC + 4 * q + kq] = gf.r[q];
        }
        float den = 1.0f;
        if (a.use_avg) {                                    // :206-209 under autodiff, the expression of ggnn_bwd_dx_f32
            float deg = 0.f;
            for (int t = 0; t < a.T; ++t) deg += a.nin[(size_t)rc * a.T + t];
            den = deg + 1e-7f;
        }

        // Eight of the nine piece products instead of the format's six.  A split product drops w_mid a_lo, w_lo a_mid and w_lo a_lo;
        // the pieces are truncations, so every dropped term has the sign of its product and the result is short by ~2^-25 of
        // sum |dP| |W| -- inside the project's product bound for one launch, but the same sign in every timestep: over the eight
        // layers of the README configuration layer 0's gradients came out 4e-7 (normwise) from the autograd route's, whose
        // ggnn_bwd_dx_f32 is an f32 MFMA, against 2e-7 of that route's own distance from float64.  Two calls on re-arranged planes
        // give all but w_lo a_lo (2^-32): {mid, lo, 0} -> w_lo a_mid + w_mid a_lo + w_mid a_mid + w_hi a_lo + w_hi a_mid, then
        // {hi, 0, 0} -> (w_lo + w_mid + w_hi) a_hi, smallest terms first; the D % 16 remainder columns (f32 MFMA) ride in the second.
        SFrag<D> sf, sa;
        split_frag<D, kSplitBf16x3>(sf, gf);
        Frag<D> zf;
#pragma unroll
        for (int c = 0; c < S::NC; ++c) zf.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < S::NR; ++q) zf.r[q] = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < SplitCfg<D>::NC2; ++c2) {
            sa.hi[c2] = sf.hi[c2]; sa.mid[c2] = u32x4{0u, 0u, 0u, 0u}; sa.lo[c2] = u32x4{0u, 0u, 0u, 0u};
            sf.hi[c2] = sf.mid[c2]; sf.mid[c2] = sf.lo[c2]; sf.lo[c2] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int s = 0; s <= NX; ++s) {
            f32x4 acc[NT];
            stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc, sf, zf, img + s * I::IMG, li, kq);
            stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc, sa, gf, img + s * I::IMG, li, kq);
            if (live) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int c0 = nt * 16 + 4 * kq;
                    if (c0 < D) {
                        f32x4 v = acc[nt];
                        if (s == NX - 1 && a.use_avg) v = v / den;
                        st4_b(a.q[s], ((unsigned)r * (unsigned)D + c0) * 4u, v);
                    }
                }
            }
        }
    }
}

template <int D, int NX>
int rnn_bwd_launch(const RnnBwdArgs& a, hipStream_t st) {
    using C = RnnCfg<D, NX>;
    static_assert(C::FITS, "the resident images must fit a CU's LDS");
    const long long n_tiles = (a.V + 15) / 16;
    const long long blocks = std::min<long long>((n_tiles + C::NW - 1) / C::NW, (long long)C::WG_PER_CU * num_cus());
    if (a.gz) {
        static std::atomic<unsigned long long> lds_ok{0};
        if (C::LDS > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&rnn_bwd_fused_kernel<D, NX, true>, C::LDS, lds_ok));
        hipLaunchKernelGGL((rnn_bwd_fused_kernel<D, NX, true>), dim3((unsigned)blocks), dim3(C::NW * 64), C::LDS, st, a);
    } else {
        static std::atomic<unsigned long long> lds_ok{0};
        if (C::LDS > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&rnn_bwd_fused_kernel<D, NX, false>, C::LDS, lds_ok));
        hipLaunchKernelGGL((rnn_bwd_fused_kernel<D, NX, false>), dim3((unsigned)blocks), dim3(C::NW * 64), C::LDS, st, a);
    }
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D>
int rnn_bwd_pack(const float* W, int nx, float* packed, hipStream_t st) {
    hipLaunchKernelGGL((rnn_bwd_pack_kernel<D>), dim3(16, (unsigned)(nx + 1)), dim3(256), 0, st, W, packed);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

int rnn_bwd_dispatch(const RnnBwdArgs& a, int D, int nx, hipStream_t st) {
    switch (D * 4 + nx) {
        case 32 * 4 + 1: return rnn_bwd_launch<32, 1>(a, st);
        case 32 * 4 + 2: return rnn_bwd_launch<32, 2>(a, st);
        case 32 * 4 + 3: return rnn_bwd_launch<32, 3>(a, st);
        case 64 * 4 + 1: return rnn_bwd_launch<64, 1>(a, st);
        case 64 * 4 + 2: return rnn_bwd_launch<64, 2>(a, st);
        case 64 * 4 + 3: return rnn_bwd_launch<64, 3>(a, st);
        default: return rnn_bwd_launch<100, 1>(a, st);
    }
}

int rnn_bwd_impl(const float* g, const float* gz, const int32_t* gz_heads, int64_t num_rows, const float* out, const float* packed,
                 float* dP, float* const* dx, float* dh, const float* nin, int T, int use_avg, int nx, int V, int D, int act,
                 ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && num_rows >= 0, "bad sizes V=%d D=%d rows=%lld", V, D, (long long)num_rows);
    GGNN_CHECK_ARG(act == GGNN_ACT_TANH || act == GGNN_ACT_RELU, "unknown activation %d", act);
    if (!ggnn_rnn_fused_supported(D, nx))
        return fail(GGNN_E_UNSUPPORTED, "fused RNN cell backward supports D = 32, 64 with nx = 1..3 and D = 100 with nx = 1 (got D=%d nx=%d)", D, nx);
    if ((unsigned long long)V * D >= (1ULL << 30) || (unsigned long long)num_rows * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "V*D and num_rows*D must be < 2^30 (32-bit byte offsets)");
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(g && out && packed && dP && dx && dh, "null pointer");
    GGNN_CHECK_ARG(!use_avg || (nin && T > 0), "nin [V, T] is required for mean aggregation");
    GGNN_CHECK_ARG(aligned16(g) && aligned16(out) && aligned16(packed) && aligned16(dP) && aligned16(dh), "pointers must be 16-byte aligned");
    RnnBwdArgs a{};
    float* outputs[5] = {dP, dh, nullptr, nullptr, nullptr};
    for (int s = 0; s < nx; ++s) {
        GGNN_CHECK_ARG(dx[s] && aligned16(dx[s]), "dx[%d] null or misaligned", s);
        a.q[s] = dx[s];
        outputs[2 + s] = dx[s];
    }
    a.q[nx] = dh;
    const void* inputs[6] = {g, out, packed, gz, gz_heads, nin};
    for (int i = 0; i < 2 + nx; ++i) {
        for (const void* in : inputs) GGNN_CHECK_ARG(!in || (const void*)outputs[i] != in, "an output aliases an input");
        for (int j = 0; j < i; ++j) GGNN_CHECK_ARG(outputs[i] != outputs[j], "two outputs alias each other");
    }
    if (num_rows == 0) gz = nullptr;                        // no rows to gather from: the plain form
    a.g = g; a.out = out; a.packed = packed; a.gz = gz; a.gz_heads = gz_heads; a.nin = nin; a.dP = dP;
    a.num_rows = (int)num_rows; a.T = T; a.use_avg = use_avg ? 1 : 0; a.V = V; a.act = act;
    return rnn_bwd_dispatch(a, D, nx, (hipStream_t)stream);
}

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_rnn_fused_supported(int D, int nx) {
    if (nx < 1 || nx > 3) return 0;
    return (D == 32 || D == 64 || (D == 100 && nx == 1)) ? 1 : 0;
}

extern "C" size_t ggnn_rnn_packed_bytes(int D, int nx) {
    if (!ggnn_rnn_fused_supported(D, nx)) return 0;
    size_t bytes = 0;
    rnn_with_cfg(D, nx, [&](auto c) { bytes = (size_t)decltype(c)::LDS; });
    return bytes;
}

extern "C" void ggnn_rnn_fused_launch_geometry(int D, int nx, int* rows_per_workgroup, int* max_workgroups) {
    int rows = 0, wgs = 0;
    if (ggnn_rnn_fused_supported(D, nx))
        rnn_with_cfg(D, nx, [&](auto c) { rows = decltype(c)::NW * 16; wgs = decltype(c)::WG_PER_CU * num_cus(); });
    if (rows_per_workgroup) *rows_per_workgroup = rows;
    if (max_workgroups) *max_workgroups = wgs;
}

extern "C" int ggnn_rnn_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream) {
    if (!ggnn_rnn_fused_supported(D, nx))
        return fail(GGNN_E_UNSUPPORTED, "fused RNN cell supports D = 32, 64 with nx = 1..3 and D = 100 with nx = 1 (got D=%d nx=%d)", D, nx);
    GGNN_CHECK_ARG(W && packed && aligned16(packed) && (const void*)W != (const void*)packed, "null, misaligned or aliasing pointer");
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return rnn_pack<100>(W, nx, packed, st);
        case 64: return rnn_pack<64>(W, nx, packed, st);
        default: return rnn_pack<32>(W, nx, packed, st);
    }
}

extern "C" int ggnn_rnn_packed_gather_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* b,
                                          float* h_out, const float* Hrows, int64_t num_rows, const int32_t* row_ptr,
                                          const int32_t* gather_row, int64_t M, const float* nin, int T, int use_avg,
                                          float* save_incoming, int V, int D, int act, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0 && num_rows >= 0 && M >= 0 && M < (1LL << 31), "bad sizes V=%d D=%d rows=%lld M=%lld", V, D,
                   (long long)num_rows, (long long)M);
    GGNN_CHECK_ARG(act == GGNN_ACT_TANH || act == GGNN_ACT_RELU, "unknown activation %d", act);
    if (!ggnn_rnn_fused_supported(D, nx))
        return fail(GGNN_E_UNSUPPORTED, "fused RNN cell supports D = 32, 64 with nx = 1..3 and D = 100 with nx = 1 (got D=%d nx=%d)", D, nx);
    if ((unsigned long long)V * D >= (1ULL << 30) || (unsigned long long)num_rows * D >= (1ULL << 30))
        return fail(GGNN_E_UNSUPPORTED, "V*D and num_rows*D must be < 2^30 (32-bit byte offsets)");
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(h && packed && b && h_out && row_ptr, "null pointer");
    GGNN_CHECK_ARG(M == 0 || num_rows == 0 || (Hrows && gather_row), "Hrows / gather_row missing");
    GGNN_CHECK_ARG(!use_avg || (nin && T > 0), "nin [V, T] is required for mean aggregation");
    GGNN_CHECK_ARG(nx == 1 || x_segs, "residual segments missing");
    GGNN_CHECK_ARG(aligned16(h) && aligned16(packed) && aligned16(b) && aligned16(h_out) && aligned16(Hrows) &&
                   (!save_incoming || aligned16(save_incoming)), "pointers must be 16-byte aligned");
    RnnFusedArgs a{};
    const void* inputs[8] = {h, packed, b, Hrows, nin, nullptr, nullptr, nullptr};
    for (int s = 0; s + 1 < nx; ++s) {
        GGNN_CHECK_ARG(x_segs[s] && aligned16(x_segs[s]), "residual segment %d null or misaligned", s);
        a.x[s] = x_segs[s];
        inputs[5 + s] = x_segs[s];
    }
    for (const void* in : inputs)
        GGNN_CHECK_ARG(!in || ((const void*)h_out != in && (const void*)save_incoming != in), "h_out / save_incoming aliases an input");
    GGNN_CHECK_ARG(h_out != save_incoming, "h_out aliases save_incoming");
    a.h = h; a.packed = packed; a.b = b; a.h_out = h_out; a.H = Hrows; a.row_ptr = row_ptr; a.gidx = gather_row; a.nin = nin;
    a.save = save_incoming;
    a.num_rows = (int)num_rows;
    a.M = (num_rows > 0 && Hrows && gather_row) ? (int)M : 0;      // no rows to gather from: every node's slot range is empty
    a.T = T; a.use_avg = use_avg ? 1 : 0; a.V = V; a.act = act;
    return rnn_dispatch(a, D, nx, (hipStream_t)stream);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------------
extern "C" int ggnn_rnn_bwd_fused_supported(int D, int nx) { return ggnn_rnn_fused_supported(D, nx); }

extern "C" size_t ggnn_rnn_bwd_packed_bytes(int D, int nx) { return ggnn_rnn_packed_bytes(D, nx); }

extern "C" int ggnn_rnn_bwd_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream) {
    if (!ggnn_rnn_fused_supported(D, nx))
        return fail(GGNN_E_UNSUPPORTED, "fused RNN cell backward supports D = 32, 64 with nx = 1..3 and D = 100 with nx = 1 (got D=%d nx=%d)", D, nx);
    GGNN_CHECK_ARG(W && packed && aligned16(packed) && (const void*)W != (const void*)packed, "null, misaligned or aliasing pointer");
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return rnn_bwd_pack<100>(W, nx, packed, st);
        case 64: return rnn_bwd_pack<64>(W, nx, packed, st);
        default: return rnn_bwd_pack<32>(W, nx, packed, st);
    }
}

extern "C" int ggnn_rnn_bwd_fused_f32(const float* g, const float* out, const float* packed, float* dP, float* const* dx, float* dh,
                                      const float* nin, int T, int use_avg, int nx, int V, int D, int act, ggnn_stream_t stream) {
    return rnn_bwd_impl(g, nullptr, nullptr, 0, out, packed, dP, dx, dh, nin, T, use_avg, nx, V, D, act, stream);
}

extern "C" int ggnn_rnn_bwd_fused_gather_f32(const float* g, const float* gz, const int32_t* gz_heads, int64_t num_rows, const float* out,
                                             const float* packed, float* dP, float* const* dx, float* dh, const float* nin, int T,
                                             int use_avg, int nx, int V, int D, int act, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(gz && gz_heads && aligned16(gz) && aligned16(gz_heads), "gathered gradient: null or misaligned pointer");
    return rnn_bwd_impl(g, gz, gz_heads, num_rows, out, packed, dP, dx, dh, nin, T, use_avg, nx, V, D, act, stream);
}
