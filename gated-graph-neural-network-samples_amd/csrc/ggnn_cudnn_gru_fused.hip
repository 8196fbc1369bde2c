// CudnnCompatibleGRUCell (chem_tensorflow_sparse.py:105-108) in one launch:
//
//     [r|u] = sigmoid([x_0 | .. | x_{nx-1} | h] Wg + bg)          Wg  [(nx+1) D, 2D]
//     hc    = h Wch + bch                                        Wch [D, D]
//     c     = tanh([x_0 | .. | x_{nx-1}] Wcx + bcx + r * hc)      Wcx [nx D, D]
//     h'    = u*h + (1-u)*c
//
// x_{nx-1} is the aggregated messages (ggnn_gather_segment_sum_f32 over the compact rows wrote them: an ordinary input segment here,
// so layers with an edge bias or sum aggregation are no special case), the other x are residual states.  The composed route
// (cudnn_gru_impl, ggnn_gemm.hip) runs three f32-MFMA GEMM launches and sends r, u and hc through HBM as [V, D] buffers; here they
// stay in registers.  Unlike the TF GRUCell, r multiplies the hidden projection AFTER the product, so no accumulator has to become
// an A operand: the cell is four accumulator sets (r, u, cx, ch) over 3 (nx + 1) weight blocks [D, D] and an element-wise epilogue.
//
// Operands: exact bf16x3 only (SplitCfg<D, kSplitBf16x3> stage images, six partial products accumulated in f32).
//
// Stage order = image order (cudnn_pack_kernel), chosen so that each operand fragment is read from HBM once per pass and split once:
//     for each x_s:  Wg rows of x_s, r columns | Wg rows of x_s, u columns | Wcx rows of x_s
//     for h:         Wg rows of h,   r columns | Wg rows of h,   u columns | Wch
// Accumulation order is therefore fixed -- r / u: the x segments in order, h last; cx: the x segments in order; ch: h alone -- and
// h' is bit-identical from run to run and with or without the saves.
//
// Weight streaming: a two-slot LDS-DMA ring (the structure of the fused GRU's ring form 0).  One barrier per stage: it publishes the
// image of stage i (every wave waits for its own DMA pieces before it) and retires the slot of stage i - 1, into which the DMA of stage
// i + 1 is issued at once, under the MFMAs of stage i.  The last stage of a pass brings in the first image of the workgroup's next pass.
// An image is 8 KiB at D = 32, 24 KiB at D = 64, 72 KiB at D = 100: the ring takes 16 / 48 / 144 KiB of the CU's 160.
//
// Row tiling: persistent workgroups of 8 waves, a wave owns one 16-row tile per pass (128 rows per pass), passes are assigned
// statically (pass = blockIdx.x + k gridDim.x): no ticket counter, no atomics.  Every wave executes 3 (nx + 1) barriers per pass,
// whatever V is.  Rows >= V are neither read nor written: their lanes read row V - 1 and store nothing.  Control flow around
// barriers is uniform per workgroup.  32-bit byte offsets: V * D must stay below 2^30 (the entry point refuses larger calls).
//
// The operand fragment of the NEXT segment (or of the next pass's first segment) is requested under the third stage of the current one.
//
// Training form (SAVE): the same launch also stores r, u, c, hc as [V, D] each -- what variants._hip_backward reads.  The epilogue's
// contractions are written out (fmaf), so both instantiations compute h' with the same instructions.
#include "ggnn_split.hpp"
#include <algorithm>

namespace ggnn {
namespace {

template <int D>
using CudnnImg = SplitCfg<D, kSplitBf16x3>;

constexpr int kCudnnWaves = 8;                         // waves per workgroup; each owns a 16-row tile of the pass
constexpr int kCudnnRows = kCudnnWaves * 16;           // rows per pass

// Occupancy: the launch bound is the occupancy the launcher claims.  D = 100: the ring is 144 KiB, one workgroup per CU = 2 waves per
// SIMD = 256 registers.  D = 64: four accumulator sets of 16 registers do not fit 128 registers without scratch (92 .. 152 B per
// lane when bounded so), so it runs one workgroup per CU as well.  D = 32: two workgroups per CU = 4 waves per SIMD = 128 registers.
template <int D>
struct CudnnCfg {
    static constexpr int LDS = 2 * CudnnImg<D>::IMG_BYTES;
    static constexpr int WG_PER_CU = D == 32 ? 2 : 1;
    static constexpr int WAVES_PER_SIMD = WG_PER_CU * kCudnnWaves / 4;
    static_assert(WG_PER_CU * LDS <= 160 * 1024, "the rings of a CU's workgroups must fit its LDS");
};

struct CudnnFusedArgs {
    const float* x[3];                                 // the nx input segments; the last one is the aggregated messages
    const float* h;
    const float* packed;                               // 3 (nx + 1) images, IMG_BYTES apart, in stage order
    const float* bg;
    const float* bcx;
    const float* bch;
    float* h_out;
    float* save_r;                                     // all four null (inference) or [V, D] each
    float* save_u;
    float* save_c;
    float* save_hc;
    int V;
};

template <int D>
__global__ void cudnn_pack_kernel(const float* __restrict__ Wg, const float* __restrict__ Wcx, const float* __restrict__ Wch, int nx,
                                  float* __restrict__ packed) {
    const int ci = blockIdx.y, seg = ci / 3, which = ci % 3;      // stage order: segment-major, {r, u, candidate} inside
    const int first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    StageValue<D> v{Wg, seg * D, which * D, 2 * D, -1, nullptr, 0, 0, -1};
    if (which == 2) {
        if (seg < nx) { v.W = Wcx; v.r0 = seg * D; } else { v.W = Wch; v.r0 = 0; }
        v.c0 = 0; v.ldw = D;
    }
    pack_split_image<D, kSplitBf16x3>(v, packed + (size_t)ci * CudnnImg<D>::IMG, first, stride);
}

// sigmoid(z + b) with bs = -log2(e) b, tanh(z + b) with bs = 2 log2(e) b: sigmoid4_acc / tanh4_acc of the fused GRU (exp2 / rcp
// units), every contraction written out
__device__ __forceinline__ f32x4 cudnn_sigmoid4(f32x4 z, f32x4 bs) {
    const f32x4 e = {__builtin_fmaf(z.x, -kLog2e, bs.x), __builtin_fmaf(z.y, -kLog2e, bs.y), __builtin_fmaf(z.z, -kLog2e, bs.z),
                     __builtin_fmaf(z.w, -kLog2e, bs.w)};
    return rcp_4(exp2_4(e) + 1.0f);
}
__device__ __forceinline__ f32x4 cudnn_tanh4(f32x4 z, f32x4 bs) {
    constexpr float k = 2.0f * kLog2e;
    const f32x4 e = {__builtin_fmaf(z.x, k, bs.x), __builtin_fmaf(z.y, k, bs.y), __builtin_fmaf(z.z, k, bs.z), __builtin_fmaf(z.w, k, bs.w)};
    const f32x4 q = rcp_4(exp2_4(e) + 1.0f);
    return f32x4{__builtin_fmaf(-2.0f, q.x, 1.0f), __builtin_fmaf(-2.0f, q.y, 1.0f), __builtin_fmaf(-2.0f, q.z, 1.0f),
                 __builtin_fmaf(-2.0f, q.w, 1.0f)};
}
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
    return f32x4{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y), __builtin_fmaf(a.z, b.z, c.z), __builtin_fmaf(a.w, b.w, c.w)};
}

template <int D, int NX, bool SAVE>
__global__ __launch_bounds__(kCudnnWaves * 64, CudnnCfg<D>::WAVES_PER_SIMD) void cudnn_gru_fused_kernel(CudnnFusedArgs a) {
    using S = StageCfg<D>;
    using I = CudnnImg<D>;
    constexpr int NT = S::NT, NS = 3 * (NX + 1);
    extern __shared__ __attribute__((aligned(16))) float ring[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int V = a.V;
    const int n_pass = (V + kCudnnRows - 1) / kCudnnRows;
    const int first_pass = blockIdx.x, pass_stride = gridDim.x;
    if (first_pass >= n_pass) return;                       // (whole workgroup; the launcher starts at most n_pass of them)

    int par = 0;                                            // ring slot of the stage to come
    dma_image_asm<I::IMG_BYTES, kCudnnWaves>(a.packed, ring, wave, lane);
    Frag<D> fn;                                             // the operand fragment requested ahead
    {
        const int r0 = first_pass * kCudnnRows + wave * 16 + li;
        load_frag<D>(fn, a.x[0], r0 < V ? r0 : V - 1, kq);
    }

    for (int pass = first_pass; pass < n_pass; pass += pass_stride) {
        const bool more = pass + pass_stride < n_pass;      // (uniform per workgroup)
        const int r = pass * kCudnnRows + wave * 16 + li;
        const bool live = r < V;
        const int rc = live ? r : V - 1;                    // (a row of its own for every lane: nothing beyond V is read)
        int rn = rc;                                        // this lane's row in the workgroup's next pass
        if (more) {
            const int t = r + pass_stride * kCudnnRows;
            rn = t < V ? t : V - 1;
        }

        f32x4 acc_r[NT], acc_u[NT], acc_x[NT], acc_h[NT];
        Frag<D> f;
        SFrag<D> sf;
        f32x4 h_tail = {0.f, 0.f, 0.f, 0.f};                // h at the columns of the partly filled last tile (D % 16 != 0)
#pragma unroll
        for (int s = 0; s <= NX; ++s) {
            f = fn;
            split_frag<D, kSplitBf16x3>(sf, f);
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const int i = 3 * s + w;                    // stage of the pass = image
                dma_wait();
                __syncthreads();                            // image i has landed; nobody reads the other slot any more
                const float* cur = ring + ((par + i) & 1) * I::IMG;
                float* nxt = ring + ((par + i + 1) & 1) * I::IMG;
                if (i + 1 < NS) dma_image_asm<I::IMG_BYTES, kCudnnWaves>(a.packed + (size_t)(i + 1) * I::IMG, nxt, wave, lane);
                else if (more) dma_image_asm<I::IMG_BYTES, kCudnnWaves>(a.packed, nxt, wave, lane);
                if (w == 2) {
                    if (s < NX) load_frag<D>(fn, s + 1 < NX ? a.x[s + 1] : a.h, rc, kq);
                    else {
                        load_frag<D>(fn, a.x[0], rn, kq);
                        if constexpr (S::NR > 0) {
                            constexpr int c0 = 16 * S::NC;
                            if (c0 + 4 * kq < D) h_tail = ld4_b(a.h, ((unsigned)rc * (unsigned)D + c0 + 4u * (unsigned)kq) * 4u);
                        }
                    }
                }
                if (w == 0) {
                    if (s == 0) stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc_r, sf, f, cur, li, kq);
                    else stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc_r, sf, f, cur, li, kq);
                } else if (w == 1) {
                    if (s == 0) stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc_u, sf, f, cur, li, kq);
                    else stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc_u, sf, f, cur, li, kq);
                } else if (s < NX) {
                    if (s == 0) stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc_x, sf, f, cur, li, kq);
                    else stage_mma_split<D, NT, false, false, kSplitBf16x3>(acc_x, sf, f, cur, li, kq);
                } else {
                    stage_mma_split<D, NT, true, false, kSplitBf16x3>(acc_h, sf, f, cur, li, kq);
                }
            }
        }
        par = (par + NS) & 1;

        // epilogue in registers; f is the h fragment: its float4 c covers the columns of output tile c
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c0 = nt * 16 + 4 * kq;
            if (c0 < D) {
                const f32x4 rv = cudnn_sigmoid4(acc_r[nt], ld4(a.bg + c0) * (-kLog2e));
                const f32x4 uv = cudnn_sigmoid4(acc_u[nt], ld4(a.bg + D + c0) * (-kLog2e));
                const f32x4 hc = acc_h[nt] + ld4(a.bch + c0);
                const f32x4 z = fma4(rv, hc, acc_x[nt]);    // t = r * hc folded into the cx accumulator
                const f32x4 cv = cudnn_tanh4(z, ld4(a.bcx + c0) * (2.0f * kLog2e));
                f32x4 hv = h_tail;
                if (nt < S::NC) hv = f.v[nt < S::NC ? nt : 0];
                const f32x4 out = fma4(uv, hv, fma4(-uv, cv, cv));   // u h + (1 - u) c
                if (live) {
                    const unsigned ob = ((unsigned)r * (unsigned)D + (unsigned)c0) * 4u;
                    st4_b(a.h_out, ob, out);
                    if constexpr (SAVE) {
                        st4_b(a.save_r, ob, rv);
                        st4_b(a.save_u, ob, uv);
                        st4_b(a.save_c, ob, cv);
                        st4_b(a.save_hc, ob, hc);
                    }
                }
            }
        }
    }
}

template <int D, int NX, bool SAVE>
int cudnn_launch_one(const CudnnFusedArgs& a, hipStream_t st) {
    using C = CudnnCfg<D>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (C::LDS > 48 * 1024) GGNN_CHECK_HIP(allow_dynamic_lds(&cudnn_gru_fused_kernel<D, NX, SAVE>, C::LDS, lds_ok));
    const long long n_pass = ((long long)a.V + kCudnnRows - 1) / kCudnnRows;
    const long long blocks = std::min<long long>(n_pass, (long long)C::WG_PER_CU * num_cus());
    hipLaunchKernelGGL((cudnn_gru_fused_kernel<D, NX, SAVE>), dim3((unsigned)blocks), dim3(kCudnnWaves * 64), C::LDS, st, a);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

template <int D, int NX>
int cudnn_launch(const CudnnFusedArgs& a, hipStream_t st) {
    return a.save_r ? cudnn_launch_one<D, NX, true>(a, st) : cudnn_launch_one<D, NX, false>(a, st);
}

template <int D>
int cudnn_launch_d(const CudnnFusedArgs& a, int nx, hipStream_t st) {
    switch (nx) {
        case 1: return cudnn_launch<D, 1>(a, st);
        case 2: return cudnn_launch<D, 2>(a, st);
        default: return cudnn_launch<D, 3>(a, st);
    }
}

template <int D>
int cudnn_pack(const float* Wg, const float* Wcx, const float* Wch, int nx, float* packed, hipStream_t st) {
    hipLaunchKernelGGL((cudnn_pack_kernel<D>), dim3(16, (unsigned)(3 * (nx + 1))), dim3(256), 0, st, Wg, Wcx, Wch, nx, packed);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

int cudnn_img_bytes(int D) {
    return D == 100 ? CudnnImg<100>::IMG_BYTES : D == 64 ? CudnnImg<64>::IMG_BYTES : CudnnImg<32>::IMG_BYTES;
}

const char* const kCudnnSupportedMsg = "fused CudnnCompatibleGRUCell supports D = 32, 64, 100 with nx = 1..3 (got D=%d nx=%d)";

}  // namespace
}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_cudnn_gru_fused_supported(int D, int nx) {
    if (nx < 1 || nx > 3) return 0;
    return (D == 32 || D == 64 || D == 100) ? 1 : 0;
}

extern "C" size_t ggnn_cudnn_gru_packed_bytes(int D, int nx) {
    if (!ggnn_cudnn_gru_fused_supported(D, nx)) return 0;
    return (size_t)3 * (nx + 1) * cudnn_img_bytes(D);
}

extern "C" void ggnn_cudnn_gru_fused_launch_geometry(int D, int nx, int* rows_per_pass, int* max_workgroups) {
    int rows = 0, wgs = 0;
    if (ggnn_cudnn_gru_fused_supported(D, nx)) {
        rows = kCudnnRows;
        wgs = (D == 100 ? CudnnCfg<100>::WG_PER_CU : D == 64 ? CudnnCfg<64>::WG_PER_CU : CudnnCfg<32>::WG_PER_CU) * num_cus();
    }
    if (rows_per_pass) *rows_per_pass = rows;
    if (max_workgroups) *max_workgroups = wgs;
}

extern "C" int ggnn_cudnn_gru_pack_weights_f32(const float* Wg, const float* Wcx, const float* Wch, int nx, int D, float* packed,
                                               ggnn_stream_t stream) {
    if (!ggnn_cudnn_gru_fused_supported(D, nx)) return fail(GGNN_E_UNSUPPORTED, kCudnnSupportedMsg, D, nx);
    GGNN_CHECK_ARG(Wg && Wcx && Wch && packed && aligned16(packed), "null or misaligned pointer");
    GGNN_CHECK_ARG((const void*)Wg != (const void*)packed && (const void*)Wcx != (const void*)packed &&
                   (const void*)Wch != (const void*)packed, "packed aliases a weight matrix");
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return cudnn_pack<100>(Wg, Wcx, Wch, nx, packed, st);
        case 64: return cudnn_pack<64>(Wg, Wcx, Wch, nx, packed, st);
        default: return cudnn_pack<32>(Wg, Wcx, Wch, nx, packed, st);
    }
}

extern "C" int ggnn_cudnn_gru_packed_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* bg,
                                         const float* bcx, const float* bch, float* h_out, float* save_r, float* save_u,
                                         float* save_c, float* save_hc, int V, int D, ggnn_stream_t stream) {
    GGNN_CHECK_ARG(V >= 0 && D > 0, "bad sizes V=%d D=%d", V, D);
    if (!ggnn_cudnn_gru_fused_supported(D, nx)) return fail(GGNN_E_UNSUPPORTED, kCudnnSupportedMsg, D, nx);
    if ((unsigned long long)V * D >= (1ULL << 30)) return fail(GGNN_E_UNSUPPORTED, "V*D must be < 2^30 (32-bit byte offsets)");
    if (V == 0) return GGNN_OK;
    GGNN_CHECK_ARG(x_segs && h && packed && bg && bcx && bch && h_out, "null pointer");
    float* const saves[4] = {save_r, save_u, save_c, save_hc};
    const int given = (save_r != nullptr) + (save_u != nullptr) + (save_c != nullptr) + (save_hc != nullptr);
    GGNN_CHECK_ARG(given == 0 || given == 4, "save_r / save_u / save_c / save_hc must be all null or all given");
    GGNN_CHECK_ARG(aligned16(h) && aligned16(packed) && aligned16(bg) && aligned16(bcx) && aligned16(bch) && aligned16(h_out),
                   "pointers must be 16-byte aligned");
    CudnnFusedArgs a{};
    const void* inputs[8] = {h, packed, bg, bcx, bch, nullptr, nullptr, nullptr};
    for (int s = 0; s < nx; ++s) {
        GGNN_CHECK_ARG(x_segs[s] && aligned16(x_segs[s]), "input segment %d null or misaligned", s);
        a.x[s] = x_segs[s];
        inputs[5 + s] = x_segs[s];
    }
    for (const void* in : inputs) GGNN_CHECK_ARG(!in || (const void*)h_out != in, "h_out aliases an input");
    if (given) {
        for (int i = 0; i < 4; ++i) {
            GGNN_CHECK_ARG(aligned16(saves[i]), "save buffers must be 16-byte aligned");
            GGNN_CHECK_ARG(saves[i] != h_out, "a save buffer aliases h_out");
            for (const void* in : inputs) GGNN_CHECK_ARG(!in || (const void*)saves[i] != in, "a save buffer aliases an input");
            for (int j = 0; j < i; ++j) GGNN_CHECK_ARG(saves[i] != saves[j], "two save buffers alias each other");
        }
    }
    a.h = h; a.packed = packed; a.bg = bg; a.bcx = bcx; a.bch = bch; a.h_out = h_out;
    a.save_r = save_r; a.save_u = save_u; a.save_c = save_c; a.save_hc = save_hc; a.V = V;
    hipStream_t st = (hipStream_t)stream;
    switch (D) {
        case 100: return cudnn_launch_d<100>(a, nx, st);
        case 64: return cudnn_launch_d<64>(a, nx, st);
        default: return cudnn_launch_d<32>(a, nx, st);
    }
}
