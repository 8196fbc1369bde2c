// Building blocks of the column-panel kernels for hidden sizes 128 / 192 / 256 (ggnn_panel.hip: forward GRU and transform;
// ggnn_gru_bwd_panel.hip: GRU backward): panel geometry, the f32 and chunk-major split image formats, the stage products and the
// LDS-DMA of an image.  See the header comment of ggnn_panel.hip.
#pragma once
#include "ggnn_split.hpp"
// 1: panel_part_mma_split recomputes the lane part of its LDS / L2 addresses in every call (the lane coordinates pass through an empty asm).
// Without it hipcc keeps a per-(stage, part) address register set alive across the whole pass and the split-form GRU comes out with
// 152-492 B of scratch per lane at 256 registers; with it: no scratch, 208-228 registers; D = 256 launch 507.7 -> 497.5 us (round 4).
#ifndef GGNN_PANEL_REMAT
#define GGNN_PANEL_REMAT 1
#endif
#include <type_traits>

namespace ggnn {

template <int D>
struct PanelCfg {
    static_assert(D % 64 == 0, "panel kernels need a hidden size that is a multiple of 64");
    static constexpr int PT = 4;                 // column tiles per panel
    static constexpr int BN = 64;                // columns per panel
    static constexpr int NP = D / BN;            // panels per D-column weight block
    static constexpr int NC = D / 16;            // k chunks == column tiles of a gate
    static constexpr int IMG = D * BN;           // floats per panel image
    static constexpr int IMG_BYTES = IMG * 4;
};

// image[c][kq][n][e] = value(16c + 4kq + e, n)   (n < 64): the k-interleaved layout of ggnn_stage.hpp.  value(k, n): entry (k, n) of
// the D x 64 panel -- a functor, so that one image writer serves plain, transposed and masked-on-the-fly sources.
template <int D, class F>
__device__ __forceinline__ void pack_panel_image_fn(F value, float* __restrict__ img, int first, int stride) {
    using C = PanelCfg<D>;
    for (int i = first; i < C::IMG; i += stride) {
        const int e = i & 3, n = (i >> 2) % C::BN, ck = (i >> 2) / C::BN;
        img[i] = value(4 * ck + e, n);
    }
}

// the panel of a weight block: value(k, n) = W[r0 + k][c0 + n]
// TRANS: image value (k, n) = W[c0 + n][r0 + k] instead of W[r0 + k][c0 + n] -- a panel of a TRANSPOSED block (the GRU backward)
template <bool TRANS>
struct PanelSrc {
    const float* W; int r0, c0, ldw;
    __device__ __forceinline__ float operator()(int k, int n) const {
        return TRANS ? W[(size_t)(c0 + n) * ldw + r0 + k] : W[(size_t)(r0 + k) * ldw + c0 + n];
    }
};

template <int D, bool TRANS = false>
__device__ __forceinline__ void pack_panel_image(const float* __restrict__ W, int r0, int c0, int ldw, float* __restrict__ img,
                                                 int first, int stride) {
    pack_panel_image_fn<D>(PanelSrc<TRANS>{W, r0, c0, ldw}, img, first, stride);
}

// ---- the GRU's panels in split form: image [c2][plane][g][n < 64][8 x bf16], CHUNK-major, so that it can be brought in in PARTS --
// A split 64-column panel of a 256-row block is 96 KiB: two of them do not fit the LDS.  The ring therefore holds PARTS of an
// image (D = 256: 2 x 4 chunks = 48 KiB each; 192: 3 x 2 chunks = 24 KiB; 128: the whole 48 KiB image) and a stage is PARTS
// DMA / MFMA / barrier rounds over the same accumulators.
// FMT (ggnn_split.hpp): kSplitBf16x3 = three planes per chunk (12 KiB); kSplitF16x2 (the panel GRU since the end of round 4) = two
// (8 KiB): a D = 256 image is 64 KiB and two WHOLE images fit the ring -- no parts at any width.
template <int D, int FMT = kSplitBf16x3>
struct PanelGruSplitCfg {
    static constexpr int NC2 = D / 32;
    static constexpr int NPL = SplitFmt<FMT>::NP;                  // planes per chunk
    static constexpr int CHUNK_BYTES = NPL * 4 * 64 * 16;          // 12 KiB per 32-chunk (two planes: 8)
    static constexpr int PARTS = FMT == kSplitF16x2 ? 1 : (D == 256 ? 2 : (D == 192 ? 3 : 1));
    static constexpr int CP = NC2 / PARTS;                         // chunks per part
    static constexpr int PART_BYTES = CP * CHUNK_BYTES;
    static constexpr int PART = PART_BYTES / 4;
    static constexpr int IMG_BYTES = NC2 * CHUNK_BYTES;
    static constexpr int IMG = IMG_BYTES / 4;
    static_assert(NC2 % PARTS == 0 && PART_BYTES % 8192 == 0, "parts are whole chunks and whole KiB per wave of an 8-wave workgroup");
};

template <int D, int FMT, class F>
__device__ __forceinline__ void pack_panel_gru_split_image_fn(F value, float* __restrict__ img, int first, int stride) {
    using C = PanelGruSplitCfg<D, FMT>;
    for (int i = first; i < C::IMG; i += stride) {
        const int slot = i >> 2, pr = i & 3;                       // 16-byte slot ((c2*NPL + plane)*4 + g)*64 + n
        const int n = slot % 64, g = (slot / 64) % 4, plane = (slot / 256) % C::NPL, c2 = slot / (256 * C::NPL);
        const int j0 = 2 * pr;
        const int k0 = 32 * c2 + 16 * (j0 >> 2) + 4 * g + (j0 & 3);
        const float v0 = value(k0, n), v1 = value(k0 + 1, n);
        img[i] = __uint_as_float(split_piece_bits<FMT>(v0, plane) | (split_piece_bits<FMT>(v1, plane) << 16));
    }
}

template <int D, int FMT = kSplitBf16x3, bool TRANS = false>
__device__ __forceinline__ void pack_panel_gru_split_image(const float* __restrict__ W, int r0, int c0, int ldw, float* __restrict__ img,
                                                           int first, int stride) {
    pack_panel_gru_split_image_fn<D, FMT>(PanelSrc<TRANS>{W, r0, c0, ldw}, img, first, stride);
}

// ---- the transform's panel in 3-way split form (ggnn_split.hpp): image = three bf16 planes [c2][g][n < 64][8 x bf16] -----------
// (the stationary-image transform kernel of ggnn_panel.hip; the ring kernel takes pack_panel_gru_split_image's chunk-major format)
template <int D>
struct PanelSplitCfg {
    static constexpr int NC2 = D / 32;
    static constexpr int PLANE_BYTES = NC2 * 4 * 64 * 16;          // D * 128
    static constexpr int IMG_BYTES = 3 * PLANE_BYTES;              // 96 KiB at D = 256: ONE image per workgroup, no ring
    static constexpr int IMG = IMG_BYTES / 4;
};

template <int D, class F>
__device__ __forceinline__ void pack_panel_split_image_fn(F value, float* __restrict__ img, int first, int stride) {
    using C = PanelSplitCfg<D>;
    constexpr int PW = C::PLANE_BYTES / 4;
    for (int i = first; i < C::IMG; i += stride) {
        const int plane = i / PW, w = i % PW;
        const int slot = w >> 2, pr = w & 3;
        const int n = slot % 64, cg = slot / 64, c2 = cg >> 2, g = cg & 3;
        const int j0 = 2 * pr;
        const int k0 = 32 * c2 + 16 * (j0 >> 2) + 4 * g + (j0 & 3);
        const float v0 = value(k0, n), v1 = value(k0 + 1, n);
        img[i] = __uint_as_float(split_piece_bits(v0, plane) | (split_piece_bits(v1, plane) << 16));
    }
}

template <int D>
__device__ __forceinline__ void pack_panel_split_image(const float* __restrict__ W, int r0, int c0, int ldw, float* __restrict__ img,
                                                       int first, int stride) {
    pack_panel_split_image_fn<D>(PanelSrc<false>{W, r0, c0, ldw}, img, first, stride);
}

// ---- which weight panel each image of the panel GRU kernels holds (the pack kernels of ggnn_panel.hip / ggnn_gru_bwd_panel.hip and
// the training step's one-launch image preparation read the same maps) ---------------------------------------------------------------
__host__ __device__ constexpr int panel_gru_images(int D, int nx) { return 3 * (nx + 1) * (D / 64); }
__host__ __device__ constexpr int panel_gru_bwd_images(int D, int nx) { return 3 * (nx + 1) * (D / 64); }

// forward GRU, one image per stage, in stage order:
//   phase R :  (s, p)            s < NS, p < NP     Wg rows [sD, (s+1)D), columns [64p, 64p+64)
//   phase UC:  p < NP:  for s < NX: U (Wg rows s, cols D + 64p ..), C (Wc rows s, cols 64p ..);  U (Wg rows h);  C (Wc rows h = r*h)
template <int D>
__device__ __forceinline__ PanelSrc<false> panel_gru_fwd_image_src(const float* Wg, const float* Wc, int nx, int i) {
    using C = PanelCfg<D>;
    const int ns = nx + 1, NP = C::NP;
    if (i < ns * NP) return {Wg, (i / NP) * D, (i % NP) * C::BN, 2 * D};
    const int j = i - ns * NP, p = j / (2 * ns), q = j % (2 * ns);          // q: U x_0, C x_0, .., U h, C rh
    const int s = q / 2;
    if (q % 2 == 0) return {Wg, s * D, D + p * C::BN, 2 * D};
    return {Wc, s * D, p * C::BN, D};
}

// GRU backward: image i = (block b, operand w, panel p), b = 0: the h rows, b = 1 + s: the rows of x segment s;  w = 0: Wc^T, 1: Wg_r^T,
// 2: Wg_u^T.  image[k][n] = B(k, 64p + n) with out[:, n] = sum_k A[:, k] B(k, n):  B(k, n) = W[seg D + n][c0 + k]
template <int D>
__device__ __forceinline__ PanelSrc<true> panel_gru_bwd_image_src(const float* Wg, const float* Wc, int nx, int i) {
    using C = PanelCfg<D>;
    constexpr int NP = C::NP;
    const int b = i / (3 * NP), w = (i / NP) % 3, p = i % NP;
    const int seg = b == 0 ? nx : b - 1;
    return {w == 0 ? Wc : Wg, w == 2 ? D : 0, seg * D + p * C::BN, w == 0 ? D : 2 * D};
}

template <int FMT = kSplitBf16x3>
__device__ __forceinline__ void frag_planes(f32x4 x, f32x4 y, u32x4& hi, u32x4& mid, u32x4& lo) {
    // The fragment is the same for every stage of its segment, so the compiler would split it ONCE and keep all planes live across
    // the stages (96 registers at D = 256: ~450 B of scratch).  The empty asm makes the inputs opaque: the split is redone per stage,
    // 44 vector instructions per 24 MFMAs, and only one chunk's planes are live.
    asm volatile("" : "+v"(x.x), "+v"(x.y), "+v"(x.z), "+v"(x.w), "+v"(y.x), "+v"(y.y), "+v"(y.z), "+v"(y.w));
    unsigned h[4], m[4], l[4];
    split_pair<FMT>(x.x, x.y, h[0], m[0], l[0]); split_pair<FMT>(x.z, x.w, h[1], m[1], l[1]);
    split_pair<FMT>(y.x, y.y, h[2], m[2], l[2]); split_pair<FMT>(y.z, y.w, h[3], m[3], l[3]);
    hi = u32x4{h[0], h[1], h[2], h[3]}; mid = u32x4{m[0], m[1], m[2], m[3]}; lo = u32x4{l[0], l[1], l[2], l[3]};
}

// acc[0..3] (+)= chunks [part*CP, (part+1)*CP) of the fragment x the same chunks of a split panel image; `chunks` points at the
// first of them (in LDS: a ring slot; GLOBAL: the image in L2, cooperative tail pass).  The fragment's 8 values of a chunk are split
// right before the chunk's 24 MFMAs (the next chunk's under the current one's); weight planes rotate through 12 registers.
// FMT = kSplitF16x2: three products per unit (w_lo a_hi, w_hi a_lo, w_hi a_hi), both planes of the next unit fetched a unit ahead.
template <int D, bool ZERO, bool GLOBAL, int part, int FMT = kSplitBf16x3>
__device__ __forceinline__ void panel_part_mma_split(f32x4 (&acc)[4], const Frag<D>& a, const float* chunks, int li, int kq) {
    using C = PanelGruSplitCfg<D, FMT>;
    constexpr int NU = C::CP * 4;
#if GGNN_PANEL_REMAT
    asm volatile("" : "+v"(li), "+v"(kq));      // (the lane part of the address is recomputed per call, see stage_mma_split_at's REMAT)
#endif
    const unsigned voff = (unsigned)(kq * 64 + li) * 16u;
    const unsigned long long gb = reinterpret_cast<unsigned long long>(chunks);
    const float* sbase = chunks;
    if constexpr (GLOBAL) {     // wave-uniform base in scalar registers + one 32-bit per-lane offset (see panel_mma_global)
        const unsigned glo = __builtin_amdgcn_readfirstlane((unsigned)gb), ghi = __builtin_amdgcn_readfirstlane((unsigned)(gb >> 32));
        sbase = reinterpret_cast<const float*>(((unsigned long long)ghi << 32) | glo);
    }
    auto slot = [&](int u, int p) -> u32x4 {                        // unit u = (chunk cc, tile j), plane p
        const unsigned off = voff + (unsigned)((((u / 4) * C::NPL + p) * 4) * 64 + (u % 4) * 16) * 16u;
        if constexpr (GLOBAL) return __builtin_bit_cast(u32x4, ld4_b(sbase, off));
        else return *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(chunks) + off);
    };
    u32x4 ah, am, al;
    if constexpr (FMT == kSplitF16x2) {
        u32x4 wh = slot(0, 0), wm = slot(0, 1), nh = wh, nm = wm;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int cc = u / 4, j = u % 4;
            const bool more = u + 1 < NU;
            if (j == 0) frag_planes<FMT>(a.v[2 * (part * C::CP + cc)], a.v[2 * (part * C::CP + cc) + 1], ah, am, al);
            f32x4 c = (ZERO && cc == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
            if (more) { nm = slot(u + 1, 1); nh = slot(u + 1, 0); }
            __builtin_amdgcn_sched_barrier(0);
            c = mfma_f16(wm, ah, c);
            c = mfma_f16(wh, am, c);
            c = mfma_f16(wh, ah, c);
            __builtin_amdgcn_sched_barrier(0);
            wm = nm; wh = nh;
            acc[j] = c;
        }
        return;
    }
    u32x4 wh = slot(0, 0), wm = slot(0, 1), wl = slot(0, 2);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int cc = u / 4, j = u % 4;
        const bool more = u + 1 < NU;
        if (j == 0) frag_planes(a.v[2 * (part * C::CP + cc)], a.v[2 * (part * C::CP + cc) + 1], ah, am, al);
        f32x4 c = (ZERO && cc == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
        c = mfma_bf16(wl, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wl = slot(u + 1, 2);
        c = mfma_bf16(wm, am, c);
        c = mfma_bf16(wm, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wm = slot(u + 1, 1);
        c = mfma_bf16(wh, al, c);
        c = mfma_bf16(wh, am, c);
        c = mfma_bf16(wh, ah, c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wh = slot(u + 1, 0);
        acc[j] = c;
    }
}

// acc[0..3] (+)= fragment x panel image: per k chunk 4 ds_read_b128 feed 16 MFMAs; one chunk of read-ahead
template <int D, bool ZERO>
__device__ __forceinline__ void panel_mma(f32x4 (&acc)[4], const Frag<D>& a, const float* img, int li, int kq) {
    using C = PanelCfg<D>;
    const f32x4* base = reinterpret_cast<const f32x4*>(img) + kq * C::BN + li;
    f32x4 w[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[0][j] = base[j * 16];
#pragma unroll
    for (int c = 0; c < C::NC; ++c) {
        if (c + 1 < C::NC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[(c + 1) & 1][j] = base[(c + 1) * 4 * C::BN + j * 16];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 cin = (ZERO && c == 0 && e == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c & 1][j][e], a.v[c][e], cin, 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// LDS-DMA of `BYTES` (a multiple of NW KiB) from src to LDS dst by an NW-wave workgroup (see dma_stage_image)
template <int BYTES, int NW>
__device__ __forceinline__ void dma_block(const float* src, float* dst, int wave, int lane) {
    constexpr int PER_WAVE = BYTES / (NW * 1024);
    static_assert(BYTES % (NW * 1024) == 0, "block must split into whole KiB per wave");
    char* d = reinterpret_cast<char*>(dst) + (size_t)wave * PER_WAVE * 1024;
    const unsigned voff = (unsigned)lane * 16u;
#pragma unroll
    for (int i0 = 0; i0 < PER_WAVE; i0 += 4) {
        const unsigned long long sb = reinterpret_cast<unsigned long long>(src) + (unsigned long long)wave * PER_WAVE * 1024 + (unsigned long long)i0 * 1024;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)sb);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(sb >> 32));
        const char* s = reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
        lds_void* dl = (lds_void*)(d + i0 * 1024);
        if (i0 + 0 < PER_WAVE) __builtin_amdgcn_global_load_lds((glb_void*)(s + voff), dl, 16, 0, 0);
        if (i0 + 1 < PER_WAVE) __builtin_amdgcn_global_load_lds((glb_void*)(s + voff), dl, 16, 1024, 0);
        if (i0 + 2 < PER_WAVE) __builtin_amdgcn_global_load_lds((glb_void*)(s + voff), dl, 16, 2048, 0);
        if (i0 + 3 < PER_WAVE) __builtin_amdgcn_global_load_lds((glb_void*)(s + voff), dl, 16, 3072, 0);
    }
}

// the same product on RESIDENT planes of the fragment (split once by the caller: the ring transform, and the panel GRU's stages
// that multiply one fragment several times in a row)
template <int D, bool ZERO, int part, int FMT = kSplitBf16x3>
__device__ __forceinline__ void panel_part_mma_planes(f32x4 (&acc)[4], const u32x4 (&ph)[PanelGruSplitCfg<D>::NC2], const u32x4 (&pm)[PanelGruSplitCfg<D>::NC2],
                                                      const u32x4 (&pl)[PanelGruSplitCfg<D>::NC2], const float* chunks, int li, int kq) {
    using C = PanelGruSplitCfg<D, FMT>;
    constexpr int NU = C::CP * 4;
    asm volatile("" : "+v"(li), "+v"(kq));      // (the lane part of the address is recomputed per call: GGNN_PANEL_REMAT's reason)
    const unsigned voff = (unsigned)(kq * 64 + li) * 16u;
    auto slot = [&](int u, int p) -> u32x4 {                        // unit u = (chunk cc, tile j), plane p
        const unsigned off = voff + (unsigned)((((u / 4) * C::NPL + p) * 4) * 64 + (u % 4) * 16) * 16u;
        return *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(chunks) + off);
    };
    if constexpr (FMT == kSplitF16x2) {                             // (pm: the lo pieces; pl unused)
        u32x4 wh = slot(0, 0), wm = slot(0, 1), nh = wh, nm = wm;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int cc = part * C::CP + u / 4, j = u % 4;
            const bool more = u + 1 < NU;
            f32x4 c = (ZERO && u / 4 == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
            if (more) { nm = slot(u + 1, 1); nh = slot(u + 1, 0); }
            __builtin_amdgcn_sched_barrier(0);
            c = mfma_f16(wm, ph[cc], c);
            c = mfma_f16(wh, pm[cc], c);
            c = mfma_f16(wh, ph[cc], c);
            __builtin_amdgcn_sched_barrier(0);
            wm = nm; wh = nh;
            acc[j] = c;
        }
        return;
    }
    u32x4 wh = slot(0, 0), wm = slot(0, 1), wl = slot(0, 2);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int cc = part * C::CP + u / 4, j = u % 4;
        const bool more = u + 1 < NU;
        f32x4 c = (ZERO && u / 4 == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[j];
        c = mfma_bf16(wl, ph[cc], c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wl = slot(u + 1, 2);
        c = mfma_bf16(wm, pm[cc], c);
        c = mfma_bf16(wm, ph[cc], c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wm = slot(u + 1, 1);
        c = mfma_bf16(wh, pl[cc], c);
        c = mfma_bf16(wh, pm[cc], c);
        c = mfma_bf16(wh, ph[cc], c);
        __builtin_amdgcn_sched_barrier(0);
        if (more) wh = slot(u + 1, 0);
        acc[j] = c;
    }
}

}  // namespace ggnn
