// The shared layer of the column-panel kernels for hidden sizes 128 / 192 / 256.  Its five users:
//     ggnn_gru_panel_kernel, msg_transform_ring_kernel (ggnn_panel.hip)    forward GRU, compacted transform
//     ggnn_gru_bwd_panel_kernel (ggnn_gru_bwd_panel.hip)                   GRU backward
//     gcn_panel_layer_kernel (ggnn_gcn_panel.hip)                          GCN layer, forward and BWD
//     rnn_panel_kernel (ggnn_rnn_panel.hip)                                R-GCN cell
// Each multiplies a wave's 16 x D fragment by 64-column panel images that stream through a two-slot LDS-DMA ring.  Here: the panel
// geometry, the f32 and chunk-major split image formats, the stage products and the image DMA; the ring and its publishing barriers
// (PanelRing), the round and the part ladder (panel_round, panel_for_parts), the pass and ticket walks (PanelPassWalk, PanelTickets),
// the rows-in-flight gather ladder, and the host side of a launch.  See the header comment of ggnn_panel.hip.
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

// the 8 values of a fragment's 32-chunk (two quads) -> one quad per plane
template <int FMT = kSplitBf16x3>
__device__ __forceinline__ void chunk_planes(f32x4 x, f32x4 y, u32x4& hi, u32x4& mid, u32x4& lo) {
    unsigned h[4], m[4], l[4];
    split_pair<FMT>(x.x, x.y, h[0], m[0], l[0]); split_pair<FMT>(x.z, x.w, h[1], m[1], l[1]);
    split_pair<FMT>(y.x, y.y, h[2], m[2], l[2]); split_pair<FMT>(y.z, y.w, h[3], m[3], l[3]);
    hi = u32x4{h[0], h[1], h[2], h[3]}; mid = u32x4{m[0], m[1], m[2], m[3]}; lo = u32x4{l[0], l[1], l[2], l[3]};
}

template <int FMT = kSplitBf16x3>
__device__ __forceinline__ void frag_planes(f32x4 x, f32x4 y, u32x4& hi, u32x4& mid, u32x4& lo) {
    // The fragment is the same for every stage of its segment, so the compiler would split it ONCE and keep all planes live across
    // the stages (96 registers at D = 256: ~450 B of scratch).  The empty asm makes the inputs opaque: the split is redone per stage,
    // 44 vector instructions per 24 MFMAs, and only one chunk's planes are live.
    asm volatile("" : "+v"(x.x), "+v"(x.y), "+v"(x.z), "+v"(x.w), "+v"(y.x), "+v"(y.y), "+v"(y.z), "+v"(y.w));
    chunk_planes<FMT>(x, y, hi, mid, lo);
}

// the whole fragment -> RESIDENT planes (panel_part_mma_planes' operand), split once for the stages that multiply it in a row
// (N = D / 32; deduced, because a kernel form without planes declares one-element dummies and still names this call)
template <int D, int FMT = kSplitBf16x3, int N>
__device__ __forceinline__ void frag_to_planes(const Frag<D>& a, u32x4 (&ph)[N], u32x4 (&pm)[N], u32x4 (&pl)[N]) {
    static_assert(N == D / 32 || N == 1, "one quad per plane and 32-chunk");
#pragma unroll
    for (int c2 = 0; c2 < N; ++c2) chunk_planes<FMT>(a.v[2 * c2], a.v[2 * c2 + 1], ph[c2], pm[c2], pl[c2]);
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

// ---- the two-slot ring ---------------------------------------------------------------------------------------------------------------
// Slot `cur` holds the part the round multiplies; the other slot receives the next part during the round; the round's barrier
// publishes it and flips.  ASM: slots are filled by dma_image_asm (split images), else by dma_block (the f32 images of the GRU
// backward, which hipcc waits for itself).
//
// The counted wait.  A round's DMA pieces are the FIRST vector-memory instructions a wave issues in it, and the vector-memory counter
// retires in order.  If the wave issued `keep` more behind them (the next tile's rows, a panel's stores) and nothing after those,
// "at most keep outstanding" can only leave those `keep`: the pieces have landed, and the rest stays in flight across the barrier (it
// has until the next round's barrier).  Each kernel says at its call why its `keep` instructions are the last ones it issued.
template <int SLOT_BYTES, int NW, bool ASM = true>
struct PanelRing {
    static constexpr int SLOTF = SLOT_BYTES / 4;
    float* const lds;                                  // [2][SLOTF]
    const int wave, lane;
    int cur = 0;
    __device__ __forceinline__ void dma(const float* src, float* dst) const {
        if constexpr (ASM) dma_image_asm<SLOT_BYTES, NW>(src, dst, wave, lane);
        else dma_block<SLOT_BYTES, NW>(src, dst, wave, lane);
    }
    __device__ __forceinline__ void fill_first(const float* src) const { dma(src, lds); }
    __device__ __forceinline__ void fill_next(const float* src) const { dma(src, lds + (cur ^ 1) * SLOTF); }
    __device__ __forceinline__ const float* slot() const { return lds + cur * SLOTF; }
    // everything this wave has issued has landed, for every wave (no flip: the wait for the first fill)
    __device__ __forceinline__ void first_ready() const { if constexpr (ASM) dma_wait(); __syncthreads(); }
    __device__ __forceinline__ void publish() { first_ready(); cur ^= 1; }
    __device__ __forceinline__ void publish_keep(int keep) {         // (wave-uniform; s_waitcnt takes an immediate)
        switch (keep) {
#define GGNN_WC(N) case N: asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)" ::: "memory"); break;
            GGNN_WC(0) GGNN_WC(1) GGNN_WC(2) GGNN_WC(3) GGNN_WC(4) GGNN_WC(5) GGNN_WC(6) GGNN_WC(7) GGNN_WC(8) GGNN_WC(9) GGNN_WC(10)
            GGNN_WC(11) GGNN_WC(12) GGNN_WC(13) GGNN_WC(14) GGNN_WC(15) GGNN_WC(16) GGNN_WC(17) GGNN_WC(18) GGNN_WC(19) GGNN_WC(20)
            GGNN_WC(21) GGNN_WC(22) GGNN_WC(23) GGNN_WC(24) GGNN_WC(25) GGNN_WC(26)
#undef GGNN_WC
            default: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
        }
        __builtin_amdgcn_s_barrier();
        cur ^= 1;
    }
    template <int KEEP>
    __device__ __forceinline__ void publish_keep() { static_assert(KEEP >= 0 && KEEP <= 26, "no such wait"); publish_keep(KEEP); }
};

// what the ring's other slot receives while part `part` of image `img` is multiplied: the next part of this image, else the first
// part of image `nimg`
template <int PARTS, int IMGF, int SLOTF>
__device__ __forceinline__ const float* panel_next_part(const float* packed, int img, int part, int nimg) {
    return part + 1 < PARTS ? packed + (size_t)img * IMGF + (size_t)(part + 1) * SLOTF : packed + (size_t)nimg * IMGF;
}

// fn(part) for every part of an image, unrolled
template <int PARTS, class F>
__device__ __forceinline__ void panel_for_parts(F&& fn) {
    static_assert(PARTS >= 1 && PARTS <= 3, "an image comes in 1 .. 3 parts");
    fn(std::integral_constant<int, 0>{});
    if constexpr (PARTS > 1) fn(std::integral_constant<int, 1>{});
    if constexpr (PARTS > 2) fn(std::integral_constant<int, 2>{});
}

// One round of a stage.  Every wave issues its pieces of the next part FIRST (`more`: there is one): a part issued behind a burst
// lands late in the round or not before its barrier.  Then, for a wave with a tile (ACT; a wave without one only feeds the ring and
// meets the barriers): before() -- loads that the burst hides --, the MFMA burst mma() on the current slot, and in an image's last
// part after() -- the stage's epilogue, or this wave's loads for the next stage, which fly while the partner wave of the SIMD
// multiplies.  KEEP: before() and after() return how many vector-memory instructions they issued, and the barrier is PanelRing's
// counted wait; else the barrier is the full wait of the GRU backward.
// (The forward GRU spells the ring and this round out in its own text, with GGNN_PANEL_DMA_FIRST's early / late-wave choice: see there.)
template <int part, int PARTS, bool ACT, bool KEEP, class Ring, class Before, class Mma, class After>
__device__ __forceinline__ void panel_round(Ring& ring, bool more, const float* nsrc, Before&& before, Mma&& mma, After&& after) {
    int keep = 0;
    if (more) ring.fill_next(nsrc);
    if constexpr (ACT && KEEP) keep += before();
    else if constexpr (ACT) before();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ACT) mma();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (ACT && part == PARTS - 1) {
        if constexpr (KEEP) keep += after();
        else after();
    }
    if constexpr (KEEP) ring.publish_keep(keep);
    else ring.publish();
}

// ---- who works which 16-row tile ------------------------------------------------------------------------------------------------------
// Pass walk (GCN layer, R-GCN cell, ring transform): a workgroup's pass takes NW consecutive tiles, one per wave; its passes are
// `stride` tiles apart.  run_pass(ACT, tile, first_pass, last_pass); ACT = false_type: this wave has no tile in the pass.
template <int NW>
struct PanelPassWalk {
    int n_tiles, base, stride, n_pass;
    __device__ __forceinline__ PanelPassWalk(int n_tiles_, int first_wg, int n_wg)
        : n_tiles(n_tiles_), base(first_wg * NW), stride(n_wg * NW),
          n_pass(base < n_tiles ? (n_tiles - base + stride - 1) / stride : 0) {}      // (wave 0 has a tile in each)
    template <class F>
    __device__ __forceinline__ void run(int wave, F&& run_pass) const {
#pragma unroll 1
        for (int pass = 0; pass < n_pass; ++pass) {
            const int idx = base + pass * stride + wave;
            if (idx < n_tiles) run_pass(std::true_type{}, idx, pass == 0, pass + 1 == n_pass);
            else run_pass(std::false_type{}, idx, pass == 0, pass + 1 == n_pass);
        }
    }
};

// Ticket walk (the two GRU kernels): workgroup b works tickets b, b + nb, ..; full rounds of NW tiles per workgroup first, then the
// rest spread thin over all workgroups (tail_w tiles each).
template <int NW>
struct PanelTickets {
    int wt_total, full_tk, tail_w, n_tk;
    __device__ __forceinline__ PanelTickets(int V, int nb) {
        wt_total = (V + 15) / 16;
        full_tk = wt_total / (NW * nb) * nb;
        const int rest = wt_total - full_tk * NW;
        tail_w = (rest + nb - 1) / nb;
        n_tk = full_tk + (tail_w ? (rest + tail_w - 1) / tail_w : 0);
    }
    // the tile of `wave` in ticket t, -1: none.  same_tile: a tail ticket names ONE tile for every wave (the cooperative tail)
    __device__ __forceinline__ int tile_of(int t, int wave, bool same_tile = false) const {
        if (t < full_tk) return t * NW + wave;
        if (t >= n_tk) return -1;
        if (same_tile) return full_tk * NW + (t - full_tk);
        const int tl = full_tk * NW + (t - full_tk) * tail_w + wave;
        return (wave < tail_w && tl < wt_total) ? tl : -1;
    }
};

// ---- the gather of a pass-walk kernel ---------------------------------------------------------------------------------------------------
// gathered rows in flight per lane while it aggregates: the aggregate is D / 4 registers and so is every row (D = 256: 64 + 2 x 64;
// 192: 48 + 3 x 48; 128: 32 + 4 x 32).  One more at D = 192 / 256 spills (8 / 28 B of scratch per lane).
template <int D>
constexpr int panel_rows_in_flight() { return D <= 128 ? 4 : (D <= 192 ? 3 : 2); }

// slots [beg, end) in order: gather(N, k) adds the rows of slots k .. k+N-1, N = rows in flight, then 2, then 1
template <int D, class G>
__device__ __forceinline__ void panel_gather_ladder(int beg, int end, G&& gather) {
    constexpr int RF = panel_rows_in_flight<D>();
    int k = beg;
    for (; k + RF <= end; k += RF) gather(std::integral_constant<int, RF>{}, k);
    if constexpr (RF > 2) {
        if (k + 2 <= end) { gather(std::integral_constant<int, 2>{}, k); k += 2; }
    }
    if (k < end) gather(std::integral_constant<int, 1>{}, k);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
constexpr int kPanelNW = 8;                            // waves per workgroup: one workgroup per CU, 2 waves per SIMD
constexpr bool panel_hidden_ok(int D) { return D == 128 || D == 192 || D == 256; }

// fn(integral_constant<int, D>) for a D that panel_hidden_ok
template <class F>
auto panel_for_D(int D, F&& fn) {
    switch (D) {
        case 256: return fn(std::integral_constant<int, 256>{});
        case 192: return fn(std::integral_constant<int, 192>{});
        default: return fn(std::integral_constant<int, 128>{});
    }
}

// workgroups of a launch over `rows` rows: one per CU (the ring is up to 128 KiB and a wave holds up to 256 registers), no more than
// there are groups of `tiles_per_wg` 16-row tiles
inline int panel_blocks(long long rows, int tiles_per_wg) {
    const long long n_tiles = (rows + 15) / 16;
    return (int)std::min<long long>((n_tiles + tiles_per_wg - 1) / tiles_per_wg, (long long)num_cus());
}

// launch of a kernel with `lds` bytes of dynamic LDS, opted in once per device where it exceeds `optin_above`
template <auto Kernel, class... Args>
int panel_launch(size_t lds, size_t optin_above, int blocks, hipStream_t st, Args... args) {
    static std::atomic<unsigned long long> lds_ok{0};
    if (lds > optin_above) GGNN_CHECK_HIP(allow_dynamic_lds(Kernel, lds, lds_ok));
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(kPanelNW * 64), lds, st, args...);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}

}  // namespace ggnn
