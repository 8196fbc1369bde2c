// The fused GRU forward's instantiations as ONE table of cells, and the launch description the selection function reads.
//
// gru_select() (ggnn_gru_fused.hip) is the one function that decides which instantiation a launch runs: gru_fused_dispatch()
// launches the cell it returns, ggnn_gru_describe() reports it, ggnn_gru_cells() lists the tables below.  Each translation unit
// instantiates its kernels FROM its table (the launch switches expand the same X-macros), so a kernel that is not in a table is
// not compiled and one that is can be asked for by name (tests/test_gru_fwd_ref_host.py, tests/test_gpu_gru_fwd_cells.py).
#pragma once
#include <cstdint>
#include <cstdlib>

namespace ggnn {

// kernel families
constexpr int kGruRing = 0;      // ggnn_gru_fused_kernel, split matrix path (ggnn_gru_fused_split.hip), ticket source tested at run time
constexpr int kGruHot = 1;       // the same kernel with ticket source and gather parameters fixed at compile time (TK, G4AVG)
constexpr int kGruWide = 2;      // ggnn_gru_wide_kernel (ggnn_gru_wide.hip)
constexpr int kGruPanel = 3;     // ggnn_gru_panel_kernel (ggnn_panel.hip), hidden sizes 128 / 192 / 256
constexpr int kGruF32 = 4;       // ggnn_gru_fused_kernel on the f32 MFMA (GGNN_MATRIX=f32)

// ticket source of a fused GRU instantiation (the kernel's TK)
constexpr int kTkRuntime = -1, kTkStatic = 0, kTkCounter = 1;
// operand formats as cell fields (ggnn_split.hpp: kSplitBf16x3 = 3, kSplitF16x2 = 2); 0: the f32 MFMA
constexpr int kGruFmtF32 = 0, kGruFmtF16x2 = 2, kGruFmtBf16x3 = 3;

// One instantiation.  NW: waves per workgroup; FORM: 0 / 1 / 2 the ring forms, 6 / 61 / 64 the wide kernel's; SAVE / SAVEX: the
// instantiation stores r, u, c / the gathered segment; NTW: 16-row tiles per wave and pass; HALF: the stage images travel as halves
// (ring forms 1 / 2, wide form 64).
struct GruCell { int family, D, NX, NW, FORM, FMT, SAVE, SAVEX, GATHER, TK, G4AVG, NTW, HALF; };
constexpr int kGruCellFields = 13;

constexpr uint64_t gru_cell_key(int family, int D, int NX, int NW, int FORM, int FMT, int SAVE, int SAVEX, int GATHER, int TK,
                                int G4AVG, int NTW, int HALF) {
    uint64_t k = (uint64_t)family;
    k = k * 512 + (uint64_t)D;
    k = k * 4 + (uint64_t)NX;
    k = k * 16 + (uint64_t)NW;
    k = k * 128 + (uint64_t)FORM;
    k = k * 4 + (uint64_t)FMT;
    k = k * 2 + (uint64_t)(SAVE != 0);
    k = k * 2 + (uint64_t)(SAVEX != 0);
    k = k * 2 + (uint64_t)(GATHER != 0);
    k = k * 4 + (uint64_t)(TK + 1);
    k = k * 2 + (uint64_t)(G4AVG != 0);
    k = k * 8 + (uint64_t)NTW;
    k = k * 2 + (uint64_t)(HALF != 0);
    return k;
}
inline uint64_t gru_cell_key(const GruCell& c) {
    return gru_cell_key(c.family, c.D, c.NX, c.NW, c.FORM, c.FMT, c.SAVE, c.SAVEX, c.GATHER, c.TK, c.G4AVG, c.NTW, c.HALF);
}

// ---- ring: X(D, NX, NW, SAVE, GATHER, SAVEX, FORM, FMT) -- the plain launch (one instantiation, its stores skipped at run time
// without save buffers) and the gather-fused launch in ring forms 0 / 1 / 2, each as a training and an inference instantiation
#define GGNN_GRU_RING_NX(X, D, FMT, NX)                                                                                      \
    X(D, NX, 8, true, false, true, 0, FMT)                                                                                   \
    X(D, NX, 8, true, true, true, 0, FMT) X(D, NX, 8, false, true, false, 0, FMT)                                            \
    X(D, NX, 4, true, true, true, 1, FMT) X(D, NX, 4, false, true, false, 1, FMT)                                            \
    X(D, NX, 8, true, true, true, 2, FMT) X(D, NX, 8, false, true, false, 2, FMT)
#define GGNN_GRU_RING_D(X, D)                                                                                                \
    GGNN_GRU_RING_NX(X, D, 2, 1) GGNN_GRU_RING_NX(X, D, 2, 2) GGNN_GRU_RING_NX(X, D, 2, 3)                                   \
    GGNN_GRU_RING_NX(X, D, 3, 1) GGNN_GRU_RING_NX(X, D, 3, 2) GGNN_GRU_RING_NX(X, D, 3, 3)
#define GGNN_GRU_RING_TABLE(X) GGNN_GRU_RING_D(X, 32) GGNN_GRU_RING_D(X, 64) GGNN_GRU_RING_D(X, 100)

// ---- hot: X(NX, NW, FORM, FMT, TK) -- hidden size 100, inference, T = 4, mean aggregation, in the forms the default policy picks
#define GGNN_GRU_HOT_TK(X, NX, NW, FORM, FMT) X(NX, NW, FORM, FMT, 0) X(NX, NW, FORM, FMT, 1)
#define GGNN_GRU_HOT_TABLE(X)                                                                                                \
    GGNN_GRU_HOT_TK(X, 1, 4, 1, 2) GGNN_GRU_HOT_TK(X, 2, 4, 1, 2) GGNN_GRU_HOT_TK(X, 3, 4, 1, 2)                             \
    GGNN_GRU_HOT_TK(X, 1, 4, 1, 3) GGNN_GRU_HOT_TK(X, 2, 4, 1, 3) GGNN_GRU_HOT_TK(X, 3, 4, 1, 3)                             \
    GGNN_GRU_HOT_TK(X, 1, 8, 0, 3)

// ---- f32: X(D, NX, SAVE, GATHER)
#define GGNN_GRU_F32_NX(X, D, NX) X(D, NX, true, true) X(D, NX, false, true) X(D, NX, true, false) X(D, NX, false, false)
#define GGNN_GRU_F32_D(X, D) GGNN_GRU_F32_NX(X, D, 1) GGNN_GRU_F32_NX(X, D, 2) GGNN_GRU_F32_NX(X, D, 3)
#define GGNN_GRU_F32_TABLE(X) GGNN_GRU_F32_D(X, 32) GGNN_GRU_F32_D(X, 64) GGNN_GRU_F32_D(X, 100)

// ---- wide: X(NX, NTW, FMT, NW, HALF, FORM) -- hidden size 100, the inference launch of the tanh cell (each instantiation is
// 2 NTW unrolled pass bodies: minutes of compile time apiece).
// GGNN_WIDE_SET: 1 = nx 1 in the two-piece f16 format only (kernel experiments), 2 = + the residual fan-ins, 3 = + bf16x3.
#ifndef GGNN_WIDE_SET
#define GGNN_WIDE_SET 1
#endif
#ifndef GGNN_WIDE_BF16
#define GGNN_WIDE_BF16 0      // 1: also nx 1 in the exact bf16x3 format (experiments)
#endif
#if GGNN_WIDE_SET >= 2
#define GGNN_GRU_WIDE_SET2(X) X(2, 2, 2, 4, false, 6) X(3, 2, 2, 4, false, 6)
#else
#define GGNN_GRU_WIDE_SET2(X)
#endif
#if GGNN_WIDE_SET >= 3
#define GGNN_GRU_WIDE_SET3(X) X(1, 2, 3, 4, false, 6) X(2, 2, 3, 4, false, 6) X(3, 1, 3, 4, false, 6)
#elif GGNN_WIDE_BF16
#define GGNN_GRU_WIDE_SET3(X) X(1, 1, 3, 8, false, 61) X(1, 2, 3, 4, false, 6)
#else
#define GGNN_GRU_WIDE_SET3(X)
#endif
#define GGNN_GRU_WIDE_TABLE(X)                                                                                               \
    X(1, 2, 2, 4, false, 6) X(1, 1, 2, 8, false, 61) X(1, 1, 2, 4, true, 64) GGNN_GRU_WIDE_SET2(X) GGNN_GRU_WIDE_SET3(X)

// ---- panel: X(D, NX, SAVE, FMT) -- FMT 0: the f32 MFMA form
#define GGNN_GRU_PANEL_NX(X, D, NX) X(D, NX, true, 0) X(D, NX, false, 0) X(D, NX, true, 3) X(D, NX, false, 3) X(D, NX, true, 2) X(D, NX, false, 2)
#define GGNN_GRU_PANEL_D(X, D) GGNN_GRU_PANEL_NX(X, D, 1) GGNN_GRU_PANEL_NX(X, D, 2) GGNN_GRU_PANEL_NX(X, D, 3)
#define GGNN_GRU_PANEL_TABLE(X) GGNN_GRU_PANEL_D(X, 128) GGNN_GRU_PANEL_D(X, 192) GGNN_GRU_PANEL_D(X, 256)

// the tables' entries as cells (the launch switches build their case labels from the same expressions)
#define GGNN_GRU_RING_CELL(D, NX, NW, SAVE, GATHER, SAVEX, FORM, FMT) kGruRing, D, NX, NW, FORM, FMT, SAVE, SAVEX, GATHER, kTkRuntime, false, 1, (FORM) != 0
#define GGNN_GRU_HOT_CELL(NX, NW, FORM, FMT, TK) kGruHot, 100, NX, NW, FORM, FMT, false, false, true, TK, true, 1, (FORM) != 0
#define GGNN_GRU_F32_CELL(D, NX, SAVE, GATHER) kGruF32, D, NX, 8, 0, kGruFmtF32, SAVE, SAVE, GATHER, kTkRuntime, false, 1, false
#define GGNN_GRU_WIDE_CELL(NX, NTW, FMT, NW, HALF, FORM) kGruWide, 100, NX, NW, FORM, FMT, false, false, true, kTkRuntime, false, NTW, HALF
#define GGNN_GRU_PANEL_CELL(D, NX, SAVE, FMT) kGruPanel, D, NX, 8, 0, FMT, SAVE, false, false, kTkRuntime, false, 1, false

// What the selection reads of a launch.  form: the ring form override (-1: the library's default per fan-in and format).
struct GruLaunchDesc {
    int D, nx, fmt;                  // fmt: GGNN_GRU_FMT_* of the launch (0 = BF16X3)
    bool gather, save, save_x;       // gather-fused launch; save_r / save_u / save_c given; the gathered segment saved too
    int act, use_avg, T;
    bool tickets;                    // a ticket counter is given
    int form;
    bool matrix_split, nosave_kernel;
};

// the launch geometry of a cell: waves per workgroup, rows a workgroup takes per pass, workgroups per CU (the grid is
// min(wg_per_cu x CUs, 16-row tiles)), and whether the grid grows to one tile per workgroup when the tiles are more than that
// but at most twice as many (ring form 0's cooperative small launch)
struct GruGeometry { int waves, rows_per_pass, wg_per_cu, coop_small; };

int gru_select(const GruLaunchDesc& d, GruCell& cell, GruGeometry& geom);
bool gru_has_cell(const GruCell& c);
bool gru_wide_supported(int D, int nx, const GruLaunchDesc& d);

// GGNN_GRU_COOP_SMALL=0: few-tile launches of form 0 keep one workgroup per CU (experiments)
inline int gru_coop_small() {
    static const int v = [] { const char* e = getenv("GGNN_GRU_COOP_SMALL"); return e ? atoi(e) : 1; }();
    return v;
}

}  // namespace ggnn
