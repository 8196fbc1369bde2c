// Shared declarations of the graph-resident dense forward (ggnn_dense_graph.hip: f32 MFMA; ggnn_dense_graph_split.hip: split form).
#pragma once
#include "ggnn_common.h"

namespace ggnn {

struct DenseGraphArgs {
    const float* h0;        // [b, v, D]
    const float* A;         // [b, E, v, v]  A[g,e,dst,src]
    const float* eimg;      // E stage images of W_e            (ggnn_dense_edge_pack_f32; the split kernel: E split images)
    const float* gimg;      // 6 stage images: Wg[x,r] Wg[h,r] Wg[x,u] Wg[h,u] Wc[x] Wc[h]   (dense_gru_pack_kernel)
    const float* ebias;     // [E, D] or NULL
    const float* bg;        // [2D]
    const float* bc;        // [D]
    float* out;             // [b, v, D]
    int b, v, steps;
    unsigned long long* tdbg;   // (debug) s_memtime stamps of workgroup 0, waves 0 and 6: [step][wave sel][8]   (GGNN_DG_TPTR)
    float* saved;           // (training; split kernel only) [6][steps][b v, D]: h_t, x_t, r, u, c, r*h -- or NULL
};

// the backward of the launch above (ggnn_dense_graph_bwd.hip): one workgroup per graph walks the timesteps in reverse
struct DenseGraphBwdArgs {
    const float* d_out;     // [b, v, D]  dL/dh_steps
    const float* A;         // [b, E, v, v]
    const float* img;       // 6 + E transposed split images (dense_bwd_pack)
    const float* saved;     // what the saving forward wrote
    float* d_h0;            // [b, v, D] or NULL
    float* dpc;             // [steps, b v, D]
    float* dpg;             // [steps, b v, 2D] = [dpr | dpu]
    float* dx;              // [steps, b v, D]
    float* dM;              // [steps, b v, E D]
    int b, v, steps;
    unsigned long long* tdbg;   // (debug) s_memtime stamps of workgroup 0, waves 0 and 6: [step][wave sel][8]   (GGNN_DGB_TPTR)
};

// split form (ggnn_dense_graph_split.hip): 1 when the kernel exists for the shape and its LDS blocks fit
int dense_split_supported(int v, int E, int D);
size_t dense_split_edge_bytes(int D, int T);      // bytes of the split section of the edge images: T bf16x3 images, then T f16x2 images
size_t dense_split_gru_bytes(int D);              // ... of the six GRU images, in the split kernel's stage order (both formats)
size_t dense_split_images_offset(int D, int T, int fmt);   // byte offset of the images of format `fmt` inside a split section of T images
int dense_split_pack_edge(const float* W, int T, int D, float* packed, hipStream_t st);
int dense_split_pack_gru(const float* Wg, const float* Wc, int D, float* packed, hipStream_t st);
int dense_split_launch(const DenseGraphArgs& a, int E, int D, int fmt, hipStream_t st);
int dense_bwd_supported(int v, int E, int D);     // the backward kernel exists for the shape and its LDS blocks fit
size_t dense_bwd_packed_bytes(int D, int E);

}  // namespace ggnn
