// Arguments of the fused GRU backward launches, shared by the whole-block kernel (ggnn_gru_bwd_fused.hip: D = 32 / 64 / 100) and
// the column-panel kernel (ggnn_gru_bwd_panel.hip: D = 128 / 192 / 256).
#pragma once
#include "ggnn_common.h"

namespace ggnn {

struct GruBwdArgs {
    const float* g; const float* h; const float* r; const float* u; const float* c;
    float* dpc; float* dpg; float* rh; float* dh;
    float* dx[3];                       // nx outputs [V,D]; the last one is d_incoming (scaled when use_avg)
    const float* nin; int T; int use_avg;
    int nx; int V; int act;
    // optional: g_eff[v] = g[v] + sum over the (up to four) rows gz_heads[v] names of gz -- the per-node sum that closes the
    // PREVIOUS timestep's transform backward (dh[v] += sum_t Z[row(v,t)]), taken on load here instead of by a launch of its own
    const float* gz; const int* gz_heads;
    unsigned long long* tdbg;           // debug: s_memtime stamps of workgroup 0 (-DGGNN_BWD_STAMPS=1 builds only; tools/gru_bwd_timeline.py)
};

// ggnn_gru_bwd_panel.hip
int gru_bwd_panel_supported(int D);
size_t gru_bwd_panel_packed_bytes(int D, int nx);
// Wg / Wc given: (re)build the panel images into `packed` first; a.g == NULL or V == 0: nothing else
int gru_bwd_panel_dispatch(int D, const GruBwdArgs& a, const float* Wg, const float* Wc, float* packed, hipStream_t st);

}  // namespace ggnn
