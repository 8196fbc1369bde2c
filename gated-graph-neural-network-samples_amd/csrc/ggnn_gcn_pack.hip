// Sparse GCN batch assembly from dataset-level tables (the step before the GCN layers: chem_tensorflow_gcn.py:154-196).
//
// A_hat of a batch is the block-diagonal concatenation of the molecules' blocks, shifted by the batch's node offsets, and so is its
// transpose.  The CSR of the whole dataset (ops.gcn_csr_host run ONCE over all graphs with global node ids) therefore holds every
// batch's rows already, in the order gcn_csr_host would give them for that batch (a stable sort by row of row-major lists): a batch
// copies each graph's rows, entries and annotations and shifts the indices.  No sort, no scan, no device->host read.
//
// The node and entry offsets of the graphs in the batch come from prefix sums over the epoch's order, formed on the device once per
// epoch (ggnn_pack_batch_tables with rows = node counts, entry counts): offset of position p = cum[p] - cum[s] for a batch [s, e).
// One wave per graph (molecules average 18 atoms, ~54 entries): its h0 rows, CSR rows and entries are contiguous runs of the outputs.
#include "ggnn_common.h"

namespace ggnn {

struct GCNPackTables {                   // dataset level (device pointers)
    const int* node_ptr;                 // [Gd+1] first node of every graph
    const float* feat; int A;            // [Nd, A] node annotations
    const int* row_ptr; const int* col; const float* val;          // A_hat, CSR over global node ids
    const int* row_ptr_t; const int* col_t; const float* val_t;    // A_hat^T, the same
    const float* targets; int num_targets;                         // [Gd, num_targets]
    const float* label_mask;             // [Gd, K] or NULL (all ones)
    const long long* task_ids; int K;    // [K] target column of each task
    int Gd;
};

struct GCNPackBatch {
    const int* gid;                      // [Ge] epoch order (int32)
    const int* node_cum;                 // [Ge+1] nodes of the epoch's graphs before position p
    const int* entry_cum;                // [Ge+1] entries of the same
    int s, G, V, nnz, D;
};

struct GCNPackOut {
    float* h0;
    int* row_ptr; int* col; float* val;
    int* row_ptr_t; int* col_t; float* val_t;
    int* gnl; int* graph_ptr; long long* node_uid;
    float* tv; float* tm;                // [K, G]
};

// one graph's CSR rows [n] and entries [ne]: rows shifted by (batch first entry - dataset first entry), columns by the node offsets.
// (A_hat is block-diagonal: the graph's block holds its ne entries in A_hat and in A_hat^T alike.)
__device__ __forceinline__ void copy_csr(const int* __restrict__ rp_ds, const int* __restrict__ col_ds, const float* __restrict__ val_ds,
                                         int n0, int n, int ne, int no, int eo, int lane, int* __restrict__ rp, int* __restrict__ col,
                                         float* __restrict__ val) {
    const int e0 = rp_ds[n0];
    for (int i = lane; i < n; i += 64) rp[no + i] = rp_ds[n0 + i] - e0 + eo;
    for (int j = lane; j < ne; j += 64) {
        col[eo + j] = col_ds[e0 + j] - n0 + no;
        val[eo + j] = val_ds[e0 + j];
    }
}

template <bool kVec4>
__global__ __launch_bounds__(256) void gcn_pack_batch_kernel(GCNPackTables ds, GCNPackBatch b, GCNPackOut o) {
    const int k = (int)((blockIdx.x * 256u + threadIdx.x) >> 6);        // graph of this wave (k == G: the closing entries)
    const int lane = threadIdx.x & 63;
    if (k > b.G) return;
    if (k == b.G) {
        if (lane == 0) {
            o.row_ptr[b.V] = b.nnz;
            o.row_ptr_t[b.V] = b.nnz;
            o.graph_ptr[b.G] = b.V;
        }
        return;
    }
    const int p = b.s + k;
    const int g = b.gid[p];
    const int no = b.node_cum[p] - b.node_cum[b.s];
    const int eo = b.entry_cum[p] - b.entry_cum[b.s];
    const int n = b.node_cum[p + 1] - b.node_cum[p];
    const int ne = b.entry_cum[p + 1] - b.entry_cum[p];
    if (g < 0 || g >= ds.Gd) return;
    const int n0 = ds.node_ptr[g];
    // (the host sized the outputs from its own copies of the same counts; a disagreement writes nothing out of bounds)
    if (n != ds.node_ptr[g + 1] - n0 || no < 0 || no + n > b.V || eo < 0 || eo + ne > b.nnz) return;
    if (lane == 0) o.graph_ptr[k] = no;
    for (int i = lane; i < n; i += 64) {
        o.gnl[no + i] = k;
        o.node_uid[no + i] = ((long long)g << 20) + i;               // the state-dropout row key of pack_batch
    }
    copy_csr(ds.row_ptr, ds.col, ds.val, n0, n, ne, no, eo, lane, o.row_ptr, o.col, o.val);
    copy_csr(ds.row_ptr_t, ds.col_t, ds.val_t, n0, n, ne, no, eo, lane, o.row_ptr_t, o.col_t, o.val_t);
    for (int t = lane; t < ds.K; t += 64) {                             // masked labels are fed as 0 (chem_tensorflow_gcn.py:175-177)
        const float m = ds.label_mask ? ds.label_mask[(size_t)g * ds.K + t] : 1.0f;
        const float y = ds.targets[(size_t)g * ds.num_targets + ds.task_ids[t]];
        o.tv[(size_t)t * b.G + k] = m > 0.0f ? y : 0.0f;
        o.tm[(size_t)t * b.G + k] = m;
    }
    // h0 rows [no, no + n): the annotations zero-padded to D, one contiguous run of n * D floats
    const int A = ds.A, D = b.D;
    const float* __restrict__ src = ds.feat + (size_t)n0 * A;
    if constexpr (kVec4) {
        const int D4 = D >> 2;
        f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(o.h0 + (size_t)no * D);
        const int total = n * D4;
        for (int f = lane; f < total; f += 64) {
            const int r = f / D4, c = (f - r * D4) * 4;
            const float* row = src + (size_t)r * A;
            f32x4 v;
            v.x = c < A ? row[c] : 0.0f;
            v.y = c + 1 < A ? row[c + 1] : 0.0f;
            v.z = c + 2 < A ? row[c + 2] : 0.0f;
            v.w = c + 3 < A ? row[c + 3] : 0.0f;
            dst[f] = v;
        }
    } else {
        float* __restrict__ dst = o.h0 + (size_t)no * D;
        const int total = n * D;
        for (int f = lane; f < total; f += 64) {
            const int r = f / D, c = f - r * D;
            dst[f] = c < A ? src[(size_t)r * A + c] : 0.0f;
        }
    }
}

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_gcn_assemble_batch(const void* const* ds_tables, int Gd, int A, int num_targets, const int64_t* task_ids, int K,
                                       const int32_t* epoch_tab, int Ge, int s, int G, int V, int nnz, int D, void* const* out,
                                       ggnn_stream_t stream) {
    GGNN_CHECK_ARG(Gd >= 0 && A >= 0 && num_targets >= 0 && K >= 0 && Ge >= 0 && G >= 0 && V >= 0 && nnz >= 0 && D > 0 && A <= D,
                   "bad sizes Gd=%d A=%d num_targets=%d K=%d Ge=%d G=%d V=%d nnz=%d D=%d", Gd, A, num_targets, K, Ge, G, V, nnz, D);
    GGNN_CHECK_ARG(s >= 0 && (long long)s + G <= Ge, "batch [%d, %d) outside the epoch's %d graphs", s, s + G, Ge);
    GGNN_CHECK_ARG(G > 0 || (V == 0 && nnz == 0), "an empty batch has no nodes or entries (V=%d nnz=%d)", V, nnz);
    GGNN_CHECK_ARG((long long)V * D < (1LL << 31), "batch too large: V=%d D=%d", V, D);
    GGNN_CHECK_ARG(ds_tables && epoch_tab && out, "null pointer");
    GCNPackTables ds{};
    ds.node_ptr = static_cast<const int*>(ds_tables[0]); ds.feat = static_cast<const float*>(ds_tables[1]); ds.A = A;
    ds.row_ptr = static_cast<const int*>(ds_tables[2]); ds.col = static_cast<const int*>(ds_tables[3]);
    ds.val = static_cast<const float*>(ds_tables[4]); ds.row_ptr_t = static_cast<const int*>(ds_tables[5]);
    ds.col_t = static_cast<const int*>(ds_tables[6]); ds.val_t = static_cast<const float*>(ds_tables[7]);
    ds.targets = static_cast<const float*>(ds_tables[8]); ds.num_targets = num_targets;
    ds.label_mask = static_cast<const float*>(ds_tables[9]);
    ds.task_ids = reinterpret_cast<const long long*>(task_ids); ds.K = K; ds.Gd = Gd;
    GGNN_CHECK_ARG(G == 0 || (ds.node_ptr && ds.row_ptr && ds.row_ptr_t), "null dataset table");
    GGNN_CHECK_ARG(V == 0 || A == 0 || ds.feat, "null node features");
    GGNN_CHECK_ARG(nnz == 0 || (ds.col && ds.val && ds.col_t && ds.val_t), "null dataset entries");
    GGNN_CHECK_ARG(K == 0 || G == 0 || (ds.targets && task_ids), "null label table");
    GCNPackBatch b{};
    b.gid = epoch_tab; b.node_cum = epoch_tab + Ge; b.entry_cum = b.node_cum + (Ge + 1);
    b.s = s; b.G = G; b.V = V; b.nnz = nnz; b.D = D;
    GCNPackOut o{};
    o.h0 = static_cast<float*>(out[0]);
    o.row_ptr = static_cast<int*>(out[1]); o.col = static_cast<int*>(out[2]); o.val = static_cast<float*>(out[3]);
    o.row_ptr_t = static_cast<int*>(out[4]); o.col_t = static_cast<int*>(out[5]); o.val_t = static_cast<float*>(out[6]);
    o.gnl = static_cast<int*>(out[7]); o.graph_ptr = static_cast<int*>(out[8]); o.node_uid = static_cast<long long*>(out[9]);
    o.tv = static_cast<float*>(out[10]); o.tm = static_cast<float*>(out[11]);
    GGNN_CHECK_ARG(o.row_ptr && o.row_ptr_t && o.graph_ptr, "null output");
    GGNN_CHECK_ARG(V == 0 || (o.h0 && o.gnl && o.node_uid), "null node output");
    GGNN_CHECK_ARG(nnz == 0 || (o.col && o.val && o.col_t && o.val_t), "null entry output");
    GGNN_CHECK_ARG(K == 0 || G == 0 || (o.tv && o.tm), "null label output");
    const bool vec4 = D % 4 == 0 && aligned16(o.h0);
    const int blocks = (int)(((long long)G + 1 + 3) / 4);             // 4 waves per block, one per graph (+ one for the closing entries)
    hipStream_t st = (hipStream_t)stream;
    if (vec4)
        hipLaunchKernelGGL(gcn_pack_batch_kernel<true>, dim3(blocks), dim3(256), 0, st, ds, b, o);
    else
        hipLaunchKernelGGL(gcn_pack_batch_kernel<false>, dim3(blocks), dim3(256), 0, st, ds, b, o);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
