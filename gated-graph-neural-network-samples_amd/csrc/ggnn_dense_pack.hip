// Dense GGNN batch assembly from dataset-level tables (the step before the dense model: chem_tensorflow_dense.py:175-228, and the
// sparse form DenseGGNNChemModel._compute_for_training derives from the adjacency tensor).
//
// A dense batch gives graph k of the batch the padded node slots k*v .. k*v + v - 1, so every structure of a batch is a
// concatenation of per-graph pieces whose only batch-dependent parts are the node base k*v and, per edge type, the position of the
// graph's messages / compact rows among the batch's: the adjacency block A[k] [T, v, v], the states h0[k] [v, D], the node mask, and
// the sparse form over the b*v nodes -- the type-major message lists in np.nonzero order (type, graph, dst, src), the by-target slots
// (ops.build_message_index), the active (source, type) pairs and the by-source and backward structures of the compacted transform
// (ops.build_compact_sources, ops.CompactBackward).  data_device.dense_tables_host computes every graph's pieces once, in local
// node ids; the per-(graph, type) prefix sums of an epoch's order are formed on the device once per epoch (ggnn_pack_batch_tables);
// a batch is then ONE launch, one workgroup per graph: no sort, no scan, no device->host read.
#include "ggnn_common.h"

namespace ggnn {

constexpr int kDenseMaxTypes = 16;
constexpr int kDenseMaskWords = 4096;    // 16 KiB of LDS: blocks of T*v*v <= 131072 entries build their nonzero pattern there

struct DenseTables {                     // dataset level (device pointers), local node ids inside a graph
    const int* node_ptr;                 // [Gd+1] first node of every graph
    const float* feat; int A;            // [Nd, A] node annotations
    const float* targets; int num_targets;
    const float* label_mask;             // [Gd, K] or NULL (all ones)
    const long long* task_ids; int K;    // [K] target column of each task
    const int* msg_ptr;                  // [Gd+1] first message of every graph
    const int2* msg;                     // [Md] (src, dst), type-major, (dst, src) ascending inside a type
    const float* nin;                    // [Nd, T] incoming messages per type
    const int* in_ptr;                   // [Nd] first by-target slot of a node, inside its graph
    const int* slot_msg;                 // [Md] by-target slot -> message
    const int* pair_ptr;                 // [Gd+1] first active (source, type) pair of every graph   (NULL: no compaction tables)
    const int* pair_node;                // [Pd] pair -> source node, type-major, node ascending
    const int* msg_crow;                 // [Md] message -> rank of its pair among the graph's pairs of its type
    const int* src_ptr;                  // [Nd*T] first by-(source, type) slot of a segment, inside its graph
    const int* src_msg;                  // [Md] by-(source, type) slot -> message
    const int* rows_msg;                 // [Md] position in compact-row order (type, source, dst) -> message
    const int* pair_rows;                // [Pd] first message of a pair in compact-row order, inside the graph's messages of its type
    const int* node_pptr;                // [Nd] first pair of a node in node order, inside its graph
    const int* node_order;               // [Pd] node order (node, type) -> pair
    int Gd, T;
};

struct DenseBatch {
    const int* gid;                      // [Ge] epoch order
    const int* pre;                      // [2T][Ge+1] messages per type, then pairs per type, of the epoch's graphs before position p
    int Ge, s, G, v, D, M, R;
    int type_off[kDenseMaxTypes + 1], type_row_off[kDenseMaxTypes + 1];   // the batch's type-major list offsets
};

struct DenseOut {
    float* h0; float* adj_mat; float* mask; float* tv; float* tm;
    float* nin; int2* adj; int* row_ptr; int* gather_row; int* msg_perm;
    int* pair_node; int* gather_c; int* src_rp; int* src_gather; int* src_msg;
    int* rows_rp; int* rows_gather; int* rows_msg; int* node_rp; int* node_order;
};

template <class F>
__device__ __forceinline__ void store_one(float* __restrict__ out, int f, int cols, F val) {
    const int i = f / cols;
    out[f] = val(f, i, f - i * cols);
}

// out[f] = val(f, i, c) over the flat range f in [0, n) of a [rows, cols] block, (i, c) = divmod(f, cols): 16-byte stores for the
// aligned middle, scalar stores for a head and tail of at most three entries (a block is 16-byte aligned only when k * rows * cols is
// a multiple of 4)
template <class F>
__device__ __forceinline__ void fill_block(float* __restrict__ out, int n, int cols, int tid, F val) {
    const int head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) >> 2));
    for (int f = tid; f < head; f += 256) store_one(out, f, cols, val);
    const int n4 = (n - head) >> 2;
    f32x4* __restrict__ q = reinterpret_cast<f32x4*>(out + head);
    for (int w = tid; w < n4; w += 256) {
        const int f = head + 4 * w;
        int i = f / cols, c = f - i * cols;
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = val(f + e, i, c);
            if (++c == cols) { c = 0; ++i; }
        }
        q[w] = f32x4{x[0], x[1], x[2], x[3]};
    }
    for (int f = head + 4 * n4 + tid; f < n; f += 256) store_one(out, f, cols, val);
}

// type of position x in a type-major list with exclusive offsets off[0..T]  (empty types are skipped)
__device__ __forceinline__ int type_at(const int* off, int T, int x) {
    int t = 0;
    while (t + 1 < T && x >= off[t + 1]) ++t;
    return t;
}

// flat index (t*v + dst)*v + src of the graph's message j: ascending in j (messages are ordered (type, dst, src))
__device__ __forceinline__ int msg_key(const int2* __restrict__ msg, const int* cm, int T, int v, int j) {
    const int2 e = msg[j];
    return (type_at(cm, T, j) * v + e.y) * v + e.x;
}

__global__ __launch_bounds__(256) void dense_pack_batch_kernel(DenseTables ds, DenseBatch b, DenseOut o, int sparse, int compact) {
    __shared__ int s_cm[kDenseMaxTypes + 1], s_cp[kDenseMaxTypes + 1], s_mo[kDenseMaxTypes], s_po[kDenseMaxTypes];
    __shared__ int s_tot[3];             // messages, pairs of the batch's graphs before this one; 1 if the counts agree
    __shared__ unsigned s_bits[kDenseMaskWords];
    const int k = blockIdx.x, tid = threadIdx.x, T = ds.T, v = b.v;
    const long long V = (long long)b.G * v;
    if (k == 0 && tid == 0 && sparse) {                                 // the closing entries
        o.row_ptr[V] = b.M;
        if (compact) {
            o.src_rp[V * T] = b.M;
            o.rows_rp[b.R] = b.M;
            o.node_rp[V] = b.R;
        }
    }
    if (k >= b.G) return;
    const int p = b.s + k;
    const int g = b.gid[p];
    if (g < 0 || g >= ds.Gd) return;                                   // (uniform over the block)
    const int n0 = ds.node_ptr[g], n = ds.node_ptr[g + 1] - n0;
    if (n < 0 || n > v) return;                                         // (the host placed the graph in a bucket of size >= n)
    const int m0 = ds.msg_ptr[g], Mg = ds.msg_ptr[g + 1] - m0;
    const int q0 = compact ? ds.pair_ptr[g] : 0, Pg = compact ? ds.pair_ptr[g + 1] - q0 : 0;
    const int nA = T * v * v;
    const bool in_lds = nA <= kDenseMaskWords * 32;
    if (tid == 0) {
        const int stride = b.Ge + 1;
        int am = 0, ap = 0, mt = 0, pt = 0, ok = 1;
        for (int t = 0; t < T; ++t) {
            const int* pm = b.pre + (size_t)t * stride;
            const int* pp = b.pre + (size_t)(T + t) * stride;
            const int mc = pm[p + 1] - pm[p], pc = pp[p + 1] - pp[p];
            const int mo = pm[p] - pm[b.s], po = pp[p] - pp[b.s];
            s_cm[t] = am; s_cp[t] = ap; s_mo[t] = mo; s_po[t] = po;
            am += mc; ap += pc; mt += mo; pt += po;
            // (the host sized the outputs from its own copies of the same counts; a disagreement writes no sparse part at all)
            if (sparse) ok &= mc >= 0 && mo >= 0 && b.type_off[t] + mo + mc <= b.type_off[t + 1];
            if (compact) ok &= pc >= 0 && po >= 0 && b.type_row_off[t] + po + pc <= b.type_row_off[t + 1];
        }
        s_cm[T] = am; s_cp[T] = ap;
        ok &= am == Mg && (!sparse || mt + Mg <= b.M) && (!compact || (ap == Pg && pt + Pg <= b.R));
        s_tot[0] = mt; s_tot[1] = pt; s_tot[2] = ok;
    }
    if (in_lds)
        for (int w = tid; w < (nA + 31) >> 5; w += 256) s_bits[w] = 0u;
    // ---- labels (chem_tensorflow_dense.py:175-193: a masked label feeds label * 0, mask 0)
    for (int t = tid; t < ds.K; t += 256) {
        const float m = ds.label_mask ? ds.label_mask[(size_t)g * ds.K + t] : 1.0f;
        o.tv[(size_t)t * b.G + k] = ds.targets[(size_t)g * ds.num_targets + ds.task_ids[t]] * m;
        o.tm[(size_t)t * b.G + k] = m;
    }
    // ---- node mask, h0 = annotations zero-padded to [v, D] (:143-153)
    for (int i = tid; i < v; i += 256) o.mask[(size_t)k * v + i] = i < n ? 1.0f : 0.0f;
    const int A = ds.A, D = b.D;
    const float* __restrict__ feat = ds.feat + (size_t)n0 * A;
    fill_block(o.h0 + (size_t)k * v * D, v * D, D, tid,
               [&](int, int i, int c) { return (i < n && c < A) ? feat[(size_t)i * A + c] : 0.0f; });
    __syncthreads();                                                    // (s_cm and friends; the cleared pattern)
    // ---- A[k] [T, v, v] (:30-36), every entry written once: the nonzero pattern in LDS, or a search of the graph's sorted messages
    const int2* __restrict__ msg = ds.msg + m0;
    float* __restrict__ amat = o.adj_mat + (size_t)k * T * v * v;
    if (in_lds) {
        for (int j = tid; j < Mg; j += 256) {
            const int2 e = msg[j];
            if ((unsigned)e.x < (unsigned)n && (unsigned)e.y < (unsigned)n) {
                const int f = (type_at(s_cm, T, j) * v + e.y) * v + e.x;
                atomicOr(&s_bits[f >> 5], 1u << (f & 31));
            }
        }
        __syncthreads();
        fill_block(amat, nA, v, tid, [&](int f, int, int) { return (s_bits[f >> 5] >> (f & 31)) & 1u ? 1.0f : 0.0f; });
    } else {
        fill_block(amat, nA, v, tid, [&](int f, int, int) {
            int lo = 0, hi = Mg;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (msg_key(msg, s_cm, T, v, mid) < f) lo = mid + 1; else hi = mid;
            }
            return lo < Mg && msg_key(msg, s_cm, T, v, lo) == f ? 1.0f : 0.0f;
        });
    }
    if (!sparse || !s_tot[2]) return;
    // ---- the sparse form over the b*v nodes: in-degree table, message lists, by-target slots
    const int base = k * v, mtot = s_tot[0];
    const float* __restrict__ nin = ds.nin + (size_t)n0 * T;
    for (int x = tid; x < v * T; x += 256) o.nin[(size_t)base * T + x] = x < n * T ? nin[x] : 0.0f;
    for (int i = tid; i < v; i += 256) o.row_ptr[base + i] = mtot + (i < n ? ds.in_ptr[n0 + i] : Mg);
    for (int j = tid; j < Mg; j += 256) {
        const int2 e = msg[j];
        const int t = type_at(s_cm, T, j);
        o.adj[b.type_off[t] + s_mo[t] + (j - s_cm[t])] = make_int2(base + e.x, base + e.y);
    }
    for (int q = tid; q < Mg; q += 256) {
        const int j = ds.slot_msg[m0 + q];
        const int t = type_at(s_cm, T, j);
        o.gather_row[mtot + q] = (base + msg[j].x) * T + t;
        o.msg_perm[mtot + q] = b.type_off[t] + s_mo[t] + (j - s_cm[t]);
        if (compact) o.gather_c[mtot + q] = b.type_row_off[t] + s_po[t] + ds.msg_crow[m0 + j];
    }
    if (!compact) return;
    // ---- the compacted transform's rows and the backward's transpose structures
    const int ptot = s_tot[1];
    for (int x = tid; x < Pg; x += 256) {
        const int t = type_at(s_cp, T, x);
        const int r = b.type_row_off[t] + s_po[t] + (x - s_cp[t]);
        o.pair_node[r] = base + ds.pair_node[q0 + x];
        o.rows_rp[r] = b.type_off[t] + s_mo[t] + ds.pair_rows[q0 + x];
    }
    for (int x = tid; x < v * T; x += 256) o.src_rp[(size_t)base * T + x] = mtot + (x < n * T ? ds.src_ptr[(size_t)n0 * T + x] : Mg);
    for (int q = tid; q < Mg; q += 256) {
        const int j = ds.src_msg[m0 + q];
        const int t = type_at(s_cm, T, j);
        o.src_gather[mtot + q] = base + msg[j].y;
        o.src_msg[mtot + q] = b.type_off[t] + s_mo[t] + (j - s_cm[t]);
    }
    for (int x = tid; x < Mg; x += 256) {                               // compact-row order is type-major like the message lists
        const int t = type_at(s_cm, T, x);
        const int pos = b.type_off[t] + s_mo[t] + (x - s_cm[t]);
        const int j = ds.rows_msg[m0 + x];
        o.rows_gather[pos] = base + msg[j].y;
        o.rows_msg[pos] = b.type_off[t] + s_mo[t] + (j - s_cm[t]);
    }
    for (int i = tid; i < v; i += 256) o.node_rp[base + i] = ptot + (i < n ? ds.node_pptr[n0 + i] : Pg);
    for (int x = tid; x < Pg; x += 256) {
        const int pl = ds.node_order[q0 + x];
        const int t = type_at(s_cp, T, pl);
        o.node_order[ptot + x] = b.type_row_off[t] + s_po[t] + (pl - s_cp[t]);
    }
}

}  // namespace ggnn

using namespace ggnn;

extern "C" int ggnn_dense_assemble_batch(const void* const* ds_tables, int Gd, int A, int T, int num_targets, const int64_t* task_ids,
                                         int K, const int32_t* epoch_tab, int Ge, int s, int G, int v, int D, int M, int R,
                                         const int64_t* type_off, const int64_t* type_row_off, int sparse, void* const* out,
                                         ggnn_stream_t stream) {
    GGNN_CHECK_ARG(Gd >= 0 && A >= 0 && num_targets >= 0 && K >= 0 && Ge >= 0 && G >= 0 && M >= 0 && R >= 0,
                   "bad sizes Gd=%d A=%d num_targets=%d K=%d Ge=%d G=%d M=%d R=%d", Gd, A, num_targets, K, Ge, G, M, R);
    GGNN_CHECK_ARG(T >= 1 && T <= kDenseMaxTypes, "num_edge_types %d outside [1, %d]", T, kDenseMaxTypes);
    GGNN_CHECK_ARG(v >= 1 && D > 0 && A <= D, "bad shape v=%d D=%d (annotation size %d)", v, D, A);
    GGNN_CHECK_ARG(s >= 0 && (long long)s + G <= Ge, "batch [%d, %d) outside the epoch's %d graphs", s, s + G, Ge);
    GGNN_CHECK_ARG((long long)G * v * T < (1LL << 31) - 1 && (long long)T * v * v < (1LL << 31) && (long long)v * D < (1LL << 31),
                   "batch too large for 32-bit indices: G=%d v=%d T=%d D=%d", G, v, T, D);
    GGNN_CHECK_ARG(ds_tables && epoch_tab && out, "null pointer");
    DenseTables ds{};
    ds.node_ptr = static_cast<const int*>(ds_tables[0]); ds.feat = static_cast<const float*>(ds_tables[1]); ds.A = A;
    ds.targets = static_cast<const float*>(ds_tables[2]); ds.num_targets = num_targets;
    ds.label_mask = static_cast<const float*>(ds_tables[3]);
    ds.task_ids = reinterpret_cast<const long long*>(task_ids); ds.K = K;
    ds.msg_ptr = static_cast<const int*>(ds_tables[4]); ds.msg = static_cast<const int2*>(ds_tables[5]);
    ds.nin = static_cast<const float*>(ds_tables[6]); ds.in_ptr = static_cast<const int*>(ds_tables[7]);
    ds.slot_msg = static_cast<const int*>(ds_tables[8]); ds.pair_ptr = static_cast<const int*>(ds_tables[9]);
    ds.pair_node = static_cast<const int*>(ds_tables[10]); ds.msg_crow = static_cast<const int*>(ds_tables[11]);
    ds.src_ptr = static_cast<const int*>(ds_tables[12]); ds.src_msg = static_cast<const int*>(ds_tables[13]);
    ds.rows_msg = static_cast<const int*>(ds_tables[14]); ds.pair_rows = static_cast<const int*>(ds_tables[15]);
    ds.node_pptr = static_cast<const int*>(ds_tables[16]); ds.node_order = static_cast<const int*>(ds_tables[17]);
    ds.Gd = Gd; ds.T = T;
    GGNN_CHECK_ARG(G == 0 || (ds.node_ptr && ds.msg_ptr), "null dataset table");
    GGNN_CHECK_ARG(G == 0 || A == 0 || ds.feat, "null node features");
    GGNN_CHECK_ARG(K == 0 || G == 0 || (ds.targets && task_ids), "null label table");
    const bool compact = sparse && ds.pair_ptr != nullptr;
    DenseBatch b{};
    b.gid = epoch_tab; b.pre = epoch_tab + Ge;
    b.Ge = Ge; b.s = s; b.G = G; b.v = v; b.D = D; b.M = sparse ? M : 0; b.R = compact ? R : 0;
    if (sparse) {
        GGNN_CHECK_ARG(type_off && type_off[0] == 0 && type_off[T] == M, "type_off must run from 0 to M=%d", M);
        GGNN_CHECK_ARG(!compact || (type_row_off && type_row_off[0] == 0 && type_row_off[T] == R), "type_row_off must run from 0 to R=%d", R);
        for (int t = 0; t <= T; ++t) {
            GGNN_CHECK_ARG(t == 0 || (type_off[t] >= type_off[t - 1] && (!compact || type_row_off[t] >= type_row_off[t - 1])),
                           "type offsets must not decrease");
            b.type_off[t] = (int)type_off[t];
            b.type_row_off[t] = compact ? (int)type_row_off[t] : 0;
        }
    }
    GGNN_CHECK_ARG(G == 0 || (ds.msg && ds.slot_msg) || !sparse || M == 0, "null message tables");
    GGNN_CHECK_ARG(G == 0 || !sparse || (ds.nin && ds.in_ptr), "null node tables");
    GGNN_CHECK_ARG(!compact || G == 0 || (ds.pair_node && ds.msg_crow && ds.src_ptr && ds.src_msg && ds.rows_msg && ds.pair_rows &&
                                          ds.node_pptr && ds.node_order) || R == 0, "null compaction tables");
    DenseOut o{};
    o.h0 = static_cast<float*>(out[0]); o.adj_mat = static_cast<float*>(out[1]); o.mask = static_cast<float*>(out[2]);
    o.tv = static_cast<float*>(out[3]); o.tm = static_cast<float*>(out[4]);
    o.nin = static_cast<float*>(out[5]); o.adj = static_cast<int2*>(out[6]); o.row_ptr = static_cast<int*>(out[7]);
    o.gather_row = static_cast<int*>(out[8]); o.msg_perm = static_cast<int*>(out[9]);
    o.pair_node = static_cast<int*>(out[10]); o.gather_c = static_cast<int*>(out[11]);
    o.src_rp = static_cast<int*>(out[12]); o.src_gather = static_cast<int*>(out[13]); o.src_msg = static_cast<int*>(out[14]);
    o.rows_rp = static_cast<int*>(out[15]); o.rows_gather = static_cast<int*>(out[16]); o.rows_msg = static_cast<int*>(out[17]);
    o.node_rp = static_cast<int*>(out[18]); o.node_order = static_cast<int*>(out[19]);
    GGNN_CHECK_ARG(G == 0 || (o.h0 && o.adj_mat && o.mask), "null output");
    GGNN_CHECK_ARG(K == 0 || G == 0 || (o.tv && o.tm), "null label output");
    if (sparse) {
        GGNN_CHECK_ARG(o.row_ptr && (G == 0 || o.nin) && (M == 0 || (o.adj && o.gather_row && o.msg_perm)), "null sparse-form output");
        GGNN_CHECK_ARG(!compact || (o.src_rp && o.rows_rp && o.node_rp && (M == 0 || (o.gather_c && o.src_gather && o.src_msg &&
                                    o.rows_gather && o.rows_msg)) && (R == 0 || (o.pair_node && o.node_order))), "null compaction output");
    }
    if (G == 0 && !sparse) return GGNN_OK;
    hipLaunchKernelGGL(dense_pack_batch_kernel, dim3(G > 0 ? G : 1), dim3(256), 0, (hipStream_t)stream, ds, b, o, sparse ? 1 : 0,
                       compact ? 1 : 0);
    GGNN_CHECK_HIP(hipGetLastError());
    return GGNN_OK;
}
