/* ggnn_hip.h -- C ABI of libggnn_hip.so: the MI355X (gfx950) GGNN propagation engine.
 *
 * This is the drop-in boundary for the hot path of microsoft/gated-graph-neural-network-samples:
 * SparseGGNNChemModel.compute_final_node_representations() (chem_tensorflow_sparse.py:117-218) and
 * its dense twin (chem_tensorflow_dense.py:93-117).  The reference has no FFI of its own (it is
 * pure Python on tensorflow==1.3.0); each entry point below replaces the TF op call sites cited
 * next to it.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every pointer is a DEVICE pointer unless the
 *     parameter is documented "host".  The caller owns every buffer; the library allocates nothing.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no device
 *     synchronisation, no allocation, and is safe inside hipGraph capture.
 *   - return 0 on success, <0 on error (GGNN_E_*); ggnn_last_error() gives a thread-local message.
 *     Nothing throws or aborts across the ABI.
 *   - fp32 data, int32 indices (chem_tensorflow_sparse.py:65-71), row-major, rows 16-byte aligned,
 *     D % 4 == 0.  Supported hidden sizes D: multiples of 100, 64 or 32 (GGNN_E_UNSUPPORTED else).  Fused single-launch
 *     kernels exist for D = 32, 64, 100 (whole weight blocks as LDS stage images) and D = 128, 192, 256 (64-column
 *     panels of the weight blocks, ggnn_panel.hip); other sizes run the generic tiled GEMM kernels.
 *   - E_t = 0 and nodes with zero in-degree are valid (chem_tensorflow_sparse.py:346-347).
 */
#ifndef GGNN_HIP_H
#define GGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever the argument contract of an EXISTING entry point changes (not when symbols are added).
 *   2: ggnn_assemble_batch takes 11 output pointers (slot heads), ggnn_sparse_propagate_f32 / ggnn_gru_packed_gather_f32 take the
 *      slot-head table (round 3 changed these while the version still said 1; a caller built against that header must rebuild).
 *   3: (round 5) the operand format of the fused GRU forward is an ARGUMENT of every entry point that packs or consumes its weight
 *      images (`gru_fmt`, GGNN_GRU_FMT_*; see "Operand formats" below) instead of a process-wide environment setting:
 *      ggnn_gru_pack_weights_f32, ggnn_gru_packed_f32, ggnn_gru_packed_gather[_train]_f32, ggnn_sparse_propagate_f32,
 *      ggnn_sparse_train_prepare_f32, ggnn_sparse_train_forward_f32.  ggnn_gru_packed_bytes sizes a buffer for either format.
 *      The compacted message transform takes the format of its edge-weight images the same way: ggnn_edge_weights_pack_f32,
 *      ggnn_msg_transform_compact_f32 (`fmt`), ggnn_sparse_propagate_f32 (`edge_fmt`). */
#define GGNN_ABI_VERSION 3

#define GGNN_OK 0
#define GGNN_E_INVALID (-1)      /* bad argument (null pointer, negative size, misalignment) */
#define GGNN_E_UNSUPPORTED (-2)  /* shape outside the supported set */
#define GGNN_E_WORKSPACE (-3)    /* workspace too small */
#define GGNN_E_HIP (-4)          /* a HIP runtime call failed */
#define GGNN_E_INDEX (-5)        /* index out of range (validated entry points only) */

#define GGNN_ACT_TANH 0          /* chem_tensorflow_sparse.py:75-81 */
#define GGNN_ACT_RELU 1

typedef void* ggnn_stream_t;     /* hipStream_t */

int ggnn_abi_version(void);
const char* ggnn_last_error(void);
/* Matrix path of the fused kernels, fixed per process (environment GGNN_MATRIX, read at the first call):
 *   1 (default)  f32 products as six bf16 MFMA products of operands split exactly into three bf16 pieces (csrc/ggnn_split.hpp):
 *                f32 inputs, f32 accumulation, error bound of an f32 FMA chain, 2.5x the f32 matrix rate of gfx950;
 *   0 (GGNN_MATRIX=f32)  the f32 MFMA forms (v_mfma_f32_16x16x4_f32).
 * Packed weight images (ggnn_*_pack_*) are in the format of the mode and sized by the *_bytes functions. */
int ggnn_matrix_path_is_split(void);
/* Operand formats of the fused GRU FORWARD (ggnn_gru_*_f32 at hidden sizes 32 / 64 / 100 / 128 / 192 / 256) under the split matrix
 * path.  Chosen PER CALL by the `gru_fmt` argument of the entry points that pack or consume the GRU's weight images; an image must be
 * consumed in the format it was packed in.
 *   GGNN_GRU_FMT_BF16X3 (3; 0 means the same)  the EXACT three-piece bf16 split, six products per f32 product (the format of every
 *       other split-form kernel): f32 semantics for every finite f32 input, Inf / NaN stay non-finite.  Valid on ALL inputs.
 *   GGNN_GRU_FMT_F16X2 (2)  every f32 operand as TWO f16 pieces (round to nearest: 22 of its 24 significand bits), THREE f16 MFMA
 *       products per f32 product, f32 accumulation; weights packed x 2^8, activations unscaled.  Half the MFMAs, 48 KiB stage
 *       images.  Measured against f64 its error is below the six-product form's and the f32 MFMA's (tests/test_gpu_split_precision.py)
 *       -- INSIDE ITS OPERAND RANGE, which is a PRECONDITION the caller must establish:
 *           every GRU weight   |w| <= GGNN_F16X2_MAX_WEIGHT      (255.875 = 65504 / 2^8: beyond, the packed f16 piece overflows)
 *           every activation   |a| <= GGNN_F16X2_MAX_ACTIVATION  (65504: x segments, h, hence r*h; beyond, its f16 piece overflows)
 *           and all of them finite.
 *       Outside it the result is NOT the f32 result: an operand beyond the range becomes Inf / NaN pieces and the output non-finite
 *       (nothing is clamped or saturated silently).  ggnn_absmax_f32 below
 *       computes the maxima a caller needs; the Python host layer (formats.py) selects this format only when the bounds are PROVEN
 *       from max|h0|, the weights' maxima, the cell's activation and the aggregation -- and BF16X3 otherwise.
 * Under GGNN_MATRIX=f32 the argument is ignored (f32 MFMA kernels, f32 images).
 * ggnn_gru_forward_format(): the process default of the HOST POLICY (environment GGNN_GRU_FMT, read at the first call): 2 = "auto"
 * (F16X2 where the bounds are proven; the default), 3 = always BF16X3, 0 = the matrix path is not split.  The library's kernels do
 * not read it. */
#define GGNN_GRU_FMT_F16X2 2
#define GGNN_GRU_FMT_BF16X3 3
#define GGNN_F16X2_MAX_WEIGHT 255.875f
#define GGNN_F16X2_MAX_ACTIVATION 65504.0f
int ggnn_gru_forward_format(void);
/* Ring form of the gather-fused GRU launches (ggnn_gru_packed_gather[_train]_f32 and the drivers built on them): every form computes
 * the same products in the same order per accumulator -- results are bit-identical -- they differ in how a pass streams the stage
 * images and how many 16-row tiles a wave owns.  -1: the library's default per (fan-in, operand format); 0 / 1 / 2: the ring forms of
 * csrc/ggnn_gru_fused.hip (8 waves on whole images | two 4-wave workgroups per CU on half images | 8 waves, three half-image
 * slots); 6 / 62: the wide form of csrc/ggnn_gru_wide.hip (one wave per SIMD, two tiles per wave, gate-sequential stages; hidden
 * size 100, inference launch of the tanh cell in the two-piece f16 format -- other launches keep the ring forms), 61 / 64: the same
 * pass body as 8 waves x one tile / as two 4-wave workgroups per CU on half-image rings.  Process default: environment GGNN_GRU_FORM.  Returns the previous setting.  (Tests and experiments: compare forms
 * inside one process.) */
int ggnn_gru_form_set(int form);
/* Which instantiation of the fused GRU forward a launch runs -- the launchers' own selection function, host arithmetic only (never
 * touches the GPU).  The launch: hidden size D, nx input segments, gru_fmt, gather (ggnn_gru_packed_gather[_train]_f32) or plain
 * (ggnn_gru_packed_f32 / ggnn_gru_f32), save (r / u / c buffers given; with gather also the gathered segment), act, and of a gather
 * launch use_avg, T and whether a tile counter is given.  form / matrix_split: the ring form (ggnn_gru_form_set) and 0 or 1 for
 * GGNN_MATRIX = f32 / split; negative = this process's setting.  (GGNN_GRU_NOSAVE_KERNEL is always this process's.)
 * out = the cell {family (0 ring, 1 hot: ticket source and gather parameters fixed at compile time, 2 wide, 3 panel, 4 f32 MFMA), D, NX,
 * NW (waves), FORM, FMT (0 f32 MFMA, else GGNN_GRU_FMT_*), SAVE, SAVEX, GATHER, TK (-1 tested at run time, 0 static tickets, 1
 * counter), G4AVG, NTW (tiles per wave and pass), HALF} and the launch geometry {waves per workgroup, rows a workgroup takes per
 * pass, workgroups per CU -- the grid is min(that x CUs, ceil(V / 16)) --, 1 if the grid grows to ceil(V / 16) when that is at most
 * twice the CU count (ring form 0)}.  Returns what the launch returns for these arguments (0 / GGNN_E_INVALID /
 * GGNN_E_UNSUPPORTED): a form value without an instantiation of its own (63, 65..69) is refused, not run as another kernel.
 * ggnn_gru_cells: the tables of instantiations compiled into this library, 13 cell fields each, into out (up to `capacity` cells; out
 * may be NULL); returns their number. */
int ggnn_gru_describe(int D, int nx, int gru_fmt, int gather, int save, int act, int use_avg, int T, int tickets, int form,
                      int matrix_split, int32_t out[17]);
int ggnn_gru_cells(int32_t* out, int capacity);
/* out[i] = max |x| over the numel[i] floats at ptrs[i], i < n, in one launch per 32 tensors -- the operand-range check of
 * GGNN_GRU_FMT_F16X2.  A NaN anywhere in tensor i gives out[i] = NaN, an Inf gives Inf (the maximum is taken over the bit patterns
 * of |x|), so a host test `out[i] <= bound` fails on every non-finite input.  ptrs / numel: HOST arrays of n DEVICE pointers /
 * element counts (numel[i] == 0 gives 0); out: DEVICE [n] (read it back after synchronising the stream). */
int ggnn_absmax_f32(const float* const* ptrs, const int64_t* numel, int n, float* out, ggnn_stream_t stream);

/* ---- (a-1) message index prep: chem_tensorflow_sparse.py:120-129 -------------------------------
 * The reference concatenates the per-type target columns into message_targets[M] (type ascending,
 * list order).  We additionally bucket the M messages by target with a STABLE sort, so that the
 * segment sum can be done atomics-free with the reference's accumulation order inside each node.
 *
 *   adj        [M,2] int32  the T adjacency lists concatenated in type order, rows (src,dst)
 *   type_off   HOST [T+1]   type t owns rows type_off[t] .. type_off[t+1]-1 ; type_off[T] == M
 *   row_ptr    [V+1] int32  out: messages into node v are slots row_ptr[v] .. row_ptr[v+1]-1
 *   gather_row [M]   int32  out: slot -> src*T + type (row of the [V*T, D] transformed-state matrix)
 *   msg_perm   [M]   int32  out (may be NULL): slot -> original message index
 *   ws         scratch of at least ggnn_csr_workspace_bytes(M, V) bytes
 * Indices are validated on the device: out-of-range src/dst set *err_flag (device int32, may be
 * NULL) to 1 and are clamped, instead of faulting (TF-CPU raises InvalidArgument there).
 */
size_t ggnn_csr_workspace_bytes(int64_t M, int V);
int ggnn_build_target_csr(const int32_t* adj, const int64_t* type_off, int T, int V, int64_t M,
                          int32_t* row_ptr, int32_t* gather_row, int32_t* msg_perm, int32_t* err_flag,
                          void* ws, size_t ws_bytes, ggnn_stream_t stream);

/* The transpose index for the backward pass (a-B): messages bucketed by (src*T + type) -- V*T segments,
 * row_ptr [V*T+1] -- with gather_row[slot] = dst, so that
 *   dH[src*T+type, :] = sum over the messages leaving (src,type) of d_incoming[dst, :]
 * is the SAME gather/segment-sum kernel as the forward pass (ggnn_gather_segment_sum_f32 with V*T
 * segments).  Same workspace size and argument meaning as ggnn_build_target_csr. */
int ggnn_build_source_csr(const int32_t* adj, const int64_t* type_off, int T, int V, int64_t M,
                          int32_t* row_ptr, int32_t* gather_row, int32_t* msg_perm, int32_t* err_flag,
                          void* ws, size_t ws_bytes, ggnn_stream_t stream);

/* ---- (a-3) per-edge-type message transform: chem_tensorflow_sparse.py:160-164 -------------------
 * H[v, t*D:(t+1)*D] = h[v,:] @ W[t]  for all nodes and types in ONE [V,D]x[D,T*D] FP32-MFMA GEMM
 * (transform-first: (h[src]) W == (h W)[src]).
 *   h [V,D] (row stride ldh floats), W [T,D,D] (the reference's reshaped edge_weights, :90),
 *   H [V,T*D] out.
 */
int ggnn_msg_transform_f32(const float* h, int ldh, const float* W, float* H, int V, int D, int T,
                           ggnn_stream_t stream);

/* ---- (a-3, compacted) message transform over the ACTIVE (source node, edge type) pairs only ----------
 * The reference transforms every message row h[src] W_t (M rows, :161-164); a node with several outgoing
 * edges of one type sends the same row several times, and most (node,type) pairs emit nothing.  The
 * active pairs are enumerated once per batch, type-major / node-ascending ("compact rows"):
 *
 *   ggnn_build_compact_sources   src_row_ptr [V*T+1] (row_ptr of ggnn_build_source_csr) ->
 *                                pair_node [R] (compact row -> node; caller sizes it min(M, V*T)),
 *                                pair_id [V*T] ((v*T+t) -> compact row, -1 if inactive),
 *                                type_row_off DEVICE [T+1] (rows of type t are type_row_off[t] .. [t+1]-1)
 *   ggnn_remap_gather_rows       gather_row [M] (src*T+type) -> compact rows, for ggnn_gather_segment_sum_f32
 *   ggnn_msg_transform_compact_f32  Hc[r,:] = h[pair_node[r],:] @ W[type(r)]   (Hc [R,D]; type_row_off on the HOST)
 * Supported hidden sizes: ggnn_msg_transform_compact_supported(D) (32, 64, 100, 128, 192, 256).
 */
int ggnn_msg_transform_compact_supported(int D);
size_t ggnn_compact_workspace_bytes(int V, int T);
int ggnn_build_compact_sources(const int32_t* src_row_ptr, int V, int T, int32_t* pair_node, int32_t* pair_id,
                               int32_t* type_row_off, void* ws, size_t ws_bytes, ggnn_stream_t stream);
int ggnn_remap_gather_rows(const int32_t* gather_row, const int32_t* pair_id, int32_t* gather_row_compact, int64_t M,
                           ggnn_stream_t stream);
size_t ggnn_msg_transform_compact_workspace_bytes(int D, int T);
int ggnn_msg_transform_compact_f32(const float* h, const float* W, const int32_t* pair_node, const int64_t* type_row_off,
                                   float* Hc, void* ws, size_t ws_bytes, int V, int D, int T, int fmt, ggnn_stream_t stream);
/* Which kernel ggnn_msg_transform_compact_f32 launches for (D, T, type_row_off, fmt) IN THIS PROCESS and on what schedule -- the
 * launchers' own selection and schedule functions, host arithmetic only (never touches the GPU; GGNN_MATRIX, GGNN_PANEL_TRANSFORM and
 * GGNN_K1_WG_PER_CU are read once per process).  out [4 + 3 T]:
 *   out[0]  kernel family: GGNN_MSG_TRANSFORM_WHOLE_BLOCK (D = 32 / 64 / 100: a workgroup holds its type's whole D x D image),
 *           GGNN_MSG_TRANSFORM_RING (D = 128 / 192 / 256, split path: the type's column-panel images stream through an LDS ring),
 *           GGNN_MSG_TRANSFORM_STATIONARY (those sizes on the f32 MFMA or with GGNN_PANEL_TRANSFORM=0: one panel image per workgroup)
 *   out[1]  the operand format the products run in: 0 = the f32 MFMA, else GGNN_GRU_FMT_BF16X3 / GGNN_GRU_FMT_F16X2 (the f32 kernels
 *           and the stationary kernel ignore `fmt`; every other value of `fmt` than F16X2 means BF16X3)
 *   out[2]  waves per workgroup;  out[3]  workgroups of the launch (0: no rows, nothing is launched)
 *   per type t, at out[4 + 3 t]: its workgroups (stationary: over all its panels), the most and the fewest 16-row tiles any of its
 *           waves walks (the waves of a type share its tiles round-robin: the two differ by at most one).
 * Returns what the launch returns for these arguments before it looks at a pointer (0 / GGNN_E_INVALID / GGNN_E_UNSUPPORTED). */
#define GGNN_MSG_TRANSFORM_WHOLE_BLOCK 0
#define GGNN_MSG_TRANSFORM_RING 1
#define GGNN_MSG_TRANSFORM_STATIONARY 2
int ggnn_msg_transform_compact_describe(int D, int T, const int64_t* type_row_off, int fmt, int32_t* out);

/* ---- (a-2,a-4..a-7) gather + segment sum + bias + mean: chem_tensorflow_sparse.py:160-162,168,
 *      198-209 ------------------------------------------------------------------------------------
 * out[v,:] = ( sum_{slot in row_ptr[v]..row_ptr[v+1]} Hrows[gather_row[slot], :]
 *              + sum_t nin[v,t]*bias[t,:] )  /  ( sum_t nin[v,t] + 1e-7 )
 * with the bias term only if bias != NULL (:202-204) and the division only if use_avg (:206-209).
 * Nodes without incoming messages get the zero row (tf.unsorted_segment_sum semantics).
 *   Hrows  rows of D floats (H of ggnn_msg_transform_f32 viewed as [V*T, D])
 *   nin    [V,T] fp32 incoming-edge counts (required if bias or use_avg), out [V,D].
 */
int ggnn_gather_segment_sum_f32(const float* Hrows, const int32_t* row_ptr, const int32_t* gather_row,
                                const float* nin, const float* bias, int use_avg, float* out,
                                int V, int D, int T, ggnn_stream_t stream);

/* use_propagation_attention (chem_tensorflow_sparse.py:147-149, 170-196) fused into the segment sum:
 *   score_m = <h[src_m], h[tgt_m]> * type_factors[type_m];  a = per-target softmax of the scores (max-shifted,
 *   denominator + 1e-7);  incoming[v] = sum_m a_m * Hrows[gather_row[m]]  (then bias / mean as above).
 * gather_row must be the dense form src*T + type (ggnn_build_target_csr); h [V,D] are the un-transformed states;
 * type_factors [T] = edge_type_attention_weights (:94-96).  D <= 256. */
int ggnn_gather_segment_sum_attn_f32(const float* Hrows, const float* h, const int32_t* row_ptr, const int32_t* gather_row,
                                     const float* type_factors, const float* nin, const float* bias, int use_avg,
                                     float* out, int V, int D, int T, ggnn_stream_t stream);

/* Slot heads: heads[v] (int32 [V,4], 16-byte aligned) = the gather rows of the first four message slots of node v (-1 = no such
 * slot), built once per batch from (row_ptr, gather_row).  ggnn_gather_segment_sum_heads_f32 is ggnn_gather_segment_sum_f32 with
 * them (bit-identical results): the slot indices of a node arrive with one load that does not depend on row_ptr, so a lane has
 * its source rows in flight after ONE round trip instead of two; accumulate != 0 adds to `out` instead of overwriting it. */
int ggnn_build_slot_heads(const int32_t* row_ptr, const int32_t* gather_row, int32_t* heads, int V, ggnn_stream_t stream);
int ggnn_gather_segment_sum_heads_f32(const float* Hrows, const int32_t* row_ptr, const int32_t* gather_row, const int32_t* heads,
                                      const float* nin, const float* bias, int use_avg, float* out, int V, int D, int T,
                                      int accumulate, ggnn_stream_t stream);

/* Backward of the propagation attention (TF autodiff of chem_tensorflow_sparse.py:170-196), three kernels:
 * ggnn_attn_bwd_target_f32: per target node (by-target index: row_ptr, gather_row = src*T+type, msg_perm = slot -> message id),
 *   from d_att = dL/d(attention-weighted sum) [V,D]: the target-side state gradient dh[v] (+)= sum_e ds_e f_t h[src_e], and per
 *   MESSAGE (indexed by message id): coef_a = softmax weight a_e, coef_s = ds_e f_t, dfac = ds_e <h_src, h_tgt>;
 * ggnn_weighted_segment_sum_f32: out[seg] (+)= sum_slots weights[weight_id[slot]] * rows[gather_row[slot]] -- with the by-source
 *   index it is dH[src,type] = sum a_e d_att[dst] (weights = coef_a) and dh[src] += sum ds_e f_t h[dst] (weights = coef_s);
 * ggnn_range_sum_f32: out[b] = sum values[range_off[b] .. range_off[b+1]) (HOST offsets; d attention factor of type t: messages are
 *   type-major).  All deterministic. */
int ggnn_attn_bwd_target_f32(const float* Hrows, const float* h, const float* d_att, const int32_t* row_ptr,
                             const int32_t* gather_row, const int32_t* msg_perm, const float* type_factors, float* coef_a,
                             float* coef_s, float* dfac, float* dh, int accumulate, int V, int D, int T, ggnn_stream_t stream);
int ggnn_weighted_segment_sum_f32(const float* rows, const int32_t* row_ptr, const int32_t* gather_row, const int32_t* weight_id,
                                  const float* weights, float* out, int accumulate, int num_segments, int D, ggnn_stream_t stream);
int ggnn_range_sum_f32(const float* values, const int64_t* range_off, int num_ranges, float* out, ggnn_stream_t stream);

/* Propagation attention over the rows of the COMPACTED transform (chem_tensorflow_sparse.py:147-149, 170-196; the per-type
 * gathers and matmuls of :160-164 only for the active (source node, type) pairs).  The score <h[src], h[tgt]> * type_factors[type]
 * does not read the transformed rows, so no dense [V, T*D] product is needed:
 * ggnn_gather_segment_sum_attn_compact_f32: ggnn_gather_segment_sum_attn_f32 (same arithmetic, same results) with the message of
 *   slot e taken from Hc[slot_row[e]] -- Hc [R,D] = ggnn_msg_transform_compact_f32's output, slot_row = ggnn_remap_gather_rows'
 *   output -- while slot_pair[e] = src*T + type (ggnn_build_target_csr's gather_row) names the source node and the factor.  The
 *   scores of a target's first 8 slots stay in registers between the max pass and the exp pass: per message one h[src] row and one
 *   Hc row are read.  D <= 256 (GGNN_E_UNSUPPORTED beyond), D % 4 == 0; V == 0 is a no-op; a node without messages gets the zero
 *   row (before bias).  No atomics: deterministic.
 * ggnn_attn_bwd_target_compact_f32: ggnn_attn_bwd_target_f32 (TF autodiff of :170-196, target side) with the same addressing;
 *   outputs as there (coef_a, coef_s, dfac by message id, dh (+)=).
 * ggnn_attn_bwd_source_compact_f32: the SOURCE side of that backward, both transpose gathers in one pass over the messages leaving a
 *   node.  By-(source, type) slots (ggnn_build_source_csr): node u's slots are node_ptr[u] .. node_ptr[u+1]-1 (every T-th entry of
 *   that index's row_ptr), slot_dst = target node, slot_msg = message id, slot_row = compact row of the slot's (source, type) pair
 *   (the slots of one pair are consecutive).  dHc[slot_row] = sum over the pair's slots of coef_a[msg] * d_att[dst] (every compact row
 *   is written: each has a message);  dh[u] += sum over u's slots of coef_s[msg] * h[dst]  (dh NULL: skipped, h / coef_s unused).
 *   Bit for bit ggnn_weighted_segment_sum_f32 over the compact rows' segments, and over the nodes' with accumulate = 1 (same slot
 *   order, acc += w * row, dh's contents added last).  The first 4 slots' indices, coefficients and rows are loaded together.
 *   D <= 256, D % 4 == 0; V == 0 is a no-op.  No atomics: deterministic. */
int ggnn_gather_segment_sum_attn_compact_f32(const float* Hc, const float* h, const int32_t* row_ptr, const int32_t* slot_pair,
                                             const int32_t* slot_row, const float* type_factors, const float* nin,
                                             const float* bias, int use_avg, float* out, int V, int D, int T, ggnn_stream_t stream);
int ggnn_attn_bwd_target_compact_f32(const float* Hc, const float* h, const float* d_att, const int32_t* row_ptr,
                                     const int32_t* slot_pair, const int32_t* slot_row, const int32_t* msg_perm,
                                     const float* type_factors, float* coef_a, float* coef_s, float* dfac, float* dh, int accumulate,
                                     int V, int D, int T, ggnn_stream_t stream);
int ggnn_attn_bwd_source_compact_f32(const float* d_att, const float* h, const int32_t* node_ptr, const int32_t* slot_dst,
                                     const int32_t* slot_msg, const int32_t* slot_row, const float* coef_a, const float* coef_s,
                                     float* dHc, float* dh, int V, int D, ggnn_stream_t stream);

/* tf.unsorted_segment_sum in its general form (chem_tensorflow_sparse.py:198-200, 226-228):
 * out[ids[m],:] += data[m,:] with out zero-filled first; fp32 atomics, any id order.  Used for the
 * readout's per-graph sum and available for un-bucketed message lists. */
int ggnn_unsorted_segment_sum_f32(const float* data, const int32_t* ids, float* out, int64_t M, int D,
                                  int num_segments, ggnn_stream_t stream);

/* ---- (a-R) fused graph-level readout: chem_tensorflow_sparse.py:220-231 + utils.py:39-70 -------------
 * out[g] = sum_{v in graph g} sigmoid([hT[v] | h0[v]] . gate_W + gate_b) * (hT[v] . transform_W + transform_b)
 *   hT, h0 [V,D]; graph_nodes_list [V] int32 (:71, :304); gate_W [2D] (the [2D,1] MLP weight), transform_W [D];
 *   gate_b, transform_b DEVICE [1]; out [num_graphs] (zero-filled by the call).  fp32 atomics (one add per node): the
 *   form for an UNSORTED graph_nodes_list; the models use ggnn_readout_loss_fwd_f32 (deterministic) for batcher output. */
int ggnn_gated_readout_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const float* gate_W,
                           const float* gate_b, const float* transform_W, const float* transform_b, float* out, int V,
                           int D, int num_graphs, ggnn_stream_t stream);

/* ---- (f-2) fused readout + masked loss, forward and backward ------------------------------------------------------------
 * chem_tensorflow_sparse.py:220-231 (gated_regression; dense: chem_tensorflow_dense.py:119-129 with node_mask) +
 * chem_tensorflow.py:158-170 (masked loss / MAE of one task) + utils.py:39-70 (MLP with hid_sizes = []).
 * DETERMINISTIC and atomics-free: graph_nodes_list must be NON-DECREASING (the reference batchers append graph after
 * graph, :297-304), so out[g] is a segmented sum in node order; all cross-block reductions run in a fixed order.
 *
 * ggnn_readout_loss_fwd_f32
 *   hT, h0 [V,D]; graph_nodes_list [V] int32 sorted; graph_ptr [G+1] int32 or NULL (first node of every graph; NULL: found by
 *   binary search); node_mask [V] or NULL (dense model: 0 for padding vertices); gate_W [2D], transform_W [D]; gate_b,
 *   transform_b DEVICE [1]; target, mask [G] or NULL (this task's row of target_values / target_mask)
 *   out [G]:  out[g] = sum_{v in g} sigmoid([hT|h0][v] . gate_W + gate_b) (hT[v] . transform_W + transform_b) (node_mask[v])
 *   node_gate, node_val [V]: the per-node gate and value, kept for the backward pass
 *   stats DEVICE [3] or NULL: sum_g 0.5 diff_g^2, sum_g |diff_g|, sum_g mask_g with diff = (out - target) mask   (:161-166; the
 *   caller divides by (sum mask + 1e-7) -- under data parallelism by the ALL-REDUCED mask count)
 *   ws: ggnn_readout_workspace_bytes(V, D, G) bytes.
 * ggnn_readout_loss_bwd_f32
 *   d_out [G] or NULL (gradient w.r.t. out), d_stats DEVICE [2] or NULL (gradients w.r.t. stats[0] and stats[1]);
 *   d_hT [V,D] written (accumulate = 0) or added to (accumulate != 0: second and later tasks);
 *   d_gate_W [2D], d_gate_b [1], d_transform_W [D], d_transform_b [1] written.  D <= 256. */
size_t ggnn_readout_workspace_bytes(int V, int D, int num_graphs);
int ggnn_readout_loss_fwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const int32_t* graph_ptr,
                              const float* node_mask, const float* gate_W, const float* gate_b, const float* transform_W,
                              const float* transform_b, const float* target, const float* mask, float* out,
                              float* node_gate, float* node_val, float* stats, void* ws, size_t ws_bytes, int V, int D,
                              int num_graphs, ggnn_stream_t stream);
int ggnn_readout_loss_bwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const float* node_mask,
                              const float* gate_W, const float* transform_W, const float* node_gate, const float* node_val,
                              const float* out, const float* target, const float* mask, const float* d_out,
                              const float* d_stats, float* d_hT, int accumulate, float* d_gate_W, float* d_gate_b,
                              float* d_transform_W, float* d_transform_b, void* ws, size_t ws_bytes, int V, int D,
                              int num_graphs, ggnn_stream_t stream);

/* ---- (f-3) multi-task fused readout + masked loss: (f-2) for the K entries of task_ids in one pass ------------------------------
 * chem_tensorflow.py:150-170 runs the gated regression and the masked loss once per task; these entry points compute all K
 * tasks while reading hT and h0 ONCE in the forward and ONCE in the backward, and write d_hT once, whatever K is.  Same f32
 * arithmetic as (f-2), DETERMINISTIC and atomics-free (graph_nodes_list NON-DECREASING); every per-task result (out, stats, the
 * weight and bias gradients) is summed in an order that does not depend on K, so task k of two calls with different K agrees bit
 * for bit.  Tasks >= K are neither read nor written.
 *
 * ggnn_readout_multi_supported(D, K): 1 for D a multiple of 4 in 4..256 and 1 <= K <= 16 (no scratch at any of them), else 0.
 * ggnn_readout_multi_fwd_f32
 *   hT, h0 [V,D]; graph_nodes_list [V] int32 sorted; graph_ptr [G+1] int32 or NULL; node_mask [V] or NULL -- as in (f-2).
 *   gate_W, gate_b, transform_W, transform_b: HOST arrays of K DEVICE pointers (as ggnn_sparse_propagate_f32's per-layer arrays):
 *   gate_W[k] [2D], gate_b[k] [1], transform_W[k] [D], transform_b[k] [1]; gate_W[k] and transform_W[k] 16-byte aligned.
 *   target, mask [K,G] row-major or NULL (mask NULL with a target: all ones)
 *   out [K,G]:  out[k,g] = sum_{v in g} sigmoid([hT|h0][v] . gate_W[k] + gate_b[k]) (hT[v] . transform_W[k] + transform_b[k]) (node_mask[v])
 *   node_gv [V, 2K]: row v = gate[v,0..K) | val[v,0..K), the per-node gate and value of every task, kept for the backward pass
 *   stats DEVICE [K,3] or NULL (needs target): per task sum_g 0.5 diff^2, sum_g |diff|, sum_g mask, diff = (out - target) mask
 *   ws: ggnn_readout_multi_workspace_bytes(V, D, K, G) bytes.
 *   V == 0 with G > 0: out = 0 and the stats of an all-zero prediction.  G == 0: GGNN_OK with zeroed stats.
 * ggnn_readout_multi_bwd_f32
 *   d_out [K,G] or NULL; d_stats DEVICE [K,2] or NULL (gradients w.r.t. stats[k,0] and stats[k,1]);
 *   d_hT [V,D] written (accumulate = 0; zeros when G == 0) or added to (accumulate != 0), once, with the K tasks summed in task
 *   order;
 *   d_gate_W, d_gate_b, d_transform_W, d_transform_b: HOST arrays of K DEVICE destinations ([2D], [1], [D], [1]; any 4-byte
 *   alignment: e.g. the optimizer's flat gradient views), written.
 * Errors: null / misaligned pointers GGNN_E_INVALID, ggnn_readout_multi_supported(D, K) == 0 GGNN_E_UNSUPPORTED, a short workspace
 * GGNN_E_WORKSPACE -- all found before anything is launched. */
int ggnn_readout_multi_supported(int D, int K);
size_t ggnn_readout_multi_workspace_bytes(int V, int D, int K, int num_graphs);
int ggnn_readout_multi_fwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const int32_t* graph_ptr,
                               const float* node_mask, const float* const* gate_W, const float* const* gate_b,
                               const float* const* transform_W, const float* const* transform_b, const float* target,
                               const float* mask, float* out, float* node_gv, float* stats, void* ws, size_t ws_bytes, int V,
                               int D, int K, int num_graphs, ggnn_stream_t stream);
int ggnn_readout_multi_bwd_f32(const float* hT, const float* h0, const int32_t* graph_nodes_list, const float* node_mask,
                               const float* const* gate_W, const float* const* transform_W, const float* node_gv,
                               const float* out, const float* target, const float* mask, const float* d_out,
                               const float* d_stats, float* d_hT, int accumulate, float* const* d_gate_W,
                               float* const* d_gate_b, float* const* d_transform_W, float* const* d_transform_b, void* ws,
                               size_t ws_bytes, int V, int D, int K, int num_graphs, ggnn_stream_t stream);

/* ---- (a-8, a-G) residual concat + GRU node update: chem_tensorflow_sparse.py:211-216 -----------
 * TF-1.3 GRUCell: [r|u] = sigmoid([x|h] Wg + bg); c = act([x | r*h] Wc + bc); h' = u*h + (1-u)*c
 * with x = [x_segs[0] | ... | x_segs[nx-1]] read through nx pointers (no concat is materialised;
 * residual states first, aggregated messages last, :211-212).
 *   x_segs HOST array of nx (1..3) device pointers to [V,D]; h [V,D]; Wg [(nx+1)D, 2D]; bg [2D];
 *   Wc [(nx+1)D, D]; bc [D]; h_out [V,D] (must not alias h);
 *   ws: ggnn_gru_workspace_bytes(V,D) bytes of scratch (r*h and u);
 *   save_r/save_u/save_c: optional [V,D] outputs for a backward pass (NULL to skip).
 */
size_t ggnn_gru_workspace_bytes(int V, int D);
int ggnn_gru_f32(const float* const* x_segs, int nx, const float* h, const float* Wg, const float* bg,
                 const float* Wc, const float* bc, float* h_out, void* ws, size_t ws_bytes,
                 float* save_r, float* save_u, float* save_c, int V, int D, int act,
                 ggnn_stream_t stream);

/* The other two cell types of chem_tensorflow_sparse.py:102-112 (forward):
 *   ggnn_rnn_f32        tf.nn.rnn_cell.BasicRNNCell (:109-110): h' = act([x|h] W + b), W [(nx+1)D, D], b [D]
 *   ggnn_cudnn_gru_f32  tf.contrib.cudnn_rnn.CudnnCompatibleGRUCell (:105-108): gates as GRUCell, then
 *                       c = tanh(x Wcx + bcx + r * (h Wch + bch)); h' = u*h + (1-u)*c
 *                       Wg [(nx+1)D,2D], Wcx [nx*D, D], Wch [D,D]; ws = ggnn_cudnn_gru_workspace_bytes(V,D). */
int ggnn_rnn_f32(const float* const* x_segs, int nx, const float* h, const float* W, const float* b, float* h_out,
                 int V, int D, int act, ggnn_stream_t stream);
size_t ggnn_cudnn_gru_workspace_bytes(int V, int D);
int ggnn_cudnn_gru_f32(const float* const* x_segs, int nx, const float* h, const float* Wg, const float* bg,
                       const float* Wcx, const float* bcx, const float* Wch, const float* bch, float* h_out,
                       void* ws, size_t ws_bytes, int V, int D, ggnn_stream_t stream);

/* Non-zero if ggnn_gru_f32 runs as ONE fused launch for this hidden size (gates -> r*h -> candidate -> blend chained in
 * registers): 1 for D in {32, 64, 100} (whole-block stage images; ggnn_gru_packed_gather_f32 exists for these),
 * 2 for D in {128, 192, 256} (column-panel kernel, ggnn_panel.hip; no gather-fused variant);
 * 0 if it runs as the two launches below (ws is then used). */
int ggnn_gru_is_fused(int D);

/* Pre-packed weights (inference: weights are constant across batches).  The fused GRU and the compacted
 * transform consume k-interleaved LDS stage images of their weights; ggnn_gru_f32 /
 * ggnn_msg_transform_compact_f32 build them in a small pre-pass on every call, the functions below let the
 * caller build them once per weight version:
 *   ggnn_gru_pack_weights_f32   Wg [(nx+1)D,2D], Wc [(nx+1)D,D] -> packed (ggnn_gru_packed_bytes(D,nx) bytes: enough for either
 *                               operand format) in the format gru_fmt (GGNN_GRU_FMT_*, see "Operand formats" at the top)
 *   ggnn_gru_packed_f32         == ggnn_gru_f32 with the packed images instead of Wg / Wc (fused sizes only); gru_fmt = the format
 *                               the images were packed in.  (ggnn_gru_f32 itself, on raw weights, always multiplies in BF16X3.)
 *   ggnn_edge_weights_pack_f32  W [T,D,D] -> packed (ggnn_msg_transform_compact_workspace_bytes(D,T) bytes: enough for either
 *                               operand format), in the format `fmt` (GGNN_GRU_FMT_*; "Operand formats" at the top: BF16X3 is
 *                               exact on every input; F16X2 needs |h| <= 65504 and |W| <= 255.875 PROVEN by the caller --
 *                               forward transforms only; hidden sizes 32 / 64 / 100 and the ring kernel of 128 / 192 / 256);
 *                               then call ggnn_msg_transform_compact_f32 with W = NULL and ws = packed.
 * tile_counter (ggnn_gru_packed_f32, ggnn_gru_packed_gather_f32): NULL, or a DEVICE int32 that is 0 when the launch
 * starts (the kernel leaves it non-zero).  With a counter the 16-row tiles are handed to the workgroups dynamically:
 * same results, but the launch no longer stretches when other streams hold part of the GPU while it starts.  (Hidden sizes
 * 128 / 192 / 256, the panel kernel, deal their tiles statically: the counter is accepted and left untouched.) */
size_t ggnn_gru_packed_bytes(int D, int nx);
int ggnn_gru_pack_weights_f32(const float* Wg, const float* Wc, int nx, int D, int gru_fmt, float* packed, ggnn_stream_t stream);
int ggnn_gru_packed_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* bg,
                        const float* bc, float* h_out, float* save_r, float* save_u, float* save_c, int V, int D, int act,
                        int gru_fmt, int32_t* tile_counter, ggnn_stream_t stream);
int ggnn_edge_weights_pack_f32(const float* W, int T, int D, int fmt, float* packed, ggnn_stream_t stream);

/* GRU with the segment sum fused in (chem_tensorflow_sparse.py:198-216 in one launch, no edge bias): the
 * aggregated-messages input -- the LAST of the nx concatenated inputs -- is gathered inside the kernel,
 *   incoming[v] = (sum over the slots row_ptr[v]..row_ptr[v+1] of Hrows[gather_row[slot]]) / (sum_t nin[v,t] + 1e-7),
 * in the same slot order and arithmetic as ggnn_gather_segment_sum_f32 (bit-identical results), so the separate
 * segment-sum launch and the HBM round trip of `incoming` disappear.  x_segs: the nx-1 residual segments.
 * Hrows must hold at least one row (row 0 is fetched for the unused slots of low-degree nodes); V*T*D < 2^30. */
int ggnn_gru_packed_gather_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* bg,
                               const float* bc, float* h_out, const float* Hrows, const int32_t* row_ptr,
                               const int32_t* gather_row, const float* nin, int T, int use_avg, int V, int D, int act,
                               int gru_fmt, int32_t* tile_counter, ggnn_stream_t stream);
/* The training form of the same launch: r, u, c [V,D] and the gathered segment `incoming` [V,D] (an operand of the weight gradients)
 * are written for the backward pass -- all four pointers or none. */
int ggnn_gru_packed_gather_train_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* bg,
                                     const float* bc, float* h_out, const float* Hrows, const int32_t* row_ptr,
                                     const int32_t* gather_row, const float* nin, int T, int use_avg, float* save_r, float* save_u,
                                     float* save_c, float* save_incoming, int V, int D, int act, int gru_fmt,
                                     int32_t* tile_counter, ggnn_stream_t stream);

/* The two launches of the un-fused ggnn_gru_f32, separately addressable (profiling, large D):
 *   gates:     [r|u] = sigmoid([x|h] Wg + bg) -> rh = r*h [V,D], u [V,D] (save_r optional)
 *   candidate: c = act([x|rh] Wc + bc); h_out = u*h + (1-u)*c            (save_c optional) */
int ggnn_gru_gates_f32(const float* const* x_segs, int nx, const float* h, const float* Wg, const float* bg,
                       float* rh, float* u, float* save_r, int V, int D, ggnn_stream_t stream);
int ggnn_gru_candidate_f32(const float* const* x_segs, int nx, const float* rh, const float* h, const float* u,
                           const float* Wc, const float* bc, float* h_out, float* save_c, int V, int D, int act,
                           ggnn_stream_t stream);

/* ---- (a-9) layer / timestep driver: chem_tensorflow_sparse.py:131-218 -------------------------------
 * The whole forward propagation (every layer and timestep: transform -> gather/segment-sum -> GRU) enqueued
 * by ONE call.  All `const T* const*` parameters are HOST arrays of `num_layers` DEVICE pointers.
 *   row_ptr / gather_row        message index by target (ggnn_build_target_csr); with the compacted transform
 *                               gather_row must be the remapped rows (ggnn_remap_gather_rows)
 *   pair_node, type_row_off     compacted transform (type_row_off on the HOST); both NULL -> dense transform
 *   layer_timesteps             HOST [num_layers]                                  (:53, :131)
 *   res_ptr / res_idx           HOST CSR of residual_connections: layer l reads the states
 *                               res_idx[res_ptr[l] .. res_ptr[l+1]-1] (0 = h0, k = output of layer k-1), :140-145
 *   edge_w [T,D,D] raw and/or edge_packed (ggnn_edge_weights_pack_f32); edge_bias entries may be NULL
 *   Wg/Wc raw and/or gru_packed (ggnn_gru_pack_weights_f32); bg [2D], bc [D]
 *   gru_fmt                     HOST [num_layers] of GGNN_GRU_FMT_*: the format gru_packed[l] was packed in (NULL: BF16X3 for all;
 *                               layers that run on raw weights always multiply in BF16X3)
 *   edge_fmt                    the same for edge_packed[l] (ggnn_edge_weights_pack_f32's fmt; NULL: BF16X3 for all)
 *   layer_out                   HOST [num_layers] of DEVICE [V,D]: node_states_per_layer[l+1]; the last one is
 *                               the function's return value (:218)
 *   fuse_gather                 k > 0: layers with at most k concatenated GRU inputs (residuals + messages; 1 = no
 *                               residual inputs), packed GRU weights, a fused hidden size and no edge bias run 2 launches
 *                               per timestep (transform, ggnn_gru_packed_gather_f32) instead of 3;  0: never
 *   ws                          ggnn_sparse_propagate_workspace_bytes(V, D, T, compact_rows or -1) bytes
 */
size_t ggnn_sparse_propagate_workspace_bytes(int V, int D, int T, int64_t compact_rows);
int ggnn_sparse_propagate_f32(const float* h0, int V, int D, int T,
                              const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node,
                              const int64_t* type_row_off, const float* nin, int use_avg,
                              int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                              const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
                              const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
                              const float* const* gru_packed, const int32_t* gru_fmt, const int32_t* edge_fmt, int act,
                              int fuse_gather, float* const* layer_out, void* ws, size_t ws_bytes, ggnn_stream_t stream);

/* ggnn_sparse_propagate_f32 with use_propagation_attention (chem_tensorflow_sparse.py:131-218 with :147-149, 170-196): per timestep
 * the compacted transform, ggnn_gather_segment_sum_attn_compact_f32 and the GRU (ggnn_gru_packed_f32, or ggnn_gru_f32 for layers
 * without packed images).  The compact form is REQUIRED: pair_node / type_row_off non-NULL, gather_row = the remapped rows
 * (slot_row).  Two more arguments:
 *   slot_pair       the by-target index's own gather rows, src*T + type (ggnn_build_target_csr)
 *   attn_factors    HOST [num_layers] of DEVICE [T]: edge_type_attention_weights per layer (:94-96)
 * fuse_gather is ignored (the attention-weighted sum is never gathered inside the GRU).  Same workspace. */
int ggnn_sparse_propagate_attn_f32(const float* h0, int V, int D, int T,
                                   const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node,
                                   const int64_t* type_row_off, const float* nin, int use_avg,
                                   int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                   const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
                                   const float* const* Wg, const float* const* bg, const float* const* Wc, const float* const* bc,
                                   const float* const* gru_packed, const int32_t* gru_fmt, const int32_t* edge_fmt, int act,
                                   int fuse_gather, float* const* layer_out, void* ws, size_t ws_bytes,
                                   const int32_t* slot_pair, const float* const* attn_factors, ggnn_stream_t stream);

/* ---- BasicRNNCell with the segment sum fused in (the R-GCN configuration of the sparse GGNN) ----------------------------------
 * h' = act([x_0 | .. | x_{nx-2} | incoming | h] W + b) in ONE launch, with
 *   incoming[v] = (sum over the slots row_ptr[v]..row_ptr[v+1] of Hrows[gather_row[slot]]) / (sum_t nin[v,t] + 1e-7)
 * gathered inside the kernel in the slot order and arithmetic of ggnn_gather_segment_sum_f32 without bias (bit-identical; the
 * division only with use_avg).  The nx + 1 weight blocks [D, D] of W [(nx+1)D, D] live in LDS as exact bf16x3 images for the whole
 * launch, so the supported set is what fits 160 KiB:
 *   ggnn_rnn_fused_supported(D, nx)   1 for D in {32, 64} with nx in 1..3 and for D = 100 with nx = 1; 0 otherwise.  Every entry
 *                                     point below returns GGNN_E_UNSUPPORTED (ggnn_rnn_packed_bytes: 0) exactly where it is 0.
 *   ggnn_rnn_packed_bytes / ggnn_rnn_pack_weights_f32   W -> the nx + 1 images, once per weight version
 *   ggnn_rnn_fused_launch_geometry    {rows a workgroup covers per round of its tile loop, the most workgroups a launch starts}
 *   ggnn_rnn_packed_gather_f32        the launch.  x_segs: HOST array of the nx - 1 residual segments [V, D] (may be NULL at
 *                                     nx = 1); Hrows [num_rows, D]; row_ptr [V + 1] (values are clamped to [0, M]); gather_row [M]
 *                                     (a value outside [0, num_rows) contributes nothing and is never dereferenced); nin [V, T]
 *                                     (required with use_avg); save_incoming: NULL, or [V, D] that receives the gathered segment
 *                                     (training; h_out is bit-identical with and without it).  h_out / save_incoming must not alias
 *                                     an input.  No edge bias.  V == 0 is a no-op; V*D or num_rows*D >= 2^30: GGNN_E_UNSUPPORTED. */
int ggnn_rnn_fused_supported(int D, int nx);
size_t ggnn_rnn_packed_bytes(int D, int nx);
int ggnn_rnn_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream);
void ggnn_rnn_fused_launch_geometry(int D, int nx, int* rows_per_workgroup, int* max_workgroups);
int ggnn_rnn_packed_gather_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* b,
                               float* h_out, const float* Hrows, int64_t num_rows, const int32_t* row_ptr,
                               const int32_t* gather_row, int64_t M, const float* nin, int T, int use_avg,
                               float* save_incoming, int V, int D, int act, ggnn_stream_t stream);

/* The same cell at hidden sizes 128 / 192 / 256, where the nx + 1 blocks no longer fit LDS: the (nx + 1) D / 64 COLUMN-PANEL images
 * [D, 64] of W stream through a two-slot LDS-DMA ring (ggnn_rnn_panel.hip; exact bf16x3 only), the K segment outermost, so every
 * operand row is read once whatever nx.  Replaces, per timestep of chem_tensorflow_sparse.py:198-216 with :109-110, the launches
 * ggnn_gather_segment_sum_f32 (incoming [V, D] written to memory) + ggnn_rnn_f32 (which reads it back and re-stages W).  The gather
 * arithmetic, the defensive addressing and the save_incoming contract are ggnn_rnn_packed_gather_f32's, word for word.
 *   ggnn_rnn_panel_supported(D, nx)   1 for D in {128, 192, 256} with nx in 1..3; 0 otherwise (disjoint from
 *                                     ggnn_rnn_fused_supported).  The entry points below return GGNN_E_UNSUPPORTED
 *                                     (ggnn_rnn_panel_packed_bytes: 0, the geometry: 0 / 0) exactly where it is 0.
 *   ggnn_rnn_panel_packed_bytes       (nx + 1) * (D / 64) * (D / 32) * 12288
 *   ggnn_rnn_panel_pack_weights_f32   W [(nx+1)D, D] -> image s * (D / 64) + p = rows s D .., columns 64 p ..; once per weight version
 *   ggnn_rnn_panel_launch_geometry    {rows a workgroup covers per pass, the most workgroups a launch starts}
 *   ggnn_rnn_panel_gather_f32         the launch; the argument list and rules of ggnn_rnn_packed_gather_f32. */
int ggnn_rnn_panel_supported(int D, int nx);
size_t ggnn_rnn_panel_packed_bytes(int D, int nx);
int ggnn_rnn_panel_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream);
void ggnn_rnn_panel_launch_geometry(int D, int nx, int* rows_per_workgroup, int* max_workgroups);
int ggnn_rnn_panel_gather_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* b,
                              float* h_out, const float* Hrows, int64_t num_rows, const int32_t* row_ptr,
                              const int32_t* gather_row, int64_t M, const float* nin, int T, int use_avg,
                              float* save_incoming, int V, int D, int act, ggnn_stream_t stream);

/* The whole BasicRNNCell backward of a timestep in ONE launch (tf autodiff of h' = act([x.. | incoming | h] W + b),
 * chem_tensorflow.py:184 over chem_tensorflow_sparse.py:109-110, with :206-209 for the mean): from g = dL/dh' and the saved out = h'
 *   dP = g * act'(out)  (tanh: 1 - out^2, ReLU: out > 0; bit for bit ggnn_act_bwd_f32);   Q_s = dP W_s^T, W_s = rows sD..(s+1)D of W
 *   dx[s] = Q_s (s < nx-1);  dx[nx-1] = d_incoming = Q_{nx-1} [/ (sum_t nin[v,t] + 1e-7) with use_avg];  dh = Q_nx
 * chained in registers per 16-row tile, the nx + 1 transposed blocks resident in LDS as exact bf16x3 images -- the mirror image of
 * ggnn_rnn_packed_gather_f32, with its supported set, occupancy rule and launch geometry (ggnn_rnn_fused_launch_geometry holds for
 * both).  It replaces ggnn_act_bwd_f32 + ggnn_bwd_dx_f32 (and the transposed copy of W that launch is given).  dP [V,D] is written:
 * it is the dY of the weight-gradient product.
 *   ggnn_rnn_bwd_fused_supported(D, nx)   == ggnn_rnn_fused_supported(D, nx); the entry points below return GGNN_E_UNSUPPORTED
 *                                         (ggnn_rnn_bwd_packed_bytes: 0) exactly where it is 0.
 *   ggnn_rnn_bwd_pack_weights_f32         W [(nx+1)D, D] -> the nx + 1 images of W_s^T, once per weight version
 *   ggnn_rnn_bwd_fused_f32                dx: HOST array of nx device pointers [V,D] (the last one receives d_incoming); nin [V,T] is
 *                                         required with use_avg.  No output may alias an input or another output; every pointer is
 *                                         16-byte aligned.  Rows >= V are neither read nor written.  V == 0 is a no-op; V*D >= 2^30:
 *                                         GGNN_E_UNSUPPORTED.
 *   ggnn_rnn_bwd_fused_gather_f32         ... with g_eff[v] = g[v] + the rows of gz [num_rows, D] named by the int4 slot-head record
 *                                         gz_heads[v] (ggnn_build_slot_heads; an entry of -1 or outside [0, num_rows) adds nothing and
 *                                         is not dereferenced): the meaning of the pair in ggnn_gru_bwd_fused_gather_f32 -- bit for
 *                                         bit ggnn_gather_segment_sum_heads_f32(gz, .., accumulate = 1) into g followed by the plain
 *                                         form, for nodes with at most four rows.  num_rows*D >= 2^30: GGNN_E_UNSUPPORTED. */
int ggnn_rnn_bwd_fused_supported(int D, int nx);
size_t ggnn_rnn_bwd_packed_bytes(int D, int nx);
int ggnn_rnn_bwd_pack_weights_f32(const float* W, int nx, int D, float* packed, ggnn_stream_t stream);
int ggnn_rnn_bwd_fused_f32(const float* g, const float* out, const float* packed, float* dP, float* const* dx, float* dh,
                           const float* nin, int T, int use_avg, int nx, int V, int D, int act, ggnn_stream_t stream);
int ggnn_rnn_bwd_fused_gather_f32(const float* g, const float* gz, const int32_t* gz_heads, int64_t num_rows, const float* out,
                                  const float* packed, float* dP, float* const* dx, float* dh, const float* nin, int T,
                                  int use_avg, int nx, int V, int D, int act, ggnn_stream_t stream);

/* ggnn_sparse_propagate_f32 for graph_rnn_cell = RNN on the compacted transform.  The compact form is REQUIRED (pair_node /
 * type_row_off non-NULL, gather_row = the remapped rows; GGNN_E_INVALID otherwise).  Per timestep: the compacted transform on
 * edge_packed[l] (or raw edge_w[l]), then -- for a layer with rnn_packed[l], ggnn_rnn_fused_supported(D, nx) and no edge bias --
 * ggnn_rnn_packed_gather_f32 (with ggnn_rnn_panel_supported(D, nx) instead: ggnn_rnn_panel_gather_f32, rnn_packed[l] then being
 * ggnn_rnn_panel_pack_weights_f32's images); otherwise ggnn_gather_segment_sum_f32 over the compact rows and ggnn_rnn_f32 on rnn_w[l].
 *   rnn_w [(nx+1)D, D], rnn_b [D], rnn_packed (ggnn_rnn_pack_weights_f32; the array or single entries may be NULL): HOST arrays of
 *   num_layers DEVICE pointers.  M: the length of gather_row.  fuse_gather: as in ggnn_sparse_propagate_f32 (the largest nx that
 *   runs the fused cell; 0: never).  Same workspace as ggnn_sparse_propagate_f32. */
int ggnn_sparse_propagate_rnn_f32(const float* h0, int V, int D, int T,
                                  const int32_t* row_ptr, const int32_t* gather_row, int64_t M, const int32_t* pair_node,
                                  const int64_t* type_row_off, const float* nin, int use_avg,
                                  int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                  const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
                                  const float* const* rnn_w, const float* const* rnn_b, const float* const* rnn_packed,
                                  const int32_t* edge_fmt, int act, int fuse_gather, float* const* layer_out, void* ws,
                                  size_t ws_bytes, ggnn_stream_t stream);

/* ---- CudnnCompatibleGRUCell in one launch (chem_tensorflow_sparse.py:105-108; replaces the three launches of ggnn_cudnn_gru_f32) --
 *     [r|u] = sigmoid([x_0|..|x_{nx-1}|h] Wg + bg);  hc = h Wch + bch;  c = tanh([x_0|..|x_{nx-1}] Wcx + bcx + r * hc)
 *     h'    = u*h + (1-u)*c                              x_{nx-1}: the aggregated messages, an ordinary input segment here
 * The 3 (nx + 1) weight blocks [D, D] stream through a two-slot LDS-DMA ring as exact bf16x3 stage images (ggnn_cudnn_gru_fused.hip);
 * r, u and hc stay in registers.  Accumulation order is fixed (r / u: the x segments in order, h last; cx: the x segments in order;
 * ch: h alone), so h' is bit-identical from run to run and with or without the saves.
 *   ggnn_cudnn_gru_fused_supported(D, nx)  (:102-108) 1 for D in {32, 64, 100} with nx in 1..3; 0 otherwise.  Every entry point below
 *                                          returns GGNN_E_UNSUPPORTED (packed_bytes: 0, the geometry: 0 / 0) exactly where it is 0.
 *   ggnn_cudnn_gru_packed_bytes            (:105-108) 3 (nx + 1) images: 8 KiB each at D = 32, 24 KiB at 64, 72 KiB at 100
 *   ggnn_cudnn_gru_pack_weights_f32        (:105-108) Wg [(nx+1)D, 2D], Wcx [nx D, D], Wch [D, D] -> the images in the pass's stage
 *                                          order: per x segment its r, u and Wcx columns, then for h its r, u columns and Wch.
 *                                          Once per weight version.
 *   ggnn_cudnn_gru_fused_launch_geometry   (:105-108) {rows a workgroup covers per pass, the most workgroups a launch starts}; a
 *                                          workgroup runs the passes blockIdx, blockIdx + workgroups, .. (no counter, no atomics)
 *   ggnn_cudnn_gru_packed_f32              (:105-108) the launch.  x_segs: HOST array of the nx segments [V, D].  save_r / save_u /
 *                                          save_c / save_hc: all NULL, or all [V, D] (training: the tensors the backward reads).
 *                                          Every pointer 16-byte aligned; h_out must not be h or a segment, a save buffer must not be
 *                                          an input, h_out or another save buffer (GGNN_E_INVALID, before anything is launched).
 *                                          V == 0 is a no-op; V*D >= 2^30: GGNN_E_UNSUPPORTED (32-bit byte offsets).
 *                                          Rows >= V are neither read nor written. */
int ggnn_cudnn_gru_fused_supported(int D, int nx);
size_t ggnn_cudnn_gru_packed_bytes(int D, int nx);
int ggnn_cudnn_gru_pack_weights_f32(const float* Wg, const float* Wcx, const float* Wch, int nx, int D, float* packed,
                                    ggnn_stream_t stream);
void ggnn_cudnn_gru_fused_launch_geometry(int D, int nx, int* rows_per_pass, int* max_workgroups);
int ggnn_cudnn_gru_packed_f32(const float* const* x_segs, int nx, const float* h, const float* packed, const float* bg,
                              const float* bcx, const float* bch, float* h_out, float* save_r, float* save_u, float* save_c,
                              float* save_hc, int V, int D, ggnn_stream_t stream);

/* ggnn_sparse_propagate_f32 for graph_rnn_cell = CudnnCompatibleGRUCell (:102-108, 131-218) on the compacted transform.  The compact
 * form is REQUIRED (pair_node / type_row_off non-NULL, gather_row = the remapped rows; GGNN_E_INVALID otherwise).  Per timestep: the
 * compacted transform on edge_packed[l] (or raw edge_w[l]), ggnn_gather_segment_sum_f32 over the compact rows (with the layer's edge
 * bias, if any), then ggnn_cudnn_gru_packed_f32 for a layer with cell_packed[l] and ggnn_cudnn_gru_fused_supported(D, nx), otherwise
 * ggnn_cudnn_gru_f32 on the raw weights (every layer with nx > 3 and every layer at widths 128 / 192 / 256).
 *   wg [(nx+1)D, 2D], bg [2D], wcx [nx D, D], bcx [D], wch [D, D], bch [D], cell_packed (ggnn_cudnn_gru_pack_weights_f32; the array
 *   or single entries may be NULL): HOST arrays of num_layers DEVICE pointers; the raw weight arrays may be NULL when every layer has
 *   packed images.  ws: ggnn_sparse_propagate_cudnn_workspace_bytes (ggnn_sparse_propagate_workspace_bytes plus the composed cell's
 *   ggnn_cudnn_gru_workspace_bytes). */
size_t ggnn_sparse_propagate_cudnn_workspace_bytes(int V, int D, int T, int64_t compact_rows);
int ggnn_sparse_propagate_cudnn_f32(const float* h0, int V, int D, int T,
                                    const int32_t* row_ptr, const int32_t* gather_row, const int32_t* pair_node,
                                    const int64_t* type_row_off, const float* nin, int use_avg,
                                    int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                    const float* const* edge_w, const float* const* edge_packed, const float* const* edge_bias,
                                    const float* const* wg, const float* const* bg, const float* const* wcx, const float* const* bcx,
                                    const float* const* wch, const float* const* bch, const float* const* cell_packed,
                                    const int32_t* edge_fmt, float* const* layer_out, void* ws, size_t ws_bytes,
                                    ggnn_stream_t stream);

/* ---- (a-B) element-wise stages of the GRU backward (TF autodiff of GRUCell, chem_tensorflow.py:184) -------
 * stage 1: dpc = g*(1-u)*act'(c) -> dpc [V,D];  g*(h-c)*u*(1-u) -> dpg[:, D:2D];  g*u -> dh [V,D];
 *          r*h -> a_c[:, col0:col0+D] (row stride lda: the [x | r*h] operand of the dWc product)
 * stage 2: dh += drh*r;  drh*h*r*(1-r) -> dpg[:, 0:D]   (drh [V,D] with row stride ld_drh)
 * The dense contractions between the stages (dX = dY W^T, dW = X^T dY) are left to the vendor BLAS. */
int ggnn_gru_bwd_stage1_f32(const float* g, const float* h, const float* r, const float* u, const float* c, int act,
                            float* dpc, float* dpg, float* dh, float* a_c, int lda, int col0, int V, int D,
                            ggnn_stream_t stream);
int ggnn_gru_bwd_stage2_f32(const float* drh, int ld_drh, const float* h, const float* r, float* dh, float* dpg,
                            int V, int D, ggnn_stream_t stream);

/* ---- (a-D) dense-adjacency aggregation: chem_tensorflow_dense.py:103-112 ---------------------------
 * acts[g,i,:] = sum_e sum_j A[g,e,i,j] * ( Hm[g*v+j, e*D:(e+1)*D] + bias[e,:] )
 *   A [b,e,v,v] fp32 (A[g,e,dst,src], chem_tensorflow_dense.py:30-36), Hm [b*v, e*D] = h W_e for all e
 *   (ggnn_msg_transform_f32 output), bias [e,D] or NULL (:107-108), acts [b*v, D] out.
 * The dense step is ggnn_msg_transform_f32 -> ggnn_dense_aggregate_f32 -> ggnn_gru_f32 (nx = 1). */
/* The WHOLE dense forward (chem_tensorflow_dense.py:93-117, `steps` timesteps of  h <- GRU(sum_e A_e (h W_e + b_e), h)) in one launch:
 * workgroup g keeps graph g's v <= 32 vertex states on its CU for all timesteps (a graph reads only its own vertices).
 *   ggnn_dense_propagate_supported(v, E, D): v <= 32, E in {2,4,6,8}, D in {32,64,100}.
 *   edge_packed: ggnn_dense_edge_pack_f32 of W [E,D,D] (ggnn_dense_edge_packed_bytes(D,E) bytes: the f32 stage images followed by the
 *   split ones);  gru_packed: ggnn_dense_gru_pack_f32 of Wg [2D,2D], Wc [2D,D] (ggnn_dense_gru_packed_bytes(D) bytes, likewise);
 *   edge_bias [E,D] or NULL;  h0, out [b,v,D];  A [b,E,v,v] (A[g,e,dst,src]).
 *   ggnn_dense_propagate_is_split(v, E, D): 1 when the launch runs the split-form kernel (bf16 matrix pipe, f32 arithmetic: the
 *   process's default matrix path, and the kernel's LDS blocks fit E edge types), 0 for the f32-MFMA kernel.
 *   fmt (split-form launches; ABI 3): operand format of every D x D product, GGNN_GRU_FMT_BF16X3 (exact; 0 means the same) or
 *   GGNN_GRU_FMT_F16X2 under the precondition of "Operand formats" above -- here: every state, every aggregated message
 *   (|acts| <= v E (D max|W_e| max|h| + max|b_e|)) and r*h within 65504, every weight within 255.875.  The packed buffers hold the
 *   images of both formats (f32 | bf16x3 | f16x2 sections). */
int ggnn_dense_propagate_supported(int v, int E, int D);
int ggnn_dense_propagate_is_split(int v, int E, int D);
size_t ggnn_dense_edge_packed_bytes(int D, int T);
int ggnn_dense_edge_pack_f32(const float* W, int T, int D, float* packed, ggnn_stream_t stream);
size_t ggnn_dense_gru_packed_bytes(int D);
int ggnn_dense_gru_pack_f32(const float* Wg, const float* Wc, int D, float* packed, ggnn_stream_t stream);
int ggnn_dense_propagate_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed, const float* edge_bias,
                             const float* bg, const float* bc, float* out, int b, int v, int E, int D, int steps, int fmt,
                             ggnn_stream_t stream);
/* TRAINING on the graph-resident kernels (the backward TF autodiff derives from chem_tensorflow_dense.py:93-117 through
 * compute_gradients, chem_tensorflow.py:184; the dense model shares ONE GRU and ONE edge-weight tensor across timesteps, :84-102).
 *   ggnn_dense_train_supported(v, E, D): 1 where ggnn_dense_propagate_is_split(v, E, D) holds and the backward kernel's LDS blocks
 *   fit (v <= 32, E in {2,4,6,8}, D in {32,64,100}, split matrix path); every entry below returns GGNN_E_UNSUPPORTED otherwise.
 *   ggnn_dense_propagate_save_f32: ggnn_dense_propagate_f32 (same arguments, same `out` bit for bit) that also writes what the
 *   backward reads into `saved` (16-byte aligned, saved_bytes >= ggnn_dense_train_saved_bytes(b, v, D, steps)):
 *       saved [6][steps][b*v, D] f32 -- each tensor stacked over the timesteps, i.e. a [steps*b*v, D] row operand of the
 *       weight-gradient products;  tensor k at timestep t: 0 = h_t (the state ENTERING the step; saved[0][0] = h0),
 *       1 = x_t = sum_e A_e (h_t W_e + b_e) (:103-112), 2 = r, 3 = u, 4 = c, 5 = r*h_t of the GRU (:115).
 *   ggnn_dense_bwd_pack_f32: the 6 + E transposed split images of Wg [2D,2D], Wc [2D,D], W [E,D,D] in the order the backward consumes
 *   them (Wc[h]^T, Wg[x,r]^T, Wg[x,u]^T, Wc[x]^T, Wg[h,r]^T, Wg[h,u]^T, W_e^T); ggnn_dense_bwd_packed_bytes(D, E) bytes (0: no kernel).
 *   ggnn_dense_propagate_bwd_f32: one workgroup per graph walks the timesteps in reverse, every product in the exact bf16x3 format,
 *   no atomics (the same inputs give the same bits).  d_out [b,v,D] = dL/d out;  d_h0 [b,v,D] or NULL.  Per timestep, stacked
 *   [steps, b*v, .] in caller-owned buffers, the operands of the weight-gradient products (ggnn_xty_f32 / ggnn_gemm_tn_f32):
 *       dpc [.., D]  (dWc = [x | r*h]^T dpc),  dpg = [dpr | dpu] [.., 2D]  (dWg = [x | h]^T dpg),
 *       dx [.., D]   (db_e = sum_rows nin_e * dx),  dM [.., E*D]  (dW_e = h^T dM_e;  dM_e[src] = sum_dst A_e[dst,src] dx[dst]).
 *   b == 0 is a no-op for both launches. */
int ggnn_dense_train_supported(int v, int E, int D);
size_t ggnn_dense_train_saved_bytes(int b, int v, int D, int steps);
int ggnn_dense_propagate_save_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                                  const float* edge_bias, const float* bg, const float* bc, float* out, int b, int v, int E, int D,
                                  int steps, int fmt, float* saved, size_t saved_bytes, ggnn_stream_t stream);
size_t ggnn_dense_bwd_packed_bytes(int D, int E);
int ggnn_dense_bwd_pack_f32(const float* W, const float* Wg, const float* Wc, int E, int D, float* packed, ggnn_stream_t stream);
int ggnn_dense_propagate_bwd_f32(const float* d_out, const float* A, const float* bwd_packed, const float* saved, int b, int v, int E,
                                 int D, int steps, float* d_h0, float* dpc, float* dpg, float* dx, float* dM, ggnn_stream_t stream);
/* Edge-weight and edge-bias gradients of the dense model on the backward launch's stacked operands (TF autodiff of
 * chem_tensorflow_dense.py:103-112, chem_tensorflow.py:184), one product launch + one reduce launch, deterministic (fixed-order
 * sums, no atomics), f32 MFMA:
 *     dW[e][k][n] = sum_rows h[row][k] * dM[row][e*D + n]   -> dW [E, D, D], the variable's layout
 *     db[e][n]    = sum_rows nin[row % rows_per_step][e] * dx[row][n]   -> db [E, D]
 *   h, dx [N, D] (saved[0] and dx of ggnn_dense_propagate_bwd_f32), dM [N, E*D], N = steps*b*v;  nin [rows_per_step, E] the
 *   in-degrees of one timestep (rows_per_step = b*v), NULL = no edge biases (db, dx unused).  accumulate != 0: the results are ADDED
 *   to the destinations' contents.  D in {32, 64, 100}, E in {2, 4, 6, 8} (GGNN_E_UNSUPPORTED else);  N == 0 writes zeros, or
 *   nothing under accumulate.  Pointers 16-byte aligned;  ws: ggnn_dense_edge_grad_workspace_bytes(N, E, D) bytes, its contents
 *   before the call do not matter. */
size_t ggnn_dense_edge_grad_workspace_bytes(int N, int E, int D);
int ggnn_dense_edge_grad_f32(const float* h, const float* dM, const float* nin, const float* dx, int N, int rows_per_step, int E, int D,
                             float* dW, float* db, int accumulate, void* ws, size_t ws_bytes, ggnn_stream_t stream);
/* The dense model's optimisation step as two native launch sequences (chem_tensorflow.py:183-191 over
 * chem_tensorflow_dense.py:93-117), the dense twin of ggnn_sparse_train_*: one caller-provided workspace (256-byte aligned,
 * ggnn_dense_train_workspace_bytes(b, v, E, D, steps) bytes, the same one for both calls of a step), nothing allocated, nothing
 * synchronised.  Both refuse what ggnn_dense_train_supported(v, E, D) refuses (GGNN_E_UNSUPPORTED); b == 0 is a no-op.
 *   forward: ggnn_dense_propagate_save_f32 into the workspace; *final_off = byte offset of the final states [b*v, D] in it.
 *   backward: d_final [b*v, D] = dL/d final states.  ggnn_dense_propagate_bwd_f32 (no gradient of h0), then ADDED into the caller's
 *   (zeroed) gradient buffers: g_Wc [2D,D], g_bc [D] += [x | r*h]^T dpc and g_Wg [2D,2D], g_bg [2D] += [x | h]^T dpg with their ones
 *   rows on side_stream (NULL: the main stream), g_W [E,D,D], g_b [E,D] by ggnn_dense_edge_grad_f32 (nin [b*v, E] and g_b both NULL
 *   without edge biases).  Returns with `stream` waiting for the side stream's last product.
 * A binding's step: forward -> ggnn_readout_loss_fwd_f32 per task -> zero the gradient buffers -> ggnn_readout_loss_bwd_f32 per
 * task (d_final) -> backward -> ggnn_clip_adam_f32. */
size_t ggnn_dense_train_workspace_bytes(int b, int v, int E, int D, int steps);
int ggnn_dense_train_forward_f32(const float* h0, const float* A, const float* edge_packed, const float* gru_packed,
                                 const float* edge_bias, const float* bg, const float* bc, int b, int v, int E, int D, int steps, int fmt,
                                 void* ws, size_t ws_bytes, int64_t* final_off, ggnn_stream_t stream);
int ggnn_dense_train_backward_f32(const float* d_final, const float* A, const float* nin, const float* bwd_packed, int b, int v, int E,
                                  int D, int steps, float* g_W, float* g_b, float* g_Wg, float* g_bg, float* g_Wc, float* g_bc,
                                  void* ws, size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream);
int ggnn_dense_aggregate_f32(const float* A, const float* Hm, const float* bias, float* acts, int b, int v,
                             int e, int D, ggnn_stream_t stream);

/* Generic FP32-MFMA GEMM used by the above and by the host layer for the backward pass:
 * C[M,N] = [A0 | A1 | ...] (nseg <= 4 segments of width D each, row stride lda floats, K = nseg*D) x B[K,N].
 * a_segs is a HOST array of device pointers. */
int ggnn_gemm_f32(const float* const* a_segs, int nseg, int D, int lda, const float* B, int ldb, float* C, int ldc,
                  int M, int N, ggnn_stream_t stream);

/* Weight-gradient product of the backward pass (a-B; TF autodiff of tf.matmul, chem_tensorflow.py:184):
 * C[K,N] = A[M,K]^T B[M,N], M ~ 1e5 rows reduced into a small matrix.  The rows are split over the whole GPU and
 * the per-split partials are added in a fixed order (deterministic).  N a multiple of 4, <= 512; A row stride lda,
 * B row stride ldb (multiple of 4, B 16-byte aligned); ws: ggnn_gemm_tn_workspace_bytes(M, K, N) bytes. */
size_t ggnn_gemm_tn_workspace_bytes(int M, int K, int N);
int ggnn_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, float* C, int M, int K, int N, void* ws,
                     size_t ws_bytes, ggnn_stream_t stream);
/* The same product written the way a training step consumes it: C has row stride ldc >= N (a row block of a wider matrix, e.g. one
 * X segment's rows of a GRU weight gradient), and with accumulate != 0 the product is ADDED to C's contents.  The first pass is
 * ggnn_gemm_tn_f32's; the partials are added in their fixed order and that sum is added to C once (deterministic).  M == 0: C is
 * zeroed (accumulate == 0) or left untouched.  Same argument checks and workspace; ggnn_gemm_tn_f32 is this call with ldc = N,
 * accumulate = 0. */
int ggnn_gemm_tn_acc_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int accumulate, int M, int K, int N,
                         void* ws, size_t ws_bytes, ggnn_stream_t stream);

/* ---- (a-B) backward GEMMs of one propagation timestep, hand-written (ggnn_bwd_gemm.hip) ---------------------------------------
 * What TF autodiff derives from chem_tensorflow_sparse.py:160-164, 211-216 through compute_gradients (chem_tensorflow.py:184).
 *
 * ggnn_xty_f32: C[b] = X[rows of batch b]^T Y[rows of batch b]   -- every weight gradient (dW = X^T dY).
 *   X is given as nseg <= 4 column segments of Dseg columns each (HOST arrays x_segs / ldx: pointers and row strides), so the
 *   [residuals | incoming | h] operand of the GRU kernels is never concatenated; x_rows (device int32, or NULL) gathers the X
 *   rows (edge-weight gradients: X row of compact row r = h[pair_node[r]]); row_off HOST [nbatch+1] splits the rows into batches
 *   with one [K,N] output each (one per edge type).  Deterministic (fixed-order split reduction).
 *   Accepted: nseg 1..4, Dseg % 4 == 0, K = nseg * Dseg (tested up to K = 1024: the product is cut into ceil(ceil(Kout / 16) / 16)
 *   K blocks of <= 16 tiles), N % 4 == 0 and N <= 256, 1 <= nbatch <= 64; anything else is GGNN_E_INVALID.  With Kout = K +
 *   (ones_row != 0), REFUSED inside that domain (GGNN_E_UNSUPPORTED) is exactly: x_rows != NULL with Kout > 128 or N > 128
 *   (the row-gathered kernels hold <= 8 x 8 tiles), and every row-gathered product under the experiment GGNN_XTY_ROWS=32 (they
 *   exist with 64-row slabs only).  Every ungathered shape has a kernel on both matrix paths.  ones_row != 0: X gets a virtual column of ones, i.e. C is [K+1, N] per batch and its last row is the column
 *   sum of Y -- the bias gradient comes out of the same pass.  ws: ggnn_xty_workspace_bytes(largest batch, K, N, nbatch).
 * ggnn_colsum_f32: out[n] = sum_v Y[v, n]  (bias gradients), deterministic.
 * ggnn_gru_bwd_dx_cand_f32:  P = dpc Wc^T (WcT = Wc^T, [D, (nx+1)D] row-major):  dx [V, nx*D] = P[:, x columns];
 *   dh += P[:, h columns] * r;  dpg[:, 0:D] = P[:, h columns] * h * r * (1 - r)       (the stage-2 algebra, fused)
 * ggnn_gru_bwd_dx_gates_f32: Q = dpg Wg^T (WgT [2D, (nx+1)D]):  dx[:, residual columns] += Q;
 *   dinc [V,D] = (dx[:, last segment] + Q) (/ (sum_t nin + 1e-7) with use_avg, chem_tensorflow_sparse.py:206-209);  dh += Q[:, h columns]
 * ggnn_gather_segment_sum_acc_f32: out[v] += sum of the gathered rows (several gradient contributions meet in one tensor). */
size_t ggnn_xty_workspace_bytes(int M_max, int K, int N, int nbatch);
int ggnn_xty_f32(const float* const* x_segs, int nseg, int Dseg, const int32_t* ldx, const int32_t* x_rows, const float* Y,
                 int ldy, float* C, int K, int N, int ones_row, const int32_t* row_off, int nbatch, void* ws, size_t ws_bytes,
                 ggnn_stream_t stream);
/* The same product written the way a training step consumes it (what TF's gradient accumulation over the timesteps of a layer
 * does, chem_tensorflow.py:184):  Cb != NULL (needs ones_row): the K weight rows go to C [nbatch][K][N] and the column sums to
 * Cb [nbatch][N];  accumulate != 0: the results are ADDED to the destinations' contents. */
int ggnn_xty_acc_f32(const float* const* x_segs, int nseg, int Dseg, const int32_t* ldx, const int32_t* x_rows, const float* Y,
                     int ldy, float* C, float* Cb, int accumulate, int K, int N, int ones_row, const int32_t* row_off, int nbatch,
                     void* ws, size_t ws_bytes, ggnn_stream_t stream);
/* Which kernel ggnn_xty_acc_f32 runs for a shape -- the launcher's own selection function, host arithmetic only (never touches
 * the GPU).  gathered: x_rows != NULL.  matrix_split / planes / rows_override: 0 or 1 / 0 or 1 / 0 or 32 for the switches
 * GGNN_MATRIX (with GGNN_XTY_SPLIT), GGNN_XTY_PLANES, GGNN_XTY_ROWS; -1 = this process's value.  out = {family (0 f32 MFMA, 1 split
 * per wave, 2 split into LDS planes), gathered, rows per slab, mtm, ntm (tiles of a wave's largest X / dY group), K blocks, X
 * tiles per K block, dY tiles}.  Returns what ggnn_xty_acc_f32 returns for these sizes (GGNN_E_INVALID / GGNN_E_UNSUPPORTED / 0).
 * ggnn_xty_cells: the dispatch table, {family, gathered, rows, mtm, ntm} per instantiation into out (up to `capacity` entries;
 * out may be NULL); returns the number of instantiations. */
int ggnn_xty_describe(int K, int N, int ones_row, int gathered, int matrix_split, int planes, int rows_override, int32_t out[8]);
int ggnn_xty_cells(int32_t* out, int capacity);
size_t ggnn_colsum_workspace_bytes(int N);
int ggnn_colsum_f32(const float* Y, int ldy, int M, int N, float* out, void* ws, size_t ws_bytes, ggnn_stream_t stream);
int ggnn_gru_bwd_dx_cand_f32(const float* dpc, const float* WcT, const float* h, const float* r, float* dx, float* dh,
                             float* dpg, int nx, int V, int D, ggnn_stream_t stream);
int ggnn_gru_bwd_dx_gates_f32(const float* dpg, const float* WgT, float* dx, float* dinc, const float* nin, int T,
                              int use_avg, float* dh, int nx, int V, int D, ggnn_stream_t stream);
int ggnn_gather_segment_sum_acc_f32(const float* Hrows, const int32_t* row_ptr, const int32_t* gather_row, float* out,
                                    int V, int D, ggnn_stream_t stream);

/* Backward building blocks of the other two cell types (chem_tensorflow_sparse.py:105-110) and of any product dX = dY W^T:
 * ggnn_bwd_dx_f32: Q = dY WT with dY [V, nseg_y*D] (column segments of one matrix, row stride ldy) and WT [nseg_y*D, K];
 *   columns [0, xcols) of Q are the x segments (dx is [V, xcols]: written or added to; with split_inc the LAST D of them are
 *   the aggregated messages and go to dinc [V,D] = (acc_dx ? dx + Q : Q), divided by (sum_t nin + 1e-7) with use_avg);
 *   columns [xcols, K) (K == xcols + D; or K == xcols: no h block) -> dh (written, or added to with acc_dh).
 * ggnn_act_bwd_f32: dP = g * act'(out) for out = act(P)   (BasicRNNCell).
 * ggnn_cudnn_gru_train_f32: ggnn_cudnn_gru_f32 that also keeps the candidate c; afterwards ws holds [r*h | u | r | hc] ([V,D] each).
 * ggnn_cudnn_gru_bwd_stage_f32: dpc = g(1-u)(1-c^2); dpg = [dpc hc r(1-r) | g(h-c)u(1-u)]; dh = g u; dhc = dpc r. */
int ggnn_bwd_dx_f32(const float* dY, int ldy, int nseg_y, const float* WT, int K, float* dx, int xcols, int split_inc, float* dinc,
                    const float* nin, int T, int use_avg, float* dh, int acc_dx, int acc_dh, int V, int D, ggnn_stream_t stream);
int ggnn_act_bwd_f32(const float* g, const float* out, int act, float* dP, int V, int D, ggnn_stream_t stream);
int ggnn_cudnn_gru_train_f32(const float* const* x_segs, int nx, const float* h, const float* Wg, const float* bg,
                             const float* Wcx, const float* bcx, const float* Wch, const float* bch, float* h_out,
                             float* save_c, void* ws, size_t ws_bytes, int V, int D, ggnn_stream_t stream);
int ggnn_cudnn_gru_bwd_stage_f32(const float* g, const float* h, const float* r, const float* u, const float* c, const float* hc,
                                 float* dpc, float* dpg, float* dh, float* dhc, int V, int D, ggnn_stream_t stream);

/* The whole GRU backward of a timestep in ONE launch -- D in {32, 64, 100}: whole transposed weight blocks, ggnn_gru_bwd_fused.hip;
 * D in {128, 192, 256}: 64-column panels of them, ggnn_gru_bwd_panel.hip; ggnn_gru_bwd_is_fused(D) is 1 for these six and 0 for
 * every other D, which the launch calls refuse with GGNN_E_UNSUPPORTED -- the mirror image of the
 * fused forward kernel: from g = dL/dh' and the saved h, r, u, c it computes, chained through registers,
 *   dpc = g (1-u) act'(c);  dpu = g (h-c) u (1-u);  drh = dpc Wc^T[h rows];  dpr = drh h r (1-r);
 *   dh  = g u + drh r + [dpr|dpu] Wg^T[h rows];   dx[s] = dpc Wc^T[x_s rows] + [dpr|dpu] Wg^T[x_s rows]   (s < nx)
 *   dx[nx-1] is divided by (sum_t nin + 1e-7) when use_avg (d_incoming of the mean aggregation, chem_tensorflow_sparse.py:206-209)
 * and writes dpc [V,D], dpg = [dpr|dpu] [V,2D] and rh = r*h [V,D] for the weight-gradient products (ggnn_xty_f32).
 *   Wg [(nx+1)D, 2D], Wc [(nx+1)D, D] or NULL: with weights given, their transposed-block stage images are (re)built into
 *   `packed` (ggnn_gru_bwd_packed_bytes(D, nx) bytes; 0 for an unsupported D) first; NULL: `packed` holds them already.
 *   g == NULL: pack only.  dx: HOST array of nx device pointers [V,D].  nx in 1..3; V * 2D < 2^30 (32-bit byte offsets), beyond
 *   it GGNN_E_UNSUPPORTED.  At D in {128, 192, 256} the weight-gradient products that read dpc / dpg / rh are ggnn_gemm_tn_f32's
 *   (dpg is 2D = up to 512 columns wide; ggnn_xty_f32 takes 256). */
int ggnn_gru_bwd_is_fused(int D);
size_t ggnn_gru_bwd_packed_bytes(int D, int nx);
int ggnn_gru_bwd_fused_f32(const float* g, const float* h, const float* r, const float* u, const float* c, const float* Wg,
                           const float* Wc, float* packed, float* dpc, float* dpg, float* rh, float* dh, float* const* dx,
                           const float* nin, int T, int use_avg, int nx, int V, int D, int act, ggnn_stream_t stream);
/* ... with the incoming gradient gathered on load:  g_eff[v] = g[v] + sum of the rows of gz named by gz_heads[v] (one int4 slot-head
 * record per node as ggnn_slot_heads_i32 builds them, -1 = no such slot) -- the per-node sum that closes the transform backward of
 * the timestep processed BEFORE this one (dh[v] += sum_t Z[row(v,t)], chem_tensorflow_sparse.py:160-168 under autodiff), taken by
 * its consumer instead of by a launch of its own.  Bit for bit ggnn_gather_segment_sum_heads_f32(gz, .., accumulate = 1) into g
 * followed by ggnn_gru_bwd_fused_f32, for nodes with at most four rows (more than four slots: run the stand-alone sum).
 * `packed` holds the stage images (no Wg / Wc form). */
int ggnn_gru_bwd_fused_gather_f32(const float* g, const float* gz, const int32_t* gz_heads, const float* h, const float* r,
                                  const float* u, const float* c, float* packed, float* dpc, float* dpg, float* rh, float* dh,
                                  float* const* dx, const float* nin, int T, int use_avg, int nx, int V, int D, int act,
                                  ggnn_stream_t stream);

/* ---- optimiser: per-variable clip_by_norm + TF-1.3 Adam for ALL variables in two launches (chem_tensorflow.py:183-191) --------
 * grads / m / v are FLAT buffers of nblocks * ggnn_optim_block_floats() floats in which every variable starts on a block
 * boundary (padding zero); param_ptrs: DEVICE array [nvars] of the variables' base pointers (each 16-byte aligned; the
 * parameters stay in the model's tensors), var_numel [nvars] their element counts; block_var [nblocks]: variable of each block; var_first [nvars+1]: first block of each variable;
 * var_active [nvars]: 0 = the variable has no gradient this step (left untouched, like a None gradient); partial: nblocks floats.
 *   g <- g * clip / max(||g||_2, clip) per variable (clip_norm <= 0: no clipping);
 *   m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;  p <- p - lr_t m / (sqrt(v) + eps)      (lr_t = lr sqrt(1-b2^t) / (1-b1^t), host) */
int ggnn_optim_block_floats(void);
int ggnn_clip_adam_f32(float* const* param_ptrs, const int32_t* var_numel, const float* grads, float* m, float* v, float* partial,
                       const int32_t* block_var, const int32_t* var_first, const int32_t* var_active, int nblocks, float clip_norm,
                       float lr_t, float beta1, float beta2, float epsilon, ggnn_stream_t stream);

/* ---- batch assembly from dataset-level tables (the step BEFORE the path: chem_tensorflow_sparse.py:278-350 packs a minibatch as
 * one disconnected super-graph, :120-129 derives the message index) --------------------------------------------------------------
 * Every per-batch index structure is a concatenation of per-molecule pieces plus offsets, so the general builders (sorts, scans)
 * run ONCE over the whole dataset taken as one batch and a batch is gathered from their outputs.
 *   ds_tables [11] device pointers for the whole dataset (Gd graphs, Nd nodes, Md messages, Rd compact rows):
 *     0 node_ptr i32[Gd+1]   1 annotations f32[Nd,A]   2 nin f32[Nd,T]   3 row_ptr i32[Nd+1]   4 adj i32[Md,2] (type-major)
 *     5 slot -> src*T+type i32[Md]   6 slot -> message id i32[Md]   7 slot -> compact row i32[Md] (NULL: no compaction)
 *     8 compact row -> node i32[Rd]   9 first message of graph g in the type-t list i32[Gd,T]   10 first compact row, i32[Gd,T]
 *   ds_type_off / ds_type_row_off: host [T+1], type ranges of tables 4 and 8.
 *   batch_tab (device i32): gid[G] | node_off[G+1] | slot_off[G+1] | msg_off[T][G+1] | pair_off[T][G+1]   (exclusive prefix sums over
 *     the batch's graphs, in batch order);  type_off / type_row_off: host [T+1] of the batch.
 *   out [10]: 0 h0 f32[V,D] (annotation, zero-padded: :300-302)  1 graph_nodes_list i32[V]  2 graph_ptr i32[G+1]  3 nin f32[V,T]
 *     4 adj i32[M,2]  5 row_ptr i32[V+1]  6 gather_row i32[M]  7 msg_perm i32[M]  8 pair_node i32[R]  9 compact gather rows i32[M]
 *     10 slot heads i32[V,4] (may be NULL): what ggnn_build_slot_heads gives for (5, 9) -- for (5, 6) without compaction
 *   -- exactly what ggnn_build_target_csr + ggnn_build_compact_sources + ggnn_remap_gather_rows produce for the batch.
 *   ONE launch (the gathers are independent; block ranges of one grid work on nodes / state rows / messages / slots / compact rows):
 *   next to a running forward pass every dependent launch of the packer waits for a launch boundary of the forward stream. */
/* ... and the transpose structures of the backward pass for the same batch (graph_nodes_list = out[1] of ggnn_assemble_batch; batch_tab
 * carries one more array at its end: ptot[G+1], compact rows of the graphs before k over all types).
 *   bwd_tables [8]: 0 by-(src*T+type) row_ptr i32[Nd*T+1]  1 slot -> dst  2 slot -> message id  3 compact row -> first message slot
 *     i32[Rd+1]  4 slot -> dst  5 slot -> message id (type-major slots)  6 node -> first of its compact rows i32[Nd+1]  7 those rows i32[Rd]
 *   out [8]: the same eight arrays for the batch (V*T+1, M, M, R+1, M, M, V+1, R elements). */
int ggnn_assemble_batch_backward(const void* const* ds_tables, const void* const* bwd_tables, int A, int T, const int64_t* ds_type_off,
                                 const int64_t* ds_type_row_off, const int32_t* batch_tab, const int32_t* graph_nodes_list, int G, int V,
                                 int M, int R, int D, const int64_t* type_off, const int64_t* type_row_off, void* const* out,
                                 ggnn_stream_t stream);
int ggnn_assemble_batch(const void* const* ds_tables, int A, int T, const int64_t* ds_type_off, const int64_t* ds_type_row_off,
                        const int32_t* batch_tab, int G, int V, int M, int R, int D, const int64_t* type_off,
                        const int64_t* type_row_off, void* const* out, ggnn_stream_t stream);
/* batch_tab of the two calls above, formed on the device from the batch's graph ids (no host->device copy per batch: it would make
 * the host wait for everything queued on the stream), together with the batch's labels -- one launch:
 *   counts_t i32[rows][Gd]: per dataset graph the node count, message count, messages per type, compact rows per type, compact rows
 *     (rows = 2 + 2T + 1);  gids i64[G] dataset graph ids in batch order;
 *   batch_tab out i32[G + rows*(G+1)] = gid | exclusive prefix sums of every counts row over the batch's graphs;
 *   targets f32[Gd, num_targets], label_mask f32[Gd, num_targets] or NULL (all ones), task_ids i64[K] (device):
 *   target_values[i][j] = targets[gid[j]][task_ids[i]] * mask, target_mask[i][j] = mask   (chem_tensorflow_sparse.py:319-321, 335). */
int ggnn_pack_batch_tables(const int32_t* counts_t, int Gd, int rows, const int64_t* gids, int G, const float* targets,
                           const float* label_mask, int num_targets, const int64_t* task_ids, int K, int32_t* batch_tab,
                           float* target_values, float* target_mask, ggnn_stream_t stream);
/* Sparse GCN batch from dataset-level tables (chem_tensorflow_gcn.py:154-196): graphs [s, s + G) of an epoch's order, one launch.
 *   ds_tables [10]: 0 node_ptr i32[Gd+1]  1 node features f32[Nd, A]  2-4 A_hat as CSR over global node ids (row_ptr i32[Nd+1],
 *     col i32[nnz_d], val f32[nnz_d])  5-7 the same for A_hat^T  8 targets f32[Gd, num_targets]  9 label mask f32[Gd, K] or NULL
 *   task_ids: device i64[K], target column of each task.
 *   epoch_tab: batch_tab of ggnn_pack_batch_tables over the whole epoch order with rows (nodes per graph, A_hat entries per graph):
 *     gid[Ge] | node_cum[Ge+1] | entry_cum[Ge+1].  V and nnz are the batch's node and entry totals (the host's sums of the same counts).
 *   out [12]: 0 h0 f32[V, D] (annotations zero-padded)  1-3 row_ptr i32[V+1], col i32[nnz], val f32[nnz]  4-6 the transpose
 *     7 graph_nodes_list i32[V]  8 graph_ptr i32[G+1]  9 node_uid i64[V] = (graph id << 20) + local node
 *     10 target_values f32[K, G] (0 where the mask is 0)  11 target_mask f32[K, G].
 *   Any D > 0 with A <= D; G == 0 writes the three closing entries only. */
int ggnn_gcn_assemble_batch(const void* const* ds_tables, int Gd, int A, int num_targets, const int64_t* task_ids, int K,
                            const int32_t* epoch_tab, int Ge, int s, int G, int V, int nnz, int D, void* const* out,
                            ggnn_stream_t stream);
/* Dense GGNN batch from dataset-level tables (chem_tensorflow_dense.py:143-193 + :30-36): graphs [s, s + G) of an epoch's order, each
 * padded to v vertices, one launch (one workgroup per graph).  With sparse != 0 also the sparse form of the batch's adjacency tensor
 * over its G*v nodes, as ops.build_message_index builds it from A.nonzero() and build_compact_sources / compact_backward derive it.
 *   ds_tables [18] (data_device.dense_tables_host, local node ids, graph after graph): 0 node_ptr i32[Gd+1]  1 node features
 *     f32[Nd, A]  2 targets f32[Gd, num_targets]  3 label mask f32[Gd, K] or NULL  4 msg_ptr i32[Gd+1]  5 messages i32[Md, 2]
 *     (src, dst), ordered (type, dst, src) inside a graph  6 nin f32[Nd, T]  7 in_ptr i32[Nd]  8 slot_msg i32[Md]; compaction
 *     tables (NULL pair_ptr: none): 9 pair_ptr i32[Gd+1]  10 pair_node i32[Pd]  11 msg_crow i32[Md]  12 src_ptr i32[Nd*T]
 *     13 src_msg i32[Md]  14 rows_msg i32[Md]  15 pair_rows i32[Pd]  16 node_pptr i32[Nd]  17 node_order i32[Pd].
 *   task_ids: device i64[K], target column of each task.
 *   epoch_tab: batch_tab of ggnn_pack_batch_tables over the whole epoch order with rows (messages per type, then active
 *     (source, type) pairs per type): gid[Ge] | pre[2T][Ge+1].
 *   M, R, type_off[T+1], type_row_off[T+1] (host): the batch's message / pair totals and per-type offsets (sparse; R and
 *     type_row_off with compaction tables only).
 *   out [20]: 0 h0 f32[G, v, D]  1 adjacency f32[G, T, v, v] (every entry, 0 / 1)  2 node mask f32[G, v]  3 target_values f32[K, G]
 *     (label * mask)  4 target_mask f32[K, G];  sparse: 5 nin f32[G*v, T]  6 adj i32[M, 2] (type-major)  7 row_ptr i32[G*v+1]
 *     8 gather_row i32[M] (src*T + type)  9 msg_perm i32[M];  compaction: 10 pair_node i32[R]  11 compact gather rows i32[M]
 *     12 by-source row_ptr i32[G*v*T+1]  13 its gather rows (dst) i32[M]  14 its messages i32[M]  15 compact-row row_ptr i32[R+1]
 *     16 its gather rows i32[M]  17 its messages i32[M]  18 node row_ptr i32[G*v+1]  19 node order i32[R].
 *   Any v >= 1, D > 0 with A <= D, 1 <= T <= 16. */
int ggnn_dense_assemble_batch(const void* const* ds_tables, int Gd, int A, int T, int num_targets, const int64_t* task_ids, int K,
                              const int32_t* epoch_tab, int Ge, int s, int G, int v, int D, int M, int R, const int64_t* type_off,
                              const int64_t* type_row_off, int sparse, void* const* out, ggnn_stream_t stream);

/* ---- the optimisation step of the default sparse model as native launch sequences (chem_tensorflow.py:183-191 over
 * chem_tensorflow_sparse.py:117-218; ggnn_train.hip) -----------------------------------------------------------------------------
 * Default cell (GRU), no edge bias, no attention, a hidden size with the gather-fused GRU and the compacted transform (32, 64, 100),
 * at most 2 residual inputs and at least one timestep per layer.  Layer description as in ggnn_sparse_propagate_f32.
 *   forward:  per timestep the compacted transform + ggnn_gru_packed_gather_train_f32; every timestep's state and r / u / c /
 *     incoming stay in `ws` (ggnn_sparse_train_workspace_bytes, 256-byte aligned) for the backward call on the SAME ws.
 *     edge_packed[l]: stage images of the (weight-dropout-masked) edge weights (ggnn_edge_weights_pack_f32), gru_packed[l]:
 *     ggnn_gru_pack_weights_f32.  *final_state_offset: byte offset inside ws of the final node states [V,D].
 *   backward: d_final [V,D] = dL/d(final states) (from ggnn_readout_loss_bwd_f32).  Per timestep, last to first: the fused GRU
 *     backward, the transpose segment sum over (rows_rp, rows_gather[, rows_heads]) (segments = compact rows, gather = target node),
 *     the compacted transform with the images of W^T (edge_packed_t[l]) on identity_rows = 0..R-1, the per-node sum over
 *     (node_rp, node_order[, node_heads]); on `side_stream` the weight-gradient products, ADDED into g_edge[l] [T,D,D], g_Wg[l]
 *     [(nx+1)D, 2D], g_bg[l] [2D], g_Wc[l] [(nx+1)D, D], g_bc[l] [D] (the caller zeroes them; under weight dropout it masks g_edge
 *     afterwards).  d_state_ws[l] [V,D] (l < num_layers): scratch for the gradients of the layer inputs; their contents are UNDEFINED
 *     on return (d_state_ws[0], the gradient of h0, is not even completed: h0 is data).  Returns with `stream`
 *     ordered behind the side stream's last product.  Events come from a per-device pool the library creates on first use.
 *   prepare: ALL of a step's stage images in one launch (the weights change every step): per layer l the T edge-weight images
 *     (edge_packed[l], ggnn_msg_transform_compact_workspace_bytes) and those of the transposed weights (edge_packed_t[l]) -- of the
 *     variable edge_w[l] [T*D, D] masked on the fly like ggnn_dropout_f32(keep_prob, seeds[l]) masks it (keep_prob 1: unmasked) --,
 *     the fused GRU's images (gru_packed[l], ggnn_gru_packed_bytes(D, nx[l])) and its backward's (gru_bwd_packed[l]).  num_layers <= 16;
 *     nx, seeds, and the pointer arrays are HOST arrays.
 *   gru_fmt (prepare and forward; HOST [num_layers] of GGNN_GRU_FMT_*, or NULL = BF16X3 for every layer): the operand format of
 *     layer l's GRU forward images / launches -- the same array must be given to both calls of a step. */
int ggnn_sparse_train_prepare_f32(int num_layers, int T, int D, const int32_t* nx, const float* const* edge_w, float keep_prob,
                                  const uint64_t* seeds, const float* const* Wg, const float* const* Wc, const int32_t* gru_fmt,
                                  float* const* edge_packed, float* const* edge_packed_t, float* const* gru_packed,
                                  float* const* gru_bwd_packed, ggnn_stream_t stream);
size_t ggnn_sparse_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps);
int ggnn_sparse_train_forward_f32(const float* h0, int V, int D, int T, const int32_t* row_ptr, const int32_t* gather_row_c,
                                  const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg, int num_layers,
                                  const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                  const float* const* edge_packed, const float* const* bg, const float* const* bc,
                                  const float* const* gru_packed, const int32_t* gru_fmt, int act, void* ws, size_t ws_bytes,
                                  int64_t* final_state_offset, ggnn_stream_t stream);
int ggnn_sparse_train_backward_f32(const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off,
                                   const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
                                   const int32_t* res_ptr, const int32_t* res_idx, const int32_t* rows_rp, const int32_t* rows_gather,
                                   const int32_t* rows_heads, const int32_t* node_rp, const int32_t* node_order,
                                   const int32_t* node_heads, const int32_t* identity_rows, const float* const* edge_packed_t,
                                   const float* const* gru_bwd_packed, int act, float* const* g_edge, float* const* g_Wg,
                                   float* const* g_bg, float* const* g_Wc, float* const* g_bc, float* d_final, float* const* d_state_ws,
                                   void* ws, size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream);

/* The same step of the default model at the column-panel hidden sizes 128 / 192 / 256 (ggnn_sparse_train_panel_supported: 1 for
 * these three, else 0; the pair above keeps refusing them with GGNN_E_UNSUPPORTED, and this one refuses every other size): the
 * conditions, argument lists and conventions of the pair above, one driver with a second route (ggnn_train.hip).
 *   forward:  per timestep ggnn_msg_transform_compact_f32 on the layer's ring images, ggnn_gather_segment_sum_f32 over (row_ptr,
 *     gather_row_c) into that timestep's `incoming` (mean epilogue with use_avg; no edge bias), ggnn_gru_packed_f32 on the panel
 *     images saving r / u / c, in gru_fmt[l].
 *   backward: per timestep, last to first: the panel GRU backward (ggnn_gru_bwd_fused_f32, or ggnn_gru_bwd_fused_gather_f32 when the
 *     previous timestep's node sum is pending: T <= 4 and node_heads given), then the transpose segment sum, the transform on the W^T
 *     images and the node sum as above.  On `side_stream`, ADDED into the caller's gradient views: per X segment
 *     ggnn_gemm_tn_acc_f32 for dWc = [x.. | incoming | r*h]^T dpc and dWg = [x.. | incoming | h]^T dpg (timestep by timestep, in the autograd
 *     step's order of summation; with GGNN_TRAIN_MERGE_PRODUCTS=1 the timesteps of a layer without residual inputs as one product
 *     over S*V rows), ggnn_colsum_f32 of dpc / dpg added to g_bc / g_bg, and the
 *     row-gathered ggnn_xty_acc_f32 for the edge weights -- D = 128 straight into g_edge[l], D = 192 / 256 through 128-column views
 *     of h and dHc whose blocks one launch adds into [T, D, D].
 *   `ws`: ggnn_sparse_train_panel_workspace_bytes (0 on bad arguments or another hidden size), the SAME buffer for both calls; the
 *     calls allocate nothing and synchronise nothing.  V * 2D, compact_rows * D < 2^30 and V * total_steps < 2^31, checked before
 *     anything is enqueued (GGNN_E_UNSUPPORTED).
 *   prepare: per layer the T ring images of the edge weights and of their transposes (masked on the fly as above), the panel GRU's
 *     images in gru_fmt[l] and its backward's -- each bit for bit what ggnn_edge_weights_pack_f32 (on the masked weights / their
 *     transposes), ggnn_gru_pack_weights_f32 and ggnn_gru_bwd_fused_f32(g = NULL) write, with the buffer sizes of those calls. */
int ggnn_sparse_train_panel_supported(int D);
int ggnn_sparse_train_panel_prepare_f32(int num_layers, int T, int D, const int32_t* nx, const float* const* edge_w, float keep_prob,
                                        const uint64_t* seeds, const float* const* Wg, const float* const* Wc, const int32_t* gru_fmt,
                                        float* const* edge_packed, float* const* edge_packed_t, float* const* gru_packed,
                                        float* const* gru_bwd_packed, ggnn_stream_t stream);
size_t ggnn_sparse_train_panel_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps);
int ggnn_sparse_train_panel_forward_f32(const float* h0, int V, int D, int T, const int32_t* row_ptr, const int32_t* gather_row_c,
                                        const int32_t* pair_node, const int64_t* type_row_off, const float* nin, int use_avg,
                                        int num_layers, const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                        const float* const* edge_packed, const float* const* bg, const float* const* bc,
                                        const float* const* gru_packed, const int32_t* gru_fmt, int act, void* ws, size_t ws_bytes,
                                        int64_t* final_state_offset, ggnn_stream_t stream);
int ggnn_sparse_train_panel_backward_f32(const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off,
                                         const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
                                         const int32_t* res_ptr, const int32_t* res_idx, const int32_t* rows_rp,
                                         const int32_t* rows_gather, const int32_t* rows_heads, const int32_t* node_rp,
                                         const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
                                         const float* const* edge_packed_t, const float* const* gru_bwd_packed, int act,
                                         float* const* g_edge, float* const* g_Wg, float* const* g_bg, float* const* g_Wc,
                                         float* const* g_bc, float* d_final, float* const* d_state_ws, void* ws, size_t ws_bytes,
                                         ggnn_stream_t stream, ggnn_stream_t side_stream);

/* The same step with propagation attention (chem_tensorflow_sparse.py:147-149, 170-196) on the compacted route: the conditions and
 * conventions of the pair above (GRU cell, no edge bias, hidden size 32 / 64 / 100, images from ggnn_sparse_train_prepare_f32 with
 * gru_fmt NULL: every product in GGNN_GRU_FMT_BF16X3), a batch with M >= 1 messages.  `ws`: ggnn_sparse_attn_train_workspace_bytes
 * (0 on bad arguments), the SAME buffer for both calls.
 *   forward:  per timestep ggnn_msg_transform_compact_f32, ggnn_gather_segment_sum_attn_compact_f32 over (row_ptr, slot_pair,
 *     slot_row) with attn_factors[l] [T] into that timestep's `incoming`, ggnn_gru_packed_f32 saving r / u / c.
 *   backward: per timestep, last to first: the fused GRU backward, the compact rows recomputed (edge_packed[l]),
 *     ggnn_attn_bwd_target_compact_f32 (msg_perm: by-target slot -> message id), ggnn_range_sum_f32 of dfac over msg_type_off (HOST
 *     [T+1]: the message ids of type t) ADDED to g_attn[l] [T], ggnn_attn_bwd_source_compact_f32 over (src_node_ptr, src_dst,
 *     src_msg, src_row), then as above: the transform on W^T, the per-node sum, the products on `side_stream`. */
size_t ggnn_sparse_attn_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps, int64_t M);
int ggnn_sparse_attn_train_forward_f32(const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr,
                                       const int32_t* slot_pair, const int32_t* slot_row, const int32_t* pair_node,
                                       const int64_t* type_row_off, const float* nin, int use_avg, int num_layers,
                                       const int32_t* layer_timesteps, const int32_t* res_ptr, const int32_t* res_idx,
                                       const float* const* edge_packed, const float* const* attn_factors, const float* const* bg,
                                       const float* const* bc, const float* const* gru_packed, int act, void* ws, size_t ws_bytes,
                                       int64_t* final_state_offset, ggnn_stream_t stream);
int ggnn_sparse_attn_train_backward_f32(const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr,
                                        const int32_t* slot_pair, const int32_t* slot_row, const int32_t* msg_perm,
                                        const int64_t* msg_type_off, const int32_t* pair_node, const int64_t* type_row_off,
                                        const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
                                        const int32_t* res_ptr, const int32_t* res_idx, const int32_t* src_node_ptr,
                                        const int32_t* src_dst, const int32_t* src_msg, const int32_t* src_row, const int32_t* node_rp,
                                        const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
                                        const float* const* edge_packed, const float* const* edge_packed_t,
                                        const float* const* gru_bwd_packed, const float* const* attn_factors, int act,
                                        float* const* g_edge, float* const* g_attn, float* const* g_Wg, float* const* g_bg,
                                        float* const* g_Wc, float* const* g_bc, float* d_final, float* const* d_state_ws, void* ws,
                                        size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream);

/* The same step for graph_rnn_cell = RNN (tf BasicRNNCell, chem_tensorflow_sparse.py:109-110, the R-GCN configuration) on the
 * compacted route: the conventions of the first pair above (no attention, no edge bias, a batch with M >= 1 messages), with the
 * cell's arguments in place of the GRU's.  Every layer's (D, nx) must be in ggnn_rnn_fused_supported -- otherwise, and for a batch
 * without compact rows, GGNN_E_UNSUPPORTED / GGNN_E_INVALID is returned before anything is enqueued.  The images are per layer
 * ggnn_edge_weights_pack_f32 of W and of its transposes (edge_packed / edge_packed_t), ggnn_rnn_pack_weights_f32 (rnn_packed) and
 * ggnn_rnn_bwd_pack_weights_f32 (rnn_bwd_packed); there is no one-launch prepare for this cell.  `ws`:
 * ggnn_sparse_rnn_train_workspace_bytes (0 for a hidden size outside the cell's or on bad arguments; no r / u / c / r*h / dpg
 * buffers, so smaller than the GRU's), the SAME buffer for both calls.
 *   forward:  per timestep ggnn_msg_transform_compact_f32 and ggnn_rnn_packed_gather_f32 with save_incoming (M: the length of
 *     gather_row_c) -- the launches of the autograd route's training forward, so every state is bit-identical to it.
 *   backward: per timestep, last to first: ggnn_rnn_bwd_fused_f32 (ggnn_rnn_bwd_fused_gather_f32 when the node sum of the timestep
 *     before is pending); on `side_stream` ONE ggnn_xty_acc_f32, g_W[l] += [x.. | incoming | h]^T dP with g_b[l] += its column
 *     sums (one product per layer for a residual-free layer of several timesteps); then as above: the transpose segment sum into
 *     dHc, the transform on W^T, the per-node sum (deferred), the row-gathered edge-weight product on `side_stream`.
 *   Replaces, per timestep of variants._hip_backward's RNN branch (chem_tensorflow.py:184 over chem_tensorflow_sparse.py:109-110,
 *   198-216): ggnn_act_bwd_f32, ggnn_xty_f32, a transposed copy of W, ggnn_bwd_dx_f32, and backward.transform_backward's launches. */
size_t ggnn_sparse_rnn_train_workspace_bytes(int V, int D, int T, int64_t compact_rows, int total_steps);
int ggnn_sparse_rnn_train_forward_f32(const float* h0, int V, int D, int T, int64_t M, const int32_t* row_ptr,
                                      const int32_t* gather_row_c, const int32_t* pair_node, const int64_t* type_row_off,
                                      const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
                                      const int32_t* res_ptr, const int32_t* res_idx, const float* const* edge_packed,
                                      const float* const* rnn_b, const float* const* rnn_packed, int act, void* ws, size_t ws_bytes,
                                      int64_t* final_state_offset, ggnn_stream_t stream);
int ggnn_sparse_rnn_train_backward_f32(const float* h0, int V, int D, int T, const int32_t* pair_node, const int64_t* type_row_off,
                                       const float* nin, int use_avg, int num_layers, const int32_t* layer_timesteps,
                                       const int32_t* res_ptr, const int32_t* res_idx, const int32_t* rows_rp,
                                       const int32_t* rows_gather, const int32_t* rows_heads, const int32_t* node_rp,
                                       const int32_t* node_order, const int32_t* node_heads, const int32_t* identity_rows,
                                       const float* const* edge_packed_t, const float* const* rnn_bwd_packed, int act,
                                       float* const* g_edge, float* const* g_W, float* const* g_b, float* d_final,
                                       float* const* d_state_ws, void* ws, size_t ws_bytes, ggnn_stream_t stream,
                                       ggnn_stream_t side_stream);

/* ---- tf.nn.dropout with a counter-based mask (chem_tensorflow_sparse.py:91 edge-weight dropout, :113-114 DropoutWrapper on the
 * new node state; chem_tensorflow_dense.py:104; utils.py:68 readout weights) ------------------------------------------------------
 *   out[r,c] = x[r,c] / keep_prob * floor(keep_prob + U),   U = (Philox4x32-10(counter, key)[c % 4] >> 8) * 2^-24
 *   key = (seed lo, seed hi), counter = (rowkey lo, rowkey hi, c / 4, 0), rowkey = row_key[r] (row_key != NULL) or row_key_base + r.
 * The mask is a pure function of (seed, row key, column): ranks of a data-parallel job derive identical weight masks from the
 * same seed, a node's state mask does not depend on the batch it sits in, and the backward pass is the same call on dL/dout.
 * x, out [rows, cols] contiguous fp32 (in place allowed); any cols (16-byte accesses when cols % 4 == 0). */
int ggnn_dropout_f32(const float* x, float* out, const int64_t* row_key, int64_t row_key_base, uint64_t seed, float keep_prob,
                     int64_t rows, int cols, ggnn_stream_t stream);

/* ---- sparse GCN (chem_tensorflow_gcn.py:62-82, Kipf-style): one layer  out = dropout(relu(A_hat x W + b)) ----------------------
 * A_hat is a weighted sparse [V,V] matrix in CSR form: row_ptr [V+1], col [nnz], val [nnz] (int32, int32, fp32).  Row i of
 * S = A_hat x is summed in slot order (deterministic, no atomics); column indices outside [0, V) contribute nothing.
 * Fused single-launch kernel for D = 32, 64, 100 (ggnn_gcn_fused_supported); other hidden sizes return GGNN_E_UNSUPPORTED and are
 * composed by the caller from ggnn_weighted_segment_sum_f32, ggnn_gemm_f32 and ggnn_gcn_epilogue_f32.
 * The product S W runs in the exact bf16x3 split form only (no f16x2 format: the final layer is linear and unbounded).
 * ggnn_gcn_pack_weights_f32: the LDS image (ggnn_gcn_image_bytes(D) bytes, 16-byte aligned) of W [D,D], or of W^T (transpose != 0:
 *   the backward pass dx = A_hat^T (dP W^T) is the same layer call on the transposed CSR with that image, no bias/ReLU/dropout).
 * ggnn_gcn_layer_f32: bias [D] or NULL; relu != 0 applies ReLU; keep_prob < 1 applies the dropout of ggnn_dropout_f32 with the same
 *   (seed, row key, column) -- bit-identical masks; s_out [V,D] or NULL receives S.  out and s_out must not alias x.
 * ggnn_gcn_epilogue_f32: out = dropout(relu(P + bias)) with the same options (the composed path's third launch; in place allowed).
 * ggnn_gcn_propagate_f32: all num_layers layers of an inference forward behind one call (ReLU on all but the last layer, no
 *   dropout); W / bias are HOST arrays of num_layers device pointers (bias NULL: no bias); ws: ggnn_gcn_workspace_bytes(V, D,
 *   num_layers) bytes (weight images and two ping-pong state buffers).  V == 0 is a no-op. */
int ggnn_gcn_fused_supported(int D);
size_t ggnn_gcn_image_bytes(int D);
int ggnn_gcn_pack_weights_f32(const float* W, int D, int transpose, float* img, ggnn_stream_t stream);
int ggnn_gcn_layer_f32(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int64_t nnz, const float* img,
                       const float* bias, int relu, const int64_t* row_key, int64_t row_key_base, uint64_t seed, float keep_prob,
                       float* out, float* s_out, int V, int D, ggnn_stream_t stream);
int ggnn_gcn_epilogue_f32(const float* P, const float* bias, int relu, const int64_t* row_key, int64_t row_key_base, uint64_t seed,
                          float keep_prob, float* out, int V, int D, ggnn_stream_t stream);
size_t ggnn_gcn_workspace_bytes(int V, int D, int num_layers);
int ggnn_gcn_propagate_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col, const float* val,
                           int64_t nnz, const float* const* W, const float* const* bias, float* out, void* ws, size_t ws_bytes,
                           ggnn_stream_t stream);

/* ---- sparse GCN at hidden sizes 128 / 192 / 256: the same layer in one launch on column panels of W (ggnn_gcn_panel.hip) ---------
 * A workgroup aggregates 8 x 16 rows of S = A_hat x in registers and walks the D / 64 column panels of W, whose images stream
 * through an LDS ring; products in the exact bf16x3 split form.  Opt-in: ggnn_gcn_fused_supported and its siblings keep their values.
 * ggnn_gcn_panel_supported: 1 for D = 128, 192, 256; every entry point below returns GGNN_E_UNSUPPORTED for any other D.
 * ggnn_gcn_panel_pack_weights_f32: the D / 64 panel images (ggnn_gcn_panel_image_bytes(D) bytes in all, 16-byte aligned) of W [D,D],
 *   or of W^T (transpose != 0: the backward's dx = A_hat^T (dP W^T) is the same layer call on the transposed CSR).
 * ggnn_gcn_panel_layer_f32: the arguments, validation and results of ggnn_gcn_layer_f32 (img: the panel images).
 * ggnn_gcn_panel_propagate_f32: ggnn_gcn_propagate_f32 on this kernel; ws: ggnn_gcn_panel_workspace_bytes(V, D, num_layers) bytes.
 * ggnn_gcn_panel_launch_geometry: rows a workgroup takes per pass and the launcher's cap on workgroups (a launch wraps beyond
 *   their product); either pointer may be NULL. */
int ggnn_gcn_panel_supported(int D);
size_t ggnn_gcn_panel_image_bytes(int D);
void ggnn_gcn_panel_launch_geometry(int* rows_per_workgroup, int* max_workgroups);
int ggnn_gcn_panel_pack_weights_f32(const float* W, int D, int transpose, float* img, ggnn_stream_t stream);
int ggnn_gcn_panel_layer_f32(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                             const float* img, const float* bias, int relu, const int64_t* row_key, int64_t row_key_base,
                             uint64_t seed, float keep_prob, float* out, float* s_out, int V, int D, ggnn_stream_t stream);
size_t ggnn_gcn_panel_workspace_bytes(int V, int D, int num_layers);
int ggnn_gcn_panel_propagate_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                                 const float* val, int64_t nnz, const float* const* W, const float* const* bias, float* out,
                                 void* ws, size_t ws_bytes, ggnn_stream_t stream);

/* ---- sparse GCN: the optimisation step as native launch sequences (ggnn_gcn.hip, ggnn_gcn_train.hip) -----------------------------
 * ggnn_gcn_layer_bwd_f32: the backward of one layer with the gate of the layer BELOW in its epilogue, one launch:
 *     out = [gate_out > 0] * dropout(A_hat^T (dP W^T))      = the dP of the layer below
 *   on the transposed CSR with the image of W^T; gate_out [V,D] is the lower layer's forward output dropout(relu(P)), the dropout is
 *   that layer's (ggnn_dropout_f32's expression and mask for (seed, row key, column); keep_prob 1: none), the select is
 *   ggnn_act_bwd_f32's: bit-identical to ggnn_gcn_layer_f32 + ggnn_dropout_f32 + ggnn_act_bwd_f32.  out must not alias dP or gate_out.
 * ggnn_gcn_train_pack_f32: every weight image of a step in one launch.  W: HOST array of num_layers (<= 64) device pointers;
 *   images: 2 num_layers - 1 slots of ggnn_gcn_image_bytes(D) rounded up to 256 bytes: slot l = the image of W_l, slot
 *   num_layers + l - 1 = the image of W_l^T for l >= 1 -- ggnn_gcn_pack_weights_f32's images bit for bit.
 * ggnn_gcn_train_supported: 1 for the hidden sizes with the native step (32, 64, 100).
 * ggnn_gcn_train_forward_f32: the pack launch and num_layers saving layer launches (ReLU and dropout with seeds[l] -- HOST array --
 *   on all but the last layer; row_key [V] int64 or NULL: the row index) into ws (ggnn_gcn_train_workspace_bytes: the images,
 *   S_l, the layer outputs, one dP buffer per layer and the product workspace); *final_off = byte offset in ws of the final states.
 * ggnn_gcn_train_backward_f32: d_final [V,D] = dL/d final states; per layer g_W[l] [D,D] += S_l^T dP_l and, with g_b != NULL,
 *   g_b[l] [D] += colsum(dP_l) on side_stream (ggnn_xty_acc_f32; ggnn_colsum_f32, whose sums are the autograd route's bit for
 *   bit, rather than the product's ones row), and dP_{l-1} by ggnn_gcn_layer_bwd_f32 on stream for l >= 1;
 *   g_W / g_b: HOST arrays of device pointers, ADDED to.  On return stream waits for side_stream's last product (side_stream NULL:
 *   everything on stream).  ws as the forward call left it, same (row_key, seeds, keep_prob).
 * V == 0 is a no-op; V*D >= 2^30 and other hidden sizes return GGNN_E_UNSUPPORTED. */
int ggnn_gcn_layer_bwd_f32(const float* dP, const int32_t* row_ptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                           const float* img_T, const float* gate_out, const int64_t* row_key, int64_t row_key_base, uint64_t seed,
                           float keep_prob, float* out, int V, int D, ggnn_stream_t stream);
int ggnn_gcn_train_pack_f32(const float* const* W, int num_layers, int D, float* images, ggnn_stream_t stream);
int ggnn_gcn_train_supported(int D);
size_t ggnn_gcn_train_workspace_bytes(int V, int D, int num_layers);
int ggnn_gcn_train_forward_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                               const float* val, int64_t nnz, const float* const* W, const float* const* bias, const int64_t* row_key,
                               const uint64_t* seeds, float keep_prob, void* ws, size_t ws_bytes, int64_t* final_off,
                               ggnn_stream_t stream);
int ggnn_gcn_train_backward_f32(const float* d_final, int V, int D, int num_layers, const int32_t* row_ptr_t, const int32_t* col_t,
                                const float* val_t, int64_t nnz, const int64_t* row_key, const uint64_t* seeds, float keep_prob,
                                float* const* g_W, float* const* g_b, void* ws, size_t ws_bytes, ggnn_stream_t stream,
                                ggnn_stream_t side_stream);

/* ---- sparse GCN: the same native step at hidden sizes 128 / 192 / 256 on the column-panel kernels (ggnn_gcn_panel.hip) -----------
 * The optimisation step of chem_tensorflow.py:183-191 over the layers of chem_tensorflow_gcn.py:62-82 at the wide sizes.
 * The twins of the six entry points above, with their arguments, validation, workspace layout, streams and results; in place of
 * gcn_model.GCNLayerFn's per-layer backward on the panel route -- a transposed ggnn_gcn_panel_layer_f32, ggnn_dropout_f32 and
 * ggnn_act_bwd_f32 over [V,D], two ggnn_gcn_panel_pack_weights_f32, a ggnn_gemm_tn_f32 and a ggnn_colsum_f32, enqueued from Python.
 * ggnn_gcn_panel_layer_bwd_f32: ggnn_gcn_layer_bwd_f32 on the panel kernel, img_T = the panel images of W^T: bit-identical to
 *   ggnn_gcn_panel_layer_f32 (transposed CSR, img_T) + ggnn_dropout_f32 + ggnn_act_bwd_f32.
 * ggnn_gcn_panel_train_pack_f32: ggnn_gcn_train_pack_f32 in the panel format: slots of ggnn_gcn_panel_image_bytes(D) rounded up to
 *   256 bytes, each the D / 64 panel images of W_l (slot l) or W_l^T (slot num_layers + l - 1, l >= 1) --
 *   ggnn_gcn_panel_pack_weights_f32's images bit for bit.
 * ggnn_gcn_panel_train_supported: 1 for the hidden sizes with this step (128, 192, 256); ggnn_gcn_train_supported and the
 *   ggnn_gcn_train_* calls keep their values and return codes at these sizes.
 * ggnn_gcn_panel_train_forward_f32 / _backward_f32: ggnn_gcn_train_forward_f32 / _backward_f32 over ggnn_gcn_panel_train_pack_f32,
 *   ggnn_gcn_panel_layer_f32 and ggnn_gcn_panel_layer_bwd_f32; ws: ggnn_gcn_panel_train_workspace_bytes(V, D, num_layers) bytes
 *   (0 for an unsupported D). */
int ggnn_gcn_panel_layer_bwd_f32(const float* dP, const int32_t* row_ptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                                 const float* img_T, const float* gate_out, const int64_t* row_key, int64_t row_key_base,
                                 uint64_t seed, float keep_prob, float* out, int V, int D, ggnn_stream_t stream);
int ggnn_gcn_panel_train_pack_f32(const float* const* W, int num_layers, int D, float* images, ggnn_stream_t stream);
int ggnn_gcn_panel_train_supported(int D);
size_t ggnn_gcn_panel_train_workspace_bytes(int V, int D, int num_layers);
int ggnn_gcn_panel_train_forward_f32(const float* h0, int V, int D, int num_layers, const int32_t* row_ptr, const int32_t* col,
                                     const float* val, int64_t nnz, const float* const* W, const float* const* bias,
                                     const int64_t* row_key, const uint64_t* seeds, float keep_prob, void* ws, size_t ws_bytes,
                                     int64_t* final_off, ggnn_stream_t stream);
int ggnn_gcn_panel_train_backward_f32(const float* d_final, int V, int D, int num_layers, const int32_t* row_ptr_t,
                                      const int32_t* col_t, const float* val_t, int64_t nnz, const int64_t* row_key,
                                      const uint64_t* seeds, float keep_prob, float* const* g_W, float* const* g_b, void* ws,
                                      size_t ws_bytes, ggnn_stream_t stream, ggnn_stream_t side_stream);

/* ---- measurement aid (bench.py's roofline leg; not on the product path) --------------------------------------------------------
 * The dense bf16 MFMA rate the chip SUSTAINS: `launches` back-to-back launches (~16 ms each) of v_mfma_f32_16x16x32_bf16 on
 * register operands, 8 waves per CU; mode 0 all-zero operands, 1 random operands, 2 the operand pattern and planes of the 3-way
 * split product (csrc/ggnn_split.hpp).  Reports the last launch: whole-chip dense TFLOP/s and the mean shader clock inside it
 * (the data-sheet peak, 2.5 PF, is 256 CUs x 4 x 8192 flops / 16 clocks at 2.4 GHz; under random operands the chip runs at its
 * socket power limit well below that clock).  ws: ggnn_probe_mfma_workspace_bytes() of device memory.  Synchronises `stream`. */
size_t ggnn_probe_mfma_workspace_bytes(void);
int ggnn_probe_mfma_rate(int mode, int launches, void* ws, size_t ws_bytes, double* tflops, double* shader_mhz, ggnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GGNN_HIP_H */
