"""Operator layer: torch-ROCm tensors in, libggnn_hip.so HIP kernels underneath (via ctypes).

One function per TF op call site of the reference's sparse hot path
(chem_tensorflow_sparse.py:117-218):

    build_message_index   S1 (+ our bucketing by target)     :120-129
    msg_transform         S3 (transform-first)                :160-164
    gather_segment_sum    S2,S4,S5,S6,S7                      :160-162,168,198-209
    gru                   S8,S9                               :211-216
    unsorted_segment_sum  general tf.unsorted_segment_sum     :198-200, :226-228

PyTorch is plumbing only (device memory + streams).  Every function requires CUDA(HIP) tensors and
raises if the extension is missing -- there is no CPU path here.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, derived
from ._lib import check

ACT_IDS = {"tanh": 0, "relu": 1}
GRU_FUSED_MAX_INPUTS = 3        # input segments (residual inputs + aggregated messages) of the single-launch GRU kernels
GRU_MAX_INPUTS = 7              # ... of the generic two-launch GRU (8 K segments of the generic GEMM: 7 inputs + h)
GRU_FMT_F16X2, GRU_FMT_EXACT = 2, 3   # operand formats of the fused GRU forward (GGNN_GRU_FMT_F16X2 / _BF16X3; policy: formats.py)


def kernel_width(D: int) -> int:
    """Width at which node states of hidden size D live in HBM.  Hidden sizes the kernels take as they are (multiples of 32, 64
    or 100) keep their width; any other size -- the reference accepts every hidden_size (chem_tensorflow_sparse.py:46-50) -- is
    zero-padded to the next width that has single-launch kernels (32, 64, 100, 128, 192, 256), beyond that to a multiple of 32.
    Zero columns stay zero through every propagation step when the weights are padded with zeros (padded rows contribute 0 to
    every product; a padded state column is u*0 + (1-u)*act(0) = 0 for tanh and ReLU), so the model is unchanged."""
    D = int(D)
    if D <= 0:
        raise ValueError("hidden_size must be positive")
    if D % 32 == 0 or D % 100 == 0:
        return D
    for w in (32, 64, 100, 128, 192, 256):
        if D <= w:
            return w
    return (D + 31) // 32 * 32
# sparse_propagate: gather the segment sum inside the fused GRU (2 launches per timestep instead of 3) for layers with at
# most FUSE_GATHER concatenated GRU inputs (3 = every layer (default: +1.8 % over 1 on MI355X), 1 = only layers without
# residual inputs, 0 = never)
FUSE_GATHER = int(os.environ.get("GGNN_FUSE_GATHER", "3"))


# ---- optional per-launch timing (bench.py's roofline leg) ---------------------------------------------
_timing = None


class kernel_timing:
    """Context manager: while active every op brackets its launch(es) with HIP events recorded on the
    stream the kernel is launched on (torch's current stream == the stream handed to the C ABI) and the
    GRU is issued as its two separately addressable launches.  `.results()` -> {name: [ms, ...]}."""

    def __enter__(self):
        global _timing
        self.records = _timing = []
        return self

    def __exit__(self, *exc):
        global _timing
        _timing = None

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for name, s, e in self.records:
            out.setdefault(name, []).append(s.elapsed_time(e))
        return out


def _launch(name: str, fn):
    if _timing is None:
        return check(fn())
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    _timing.append((name, s, e))
    check(rc)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/HIP tensor (the GGNN hot path has no CPU implementation)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


@dataclass
class MessageIndex:
    """Per-batch message index (built once, reused by all propagation steps and epochs).

    adj         [M,2] int32  concatenated adjacency lists (type-major)   (:124-129)
    type_off    list[T+1]    host offsets of each type in adj
    row_ptr     [V+1] int32  slots of the messages INTO node v
    gather_row  [M]   int32  slot -> src*T + type
    msg_perm    [M]   int32  slot -> original message index
    """
    adj: torch.Tensor
    type_off: List[int]
    row_ptr: torch.Tensor
    gather_row: torch.Tensor
    msg_perm: torch.Tensor
    num_nodes: int
    num_edge_types: int

    @property
    def num_messages(self) -> int:
        return int(self.type_off[-1])


def _build_index(adjacency_lists: Sequence[torch.Tensor], num_nodes: int, validate: bool, by_source: bool) -> MessageIndex:
    lib = _lib.load()
    T = len(adjacency_lists)
    if T == 0:
        raise ValueError("need at least one edge type")
    lists = [_req(a.reshape(-1, 2), torch.int32, "adjacency_lists[%d]" % i) for i, a in enumerate(adjacency_lists)]
    dev = lists[0].device
    type_off = [0]
    for a in lists:
        type_off.append(type_off[-1] + a.shape[0])
    M = type_off[-1]
    adj = torch.cat(lists, dim=0).contiguous() if M else torch.zeros((0, 2), dtype=torch.int32, device=dev)
    nseg = num_nodes * T if by_source else num_nodes
    row_ptr = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    gather_row = torch.empty(M, dtype=torch.int32, device=dev)
    msg_perm = torch.empty(M, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = lib.ggnn_csr_workspace_bytes(M, num_nodes)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    off = (ctypes.c_int64 * (T + 1))(*type_off)
    fn = lib.ggnn_build_source_csr if by_source else lib.ggnn_build_target_csr
    check(fn(_ptr(adj), off, T, num_nodes, M, _ptr(row_ptr), _ptr(gather_row), _ptr(msg_perm), _ptr(err), _ptr(ws),
             ws_bytes, _stream()))
    if validate and M and int(err.item()) != 0:
        raise IndexError("adjacency list holds a node id outside [0, %d)" % num_nodes)
    return MessageIndex(adj, type_off, row_ptr, gather_row, msg_perm, nseg, T)


def build_message_index(adjacency_lists: Sequence[torch.Tensor], num_nodes: int,
                        validate: bool = True) -> MessageIndex:
    """chem_tensorflow_sparse.py:120-129 plus the stable bucketing by target that makes the segment
    sum atomics-free.  adjacency_lists: T tensors int32 [E_t,2] (src,dst) on the GPU; E_t may be 0
    (:346-347).  With validate=True an out-of-range src/dst raises IndexError (TF-CPU raises
    InvalidArgument at the gather / segment_sum); this costs one device->host sync, once per batch."""
    return _build_index(adjacency_lists, num_nodes, validate, by_source=False)


def build_source_index(adjacency_lists: Sequence[torch.Tensor], num_nodes: int) -> MessageIndex:
    """The transpose index for the backward pass: V*T segments keyed by (src*T + type), gathering dst rows."""
    return _build_index(adjacency_lists, num_nodes, False, by_source=True)


USE_SLOT_HEADS = os.environ.get("GGNN_SLOT_HEADS", "1") != "0"


def slot_heads(owner, row_ptr: torch.Tensor, gather_row: torch.Tensor, num_segments: int) -> Optional[torch.Tensor]:
    """[num_segments, 4] int32 gather rows of the first four slots of every segment (-1 padded), built once per index and
    cached on `owner` (ggnn_build_slot_heads): the segment-sum kernels then need one dependent load level less."""
    if not USE_SLOT_HEADS or num_segments == 0:
        return None
    cached = getattr(owner, "_slot_heads", None)
    if cached is not None and cached[0] is gather_row:
        return cached[1]
    lib = _lib.load()
    heads = torch.empty((num_segments, 4), dtype=torch.int32, device=row_ptr.device)
    check(lib.ggnn_build_slot_heads(_ptr(row_ptr), _ptr(gather_row), _ptr(heads), num_segments, _stream()))
    owner._slot_heads = (gather_row, heads)
    return heads


def _segment_sum(name, Hrows, row_ptr, gather_row, heads, nin, bias, use_avg, out, V, D, T, accumulate=False):
    lib = _lib.load()
    if heads is not None:
        _launch(name, lambda: lib.ggnn_gather_segment_sum_heads_f32(
            _ptr(Hrows), _ptr(row_ptr), _ptr(gather_row), _ptr(heads), _ptr(nin), _ptr(bias), 1 if use_avg else 0, _ptr(out), V, D, T,
            1 if accumulate else 0, _stream()))
    elif accumulate:
        _launch(name, lambda: lib.ggnn_gather_segment_sum_acc_f32(_ptr(Hrows), _ptr(row_ptr), _ptr(gather_row), _ptr(out), V, D, _stream()))
    else:
        _launch(name, lambda: lib.ggnn_gather_segment_sum_f32(_ptr(Hrows), _ptr(row_ptr), _ptr(gather_row), _ptr(nin), _ptr(bias),
                                                              1 if use_avg else 0, _ptr(out), V, D, T, _stream()))
    return out


def msg_transform(h: torch.Tensor, edge_weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """H[v, t*D:(t+1)*D] = h[v] @ edge_weights[t]   (chem_tensorflow_sparse.py:160-164, all types
    in one FP32-MFMA GEMM).  h [V,D], edge_weights [T,D,D] -> H [V, T*D]."""
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(edge_weights, torch.float32, "edge_weights")
    V, D = h.shape
    T = edge_weights.shape[0]
    if edge_weights.shape != (T, D, D):
        raise ValueError("edge_weights must be [T,D,D]")
    if out is None:
        out = torch.empty((V, T * D), dtype=torch.float32, device=h.device)
    else:
        _req(out, torch.float32, "out")
        if out.shape != (V, T * D):
            raise ValueError("out must be [V, T*D]")
    _launch("msg_transform", lambda: lib.ggnn_msg_transform_f32(_ptr(h), D, _ptr(edge_weights), _ptr(out), V, D, T, _stream()))
    return out


def gather_segment_sum(H: torch.Tensor, index: MessageIndex, num_incoming_edges_per_type: Optional[torch.Tensor],
                       edge_biases: Optional[torch.Tensor], use_avg: bool,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """incoming[v] = (sum of H rows of the messages into v [+ nin[v] @ edge_biases]) [/ (sum_t nin[v,t] + 1e-7)]
    (chem_tensorflow_sparse.py:160-162,168,198-209).  H [V, T*D] from msg_transform."""
    lib = _lib.load()
    _req(H, torch.float32, "H")
    V, T = index.num_nodes, index.num_edge_types
    if H.shape[0] != V or H.shape[1] % T:
        raise ValueError("H must be [V, T*D]")
    D = H.shape[1] // T
    nin = num_incoming_edges_per_type
    if nin is not None:
        _req(nin, torch.float32, "num_incoming_edges_per_type")
        if nin.shape != (V, T):
            raise ValueError("num_incoming_edges_per_type must be [V,T]")
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
        if edge_biases.shape != (T, D):
            raise ValueError("edge_biases must be [T,D]")
    if out is None:
        out = torch.empty((V, D), dtype=torch.float32, device=H.device)
    else:
        _req(out, torch.float32, "out")
    return _segment_sum("gather_segment_sum", H, index.row_ptr, index.gather_row, slot_heads(index, index.row_ptr, index.gather_row, V),
                        nin, edge_biases, use_avg, out, V, D, T)


def gru_workspace(V: int, D: int, device) -> torch.Tensor:
    lib = _lib.load()
    return torch.empty(lib.ggnn_gru_workspace_bytes(V, D) // 4, dtype=torch.float32, device=device)


def gru(x_segs: Sequence[torch.Tensor], h: torch.Tensor, Wg: torch.Tensor, bg: torch.Tensor, Wc: torch.Tensor,
        bc: torch.Tensor, activation: str = "tanh", out: Optional[torch.Tensor] = None,
        ws: Optional[torch.Tensor] = None, save: Optional[dict] = None, two_launch: bool = False,
        fmt: Optional[int] = None) -> torch.Tensor:
    """TF-1.3 GRUCell on x = concat(x_segs) without materialising the concat
    (chem_tensorflow_sparse.py:211-216).  save: optional dict receiving 'r','u','c' [V,D] tensors.
    two_launch=True forces the un-fused gates + candidate kernels (the path large D takes).
    On raw weights the products run in the exact BF16X3 operand format (ggnn_gru_f32); fmt = formats.F16X2 packs the weights
    in the two-piece f16 format and runs the fused launch in it (the CALLER vouches for the operand range, see formats.py)."""
    lib = _lib.load()
    if fmt is not None and int(fmt) != GRU_FMT_EXACT and not two_launch and lib.ggnn_gru_is_fused(h.shape[1]) \
            and len(x_segs) <= GRU_FUSED_MAX_INPUTS:
        _req(Wg, torch.float32, "Wg"); _req(Wc, torch.float32, "Wc")
        # (the images are cached per weight version and format: this branch runs once per timestep on the non-gather training path)
        packed = PACKED.gru(Wg, Wc, len(x_segs), h.shape[1], int(fmt))
        return gru_packed(x_segs, h, packed, bg, bc, activation, out=out, fmt=int(fmt), save=save)
    _req(h, torch.float32, "h")
    V, D = h.shape
    nx = len(x_segs)
    for i, x in enumerate(x_segs):
        _req(x, torch.float32, "x_segs[%d]" % i)
        if x.shape != (V, D):
            raise ValueError("x_segs[%d] must be [V,D]" % i)
    for n, w, shp in (("Wg", Wg, ((nx + 1) * D, 2 * D)), ("bg", bg, (2 * D,)), ("Wc", Wc, ((nx + 1) * D, D)), ("bc", bc, (D,))):
        _req(w, torch.float32, n)
        if tuple(w.shape) != shp:
            raise ValueError("%s must have shape %s, got %s" % (n, shp, tuple(w.shape)))
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    if out is None:
        out = torch.empty_like(h)
    if ws is None:
        ws = gru_workspace(V, D, h.device)
    sr = su = sc = None
    if save is not None:
        sr = save["r"] = torch.empty_like(h)
        su = save["u"] = torch.empty_like(h)
        sc = save["c"] = torch.empty_like(h)
    segs = (ctypes.c_void_p * nx)(*[x.data_ptr() for x in x_segs])
    if not two_launch and (_timing is None or lib.ggnn_gru_is_fused(D)):
        _launch("gru_fused[nx=%d]" % nx, lambda: lib.ggnn_gru_f32(
            segs, nx, _ptr(h), _ptr(Wg), _ptr(bg), _ptr(Wc), _ptr(bc), _ptr(out), _ptr(ws), ws.numel() * 4,
            _ptr(sr), _ptr(su), _ptr(sc), V, D, act, _stream()))
    else:   # un-fused sizes: the same two launches, individually bracketed by events
        if ws.numel() < 2 * V * D:
            raise ValueError("GRU workspace too small")
        rh = ws[:V * D]
        u = su if su is not None else ws[V * D:2 * V * D]
        _launch("gru_gates[nx=%d]" % nx, lambda: lib.ggnn_gru_gates_f32(segs, nx, _ptr(h), _ptr(Wg), _ptr(bg), _ptr(rh),
                                                                         _ptr(u), _ptr(sr), V, D, _stream()))
        _launch("gru_candidate[nx=%d]" % nx, lambda: lib.ggnn_gru_candidate_f32(
            segs, nx, _ptr(rh), _ptr(h), _ptr(u), _ptr(Wc), _ptr(bc), _ptr(out), _ptr(sc), V, D, act, _stream()))
    return out


def gemm(a_segs: Sequence[torch.Tensor], B: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = concat(a_segs, dim=1) @ B on the FP32-MFMA kernel (no concat materialised).  Segments are
    [M,D] tensors (contiguous, or equal-stride column slices of one wider row-major matrix)."""
    lib = _lib.load()
    M, D = a_segs[0].shape
    lda = a_segs[0].stride(0) if M > 1 else D
    for i, a in enumerate(a_segs):
        if not a.is_cuda or a.dtype != torch.float32:
            raise TypeError("a_segs[%d] must be a float32 CUDA/HIP tensor" % i)
        if a.shape != (M, D) or a.stride(1) != 1 or (M > 1 and a.stride(0) != lda):
            raise ValueError("all segments must be [M,D] row-major with one common row stride")
    _req(B, torch.float32, "B")
    K, N = B.shape
    if K != len(a_segs) * D:
        raise ValueError("B must be [nseg*D, N]")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=B.device)
    segs = (ctypes.c_void_p * len(a_segs))(*[a.data_ptr() for a in a_segs])
    _launch("gemm[K=%d,N=%d]" % (K, N), lambda: lib.ggnn_gemm_f32(segs, len(a_segs), D, lda, _ptr(B), N, _ptr(out), N, M, N, _stream()))
    return out


def gemm_tn(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """x^T @ dy for tall operands ([M,K]^T [M,N] -> [K,N], M ~ 1e5): the weight-gradient product of the backward
    pass on ggnn_gemm_tn_f32 (rows split over the whole GPU, deterministic reduction).  x, dy: row-major (any row
    stride), dy with a row stride and N that are multiples of 4."""
    lib = _lib.load()
    for name, t in (("x", x), ("dy", dy)):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[0] > 0 and t.stride(1) != 1):
            raise TypeError("%s must be a 2-D float32 CUDA/HIP tensor with unit column stride" % name)
    M, K = x.shape
    N = dy.shape[1]
    if dy.shape[0] != M:
        raise ValueError("x and dy must have the same number of rows")
    if M == 0:
        return torch.zeros((K, N), dtype=torch.float32, device=x.device)
    if M > 1 and (dy.stride(0) % 4 != 0 or dy.data_ptr() % 16 != 0):
        # the kernel reads dy in float4s: a row stride that is no multiple of 4 floats (a contiguous [M, 6] or [M, 513]) or a
        # misaligned view goes through ONE copy whose rows are padded to a multiple of 4 (zero columns add nothing to the product)
        n_pad = (N + 3) // 4 * 4
        buf = torch.zeros((M, n_pad), dtype=torch.float32, device=dy.device)
        buf[:, :N] = dy
        return gemm_tn(x, buf)[:, :N].contiguous() if n_pad != N else gemm_tn(x, buf)
    if N > 512 or N % 4 != 0:
        # the kernel takes N <= 512, N % 4 == 0: wider products go through in 512-column views (it takes any row stride), a ragged
        # tail (N % 4 columns: readout widths like 1 or 2) through a zero-padded copy of those columns
        n4 = N // 4 * 4
        parts = [gemm_tn(x, dy[:, c:min(c + 512, n4)]) for c in range(0, n4, 512)]
        if n4 < N:
            tail = torch.zeros((M, 4), dtype=torch.float32, device=dy.device)
            tail[:, :N - n4] = dy[:, n4:]
            parts.append(gemm_tn(x, tail)[:, :N - n4])
        return torch.cat(parts, dim=1)
    lda = x.stride(0) if M > 1 else K
    ldb = dy.stride(0) if M > 1 else N
    out = torch.empty((K, N), dtype=torch.float32, device=x.device)
    ws_bytes = lib.ggnn_gemm_tn_workspace_bytes(M, K, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _launch("gemm_tn[K=%d,N=%d]" % (K, N), lambda: lib.ggnn_gemm_tn_f32(_ptr(x), lda, _ptr(dy), ldb, _ptr(out), M, K, N,
                                                                       _ptr(ws), ws_bytes, _stream()))
    return out


def xty(x_segs: Sequence[torch.Tensor], dy: torch.Tensor, x_rows: Optional[torch.Tensor] = None,
        row_off: Optional[Sequence[int]] = None, ones_row: bool = False, add_to: Optional[torch.Tensor] = None,
        add_bias_to: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Weight-gradient product  concat(x_segs, dim=1)^T @ dy  on ggnn_xty_f32 (no concat materialised; deterministic).
    x_segs: [M', Dseg] float32 tensors with unit column stride (any row stride: column slices are fine), Dseg % 4 == 0;
    dy [M, N], N % 4 == 0, N <= 256.  Row-gathered products (x_rows) take K + ones_row <= 128 and N <= 128; every other shape
    in that domain has a kernel (include/ggnn_hip.h; ggnn_xty_describe tells which).
    x_rows (int32 [M]): row r of the X operand is x_segs[.][x_rows[r]] (edge-weight gradients on compact rows).
    row_off (host ints [B+1]): B independent products over the row ranges -> [B, K, N]; default one product -> [K, N].
    ones_row: the result has K + 1 rows, the last one the column sums of dy (the bias gradient next to the weight gradient).
    add_to (contiguous float32, B*K*N elements) [, add_bias_to (N or B*N elements; needs ones_row)]: the product (and the column
    sums) are ADDED into these buffers by the reduction kernel itself and nothing is returned (gradient accumulation)."""
    lib = _lib.load()
    nseg = len(x_segs)
    Dseg = x_segs[0].shape[1]
    if nseg > 4:
        # the kernel takes 4 column segments of X: more (layers with more than 2 residual inputs) are row blocks of the product
        if row_off is not None or x_rows is not None:
            raise ValueError("batched / row-gathered products take at most 4 segments")
        N = dy.shape[1]
        groups = [list(x_segs[i:i + 4]) for i in range(0, nseg, 4)]
        if add_to is not None:
            dst = add_to.view(nseg * Dseg, N)
            k0 = 0
            for gi, grp in enumerate(groups):
                last = gi == len(groups) - 1
                xty(grp, dy, ones_row=ones_row and last, add_to=dst[k0:k0 + len(grp) * Dseg], add_bias_to=add_bias_to if last else None)
                k0 += len(grp) * Dseg
            return None
        parts = [xty(grp, dy, ones_row=ones_row and gi == len(groups) - 1) for gi, grp in enumerate(groups)]
        return torch.cat(parts, dim=0)
    for i, x in enumerate(x_segs):
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != Dseg or (x.shape[0] > 1 and x.stride(1) != 1):
            raise TypeError("x_segs[%d] must be a [M, %d] float32 CUDA/HIP tensor with unit column stride" % (i, Dseg))
    if not dy.is_cuda or dy.dtype != torch.float32 or dy.dim() != 2 or (dy.shape[0] > 1 and dy.stride(1) != 1):
        raise TypeError("dy must be a 2-D float32 CUDA/HIP tensor with unit column stride")
    M, N = dy.shape
    K = nseg * Dseg
    batched = row_off is not None
    offs = [0, M] if row_off is None else [int(o) for o in row_off]
    B = len(offs) - 1
    Kout = K + 1 if ones_row else K
    if add_to is not None:
        if ones_row != (add_bias_to is not None):
            raise ValueError("add_to with ones_row needs add_bias_to (and vice versa)")
        for t, n in ((add_to, B * K * N), (add_bias_to, B * N)):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
                raise TypeError("accumulation buffers must be contiguous float32 CUDA/HIP tensors of %d elements" % n)
        out = None
    else:
        out = torch.empty((B, Kout, N), dtype=torch.float32, device=dy.device)
    m_max = max([offs[b + 1] - offs[b] for b in range(B)] + [0])
    ws_bytes = lib.ggnn_xty_workspace_bytes(m_max, K, N, B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device)
    segs = (ctypes.c_void_p * nseg)(*[x.data_ptr() for x in x_segs])
    ldx = (ctypes.c_int32 * nseg)(*[(x.stride(0) if x.shape[0] > 1 else Dseg) for x in x_segs])
    ro = (ctypes.c_int32 * (B + 1))(*offs)
    ldy = dy.stride(0) if M > 1 else N
    if x_rows is not None:
        _req(x_rows, torch.int32, "x_rows")
    if out is None:
        _launch("xty[K=%d,N=%d%s]" % (K, N, ",x%d" % B if batched else ""), lambda: lib.ggnn_xty_acc_f32(
            segs, nseg, Dseg, ldx, _ptr(x_rows), _ptr(dy), ldy, _ptr(add_to), _ptr(add_bias_to), 1, K, N, 1 if ones_row else 0, ro, B,
            _ptr(ws), ws_bytes, _stream()))
        return None
    _launch("xty[K=%d,N=%d%s]" % (K, N, ",x%d" % B if batched else ""), lambda: lib.ggnn_xty_f32(
        segs, nseg, Dseg, ldx, _ptr(x_rows), _ptr(dy), ldy, _ptr(out), K, N, 1 if ones_row else 0, ro, B, _ptr(ws), ws_bytes, _stream()))
    return out if batched else out[0]


def colsum(dy: torch.Tensor) -> torch.Tensor:
    """Deterministic column sums of a [M, N] float32 matrix (bias gradients)."""
    lib = _lib.load()
    M, N = dy.shape
    if N > 1024:                                       # (ggnn_colsum_f32 takes N <= 1024: wider matrices in 1024-column views)
        return torch.cat([colsum(dy[:, c:min(c + 1024, N)]) for c in range(0, N, 1024)])
    out = torch.empty(N, dtype=torch.float32, device=dy.device)
    ws_bytes = lib.ggnn_colsum_workspace_bytes(N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dy.device)
    _launch("colsum[N=%d]" % N, lambda: lib.ggnn_colsum_f32(_ptr(dy), dy.stride(0) if M > 1 else N, M, N, _ptr(out), _ptr(ws), ws_bytes, _stream()))
    return out


def segment_sum_rows_acc(rows: torch.Tensor, index, out: torch.Tensor) -> torch.Tensor:
    """out[s,:] += sum of rows[index.gather_row[slot],:] over the slots of segment s (ggnn_gather_segment_sum_acc_f32)."""
    lib = _lib.load()
    _req(rows, torch.float32, "rows"); _req(out, torch.float32, "out")
    return _segment_sum("gather_segment_sum_acc", rows, index.row_ptr, index.gather_row,
                        slot_heads(index, index.row_ptr, index.gather_row, index.num_nodes), None, None, False, out, index.num_nodes,
                        rows.shape[1], 1, accumulate=True)


def gru_bwd_is_fused(D: int) -> bool:
    return bool(_lib.load().ggnn_gru_bwd_is_fused(D))


def gru_bwd_fused(g, h, r, u, c, packed, nin, use_avg: bool, nx: int, activation: str, gather=None):
    """The GRU backward of one timestep in one launch (ggnn_gru_bwd_fused_f32) -> (dpc, dpg, rh, dh, [dx_0 .. dx_{nx-1}]);
    the last dx is d_incoming (already divided by the in-degree for mean aggregation).
    gather = (rows, heads): the incoming gradient is g[v] + the sum of the rows of `rows` named by the slot-head record heads[v]
    (ggnn_gru_bwd_fused_gather_f32)."""
    lib = _lib.load()
    V, D = h.shape
    T = nin.shape[1] if nin is not None else 1
    dev = h.device
    dpc = torch.empty_like(h); rh = torch.empty_like(h); dh = torch.empty_like(h)
    dpg = torch.empty((V, 2 * D), dtype=torch.float32, device=dev)
    dx = [torch.empty_like(h) for _ in range(nx)]
    dxp = (ctypes.c_void_p * nx)(*[t.data_ptr() for t in dx])
    if gather is not None:
        rows, heads = gather
        _req(rows, torch.float32, "rows"); _req(heads, torch.int32, "heads")
        _launch("gru_bwd_fused_gather[nx=%d]" % nx, lambda: lib.ggnn_gru_bwd_fused_gather_f32(
            _ptr(g), _ptr(rows), _ptr(heads), _ptr(h), _ptr(r), _ptr(u), _ptr(c), _ptr(packed), _ptr(dpc), _ptr(dpg), _ptr(rh), _ptr(dh),
            dxp, _ptr(nin), T, 1 if use_avg else 0, nx, V, D, ACT_IDS[activation.lower()], _stream()))
        return dpc, dpg, rh, dh, dx
    _launch("gru_bwd_fused[nx=%d]" % nx, lambda: lib.ggnn_gru_bwd_fused_f32(
        _ptr(g), _ptr(h), _ptr(r), _ptr(u), _ptr(c), None, None, _ptr(packed), _ptr(dpc), _ptr(dpg), _ptr(rh), _ptr(dh), dxp,
        _ptr(nin), T, 1 if use_avg else 0, nx, V, D, ACT_IDS[activation.lower()], _stream()))
    return dpc, dpg, rh, dh, dx


def weighted_segment_sum(rows: torch.Tensor, index: "SegmentIndex", weight_id: torch.Tensor, weights: torch.Tensor,
                         out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """out[s] (+)= sum over the slots of segment s of weights[weight_id[slot]] * rows[index.gather_row[slot]]."""
    lib = _lib.load()
    _req(rows, torch.float32, "rows"); _req(weights, torch.float32, "weights"); _req(weight_id, torch.int32, "weight_id")
    D = rows.shape[1]
    nseg = index.num_nodes
    if out is None:
        out = torch.empty((nseg, D), dtype=torch.float32, device=rows.device)
    _launch("weighted_segment_sum", lambda: lib.ggnn_weighted_segment_sum_f32(
        _ptr(rows), _ptr(index.row_ptr), _ptr(index.gather_row), _ptr(weight_id), _ptr(weights), _ptr(out), 1 if accumulate else 0,
        nseg, D, _stream()))
    return out


def attn_backward_target(H: torch.Tensor, h: torch.Tensor, d_att: torch.Tensor, index: MessageIndex, type_factors: torch.Tensor,
                         dh: torch.Tensor):
    """Target-side pass of the propagation-attention backward (ggnn_attn_bwd_target_f32): adds sum_e ds_e f_t h[src_e] to dh[v]
    and returns the per-message (coef_a, coef_s, dfac), indexed by message id."""
    lib = _lib.load()
    V, D = h.shape
    T, M = index.num_edge_types, index.num_messages
    dev = h.device
    ca = torch.empty(max(M, 1), dtype=torch.float32, device=dev); cs = torch.empty_like(ca); df = torch.empty_like(ca)
    _launch("attn_bwd_target", lambda: lib.ggnn_attn_bwd_target_f32(
        _ptr(H), _ptr(h), _ptr(d_att), _ptr(index.row_ptr), _ptr(index.gather_row), _ptr(index.msg_perm), _ptr(type_factors), _ptr(ca),
        _ptr(cs), _ptr(df), _ptr(dh), 1, V, D, T, _stream()))
    return ca, cs, df


def range_sum(values: torch.Tensor, offsets: Sequence[int]) -> torch.Tensor:
    """out[b] = sum(values[offsets[b]:offsets[b+1]]), deterministic (ggnn_range_sum_f32)."""
    lib = _lib.load()
    B = len(offsets) - 1
    out = torch.empty(B, dtype=torch.float32, device=values.device)
    off = (ctypes.c_int64 * (B + 1))(*[int(o) for o in offsets])
    check(lib.ggnn_range_sum_f32(_ptr(values), off, B, _ptr(out), _stream()))
    return out


def bwd_dx(dY: torch.Tensor, nseg_y: int, WT: torch.Tensor, xcols: int, split_inc: bool, dx: Optional[torch.Tensor],
           dinc: Optional[torch.Tensor], nin: Optional[torch.Tensor], use_avg: bool, dh: Optional[torch.Tensor], acc_dx: bool,
           acc_dh: bool, D: int) -> None:
    """Q = dY WT with the backward epilogue of ggnn_bwd_dx_f32 (x columns -> dx / dinc, h columns -> dh)."""
    lib = _lib.load()
    V = dY.shape[0]
    K = WT.shape[1]
    T = nin.shape[1] if nin is not None else 1
    _launch("bwd_dx[K=%d]" % K, lambda: lib.ggnn_bwd_dx_f32(
        _ptr(dY), dY.stride(0) if V > 1 else dY.shape[1], nseg_y, _ptr(WT), K, _ptr(dx), xcols, 1 if split_inc else 0, _ptr(dinc),
        _ptr(nin), T, 1 if use_avg else 0, _ptr(dh), 1 if acc_dx else 0, 1 if acc_dh else 0, V, D, _stream()))


def act_bwd(g: torch.Tensor, out: torch.Tensor, activation: str) -> torch.Tensor:
    """dP = g * act'(out) (BasicRNNCell backward)."""
    lib = _lib.load()
    V, D = out.shape
    dP = torch.empty_like(out)
    _launch("act_bwd", lambda: lib.ggnn_act_bwd_f32(_ptr(g), _ptr(out), ACT_IDS[activation.lower()], _ptr(dP), V, D, _stream()))
    return dP


def cudnn_gru_train(x_segs: Sequence[torch.Tensor], h: torch.Tensor, Wg, bg, Wcx, bcx, Wch, bch):
    """ops.cudnn_gru that keeps what the backward pass needs: -> (h', r, u, c, hc)."""
    lib = _lib.load()
    V, D = h.shape
    nx = len(x_segs)
    out = torch.empty_like(h); c = torch.empty_like(h)
    ws_bytes = lib.ggnn_cudnn_gru_workspace_bytes(V, D)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=h.device)
    segs = (ctypes.c_void_p * nx)(*[_req(x, torch.float32, "x").data_ptr() for x in x_segs])
    _launch("cudnn_gru[nx=%d]" % nx, lambda: lib.ggnn_cudnn_gru_train_f32(segs, nx, _ptr(h), _ptr(Wg), _ptr(bg), _ptr(Wcx), _ptr(bcx),
                                                                          _ptr(Wch), _ptr(bch), _ptr(out), _ptr(c), _ptr(ws), ws_bytes,
                                                                          V, D, _stream()))
    n = V * D
    return out, ws[2 * n:3 * n].view(V, D), ws[n:2 * n].view(V, D), c, ws[3 * n:4 * n].view(V, D)


def cudnn_gru_bwd_stage(g, h, r, u, c, hc):
    """Element-wise part of the CudnnCompatibleGRUCell backward -> (dpc, dpg = [dpr|dpu], dh = g*u, dhc)."""
    lib = _lib.load()
    V, D = h.shape
    dpc = torch.empty_like(h); dh = torch.empty_like(h); dhc = torch.empty_like(h)
    dpg = torch.empty((V, 2 * D), dtype=torch.float32, device=h.device)
    _launch("cudnn_gru_bwd_stage", lambda: lib.ggnn_cudnn_gru_bwd_stage_f32(_ptr(g), _ptr(h), _ptr(r), _ptr(u), _ptr(c), _ptr(hc),
                                                                             _ptr(dpc), _ptr(dpg), _ptr(dh), _ptr(dhc), V, D, _stream()))
    return dpc, dpg, dh, dhc


def dropout(x: torch.Tensor, keep_prob: float, seed: int, row_key: Optional[torch.Tensor] = None, row_key_base: int = 0,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tf.nn.dropout with the counter-based mask of ggnn_dropout_f32: x / keep * floor(keep + U(seed, row key, column)).
    x [rows, cols] (or [cols]: one row) contiguous float32; row_key: optional int64 [rows] (default row_key_base + row)."""
    lib = _lib.load()
    _req(x, torch.float32, "x")
    if x.dim() < 1:
        raise ValueError("x must have at least one dimension")
    cols = x.shape[-1]
    rows = x.numel() // cols if cols else 0
    if row_key is not None:
        _req(row_key, torch.int64, "row_key")
        if row_key.numel() != rows:
            raise ValueError("row_key must have one entry per row")
    if out is None:
        out = torch.empty_like(x)
    _launch("dropout", lambda: lib.ggnn_dropout_f32(_ptr(x), _ptr(out), _ptr(row_key), int(row_key_base),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, float(keep_prob), rows, cols, _stream()))
    return out


def unsorted_segment_sum(data: torch.Tensor, segment_ids: torch.Tensor, num_segments: int) -> torch.Tensor:
    """tf.unsorted_segment_sum (fp32 atomics; any id order).  data [M,D] or [M], ids [M] int32."""
    lib = _lib.load()
    _req(data, torch.float32, "data"); _req(segment_ids, torch.int32, "segment_ids")
    M = data.shape[0]
    D = 1 if data.dim() == 1 else data.shape[1]
    out = torch.empty((num_segments,) if data.dim() == 1 else (num_segments, D), dtype=torch.float32, device=data.device)
    check(lib.ggnn_unsorted_segment_sum_f32(_ptr(data), _ptr(segment_ids), _ptr(out), M, D, num_segments, _stream()))
    return out


def segment_sum_rows_by_index(rows: torch.Tensor, index: MessageIndex, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[s,:] = sum of rows[index.gather_row[slot],:] over the slots of segment s -- the plain
    gather/segment-sum kernel without epilogue.  With a source index (build_source_index) and
    rows = d_incoming [V,D] this is the backward of the forward gather: out = dH viewed as [V*T, D]."""
    lib = _lib.load()
    _req(rows, torch.float32, "rows")
    D = rows.shape[1]
    nseg = index.num_nodes
    if out is None:
        out = torch.empty((nseg, D), dtype=torch.float32, device=rows.device)
    return _segment_sum("gather_segment_sum_bwd", rows, index.row_ptr, index.gather_row,
                        slot_heads(index, index.row_ptr, index.gather_row, nseg), None, None, False, out, nseg, D, 1)


def dense_aggregate(adjacency: torch.Tensor, Hm: torch.Tensor, edge_biases: Optional[torch.Tensor],
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acts = sum_e A_e (h W_e + b_e)  (chem_tensorflow_dense.py:103-112).
    adjacency [b,e,v,v] f32, Hm [b*v, e*D] (msg_transform output), edge_biases [e,D] or None -> [b*v, D]."""
    lib = _lib.load()
    _req(adjacency, torch.float32, "adjacency"); _req(Hm, torch.float32, "Hm")
    b, E, v, v2 = adjacency.shape
    if v != v2 or Hm.shape[0] != b * v or Hm.shape[1] % E:
        raise ValueError("shape mismatch between adjacency [b,e,v,v] and Hm [b*v, e*D]")
    D = Hm.shape[1] // E
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
        if edge_biases.shape != (E, D):
            raise ValueError("edge_biases must be [e,D]")
    if out is None:
        out = torch.empty((b * v, D), dtype=torch.float32, device=Hm.device)
    _launch("dense_aggregate", lambda: lib.ggnn_dense_aggregate_f32(_ptr(adjacency), _ptr(Hm), _ptr(edge_biases), _ptr(out),
                                                                   b, v, E, D, _stream()))
    return out


def dense_propagate_supported(v: int, E: int, D: int) -> bool:
    return bool(_lib.load().ggnn_dense_propagate_supported(int(v), int(E), int(D)))


def dense_propagate(h0: torch.Tensor, adjacency: torch.Tensor, edge_packed: torch.Tensor, gru_packed: torch.Tensor,
                    edge_biases: Optional[torch.Tensor], bg: torch.Tensor, bc: torch.Tensor, steps: int,
                    fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
    """The whole dense forward (chem_tensorflow_dense.py:93-117) in one launch, graph-resident (ggnn_dense_propagate_f32).
    h0 [b,v,D], adjacency [b,e,v,v]; edge_packed = PackedWeights.dense_edge(W [e,D,D]); gru_packed = PackedWeights.dense_gru(Wg, Wc).
    fmt: operand format of the kernel's products (exact by default; formats.F16X2 when the caller has proven its range)."""
    lib = _lib.load()
    _req(h0, torch.float32, "h0"); _req(adjacency, torch.float32, "adjacency")
    b, v, D = h0.shape
    E = adjacency.shape[1]
    if adjacency.shape != (b, E, v, v):
        raise ValueError("adjacency must be [b,e,v,v]")
    for t, n, name in ((bg, 2 * D, "bg"), (bc, D, "bc")):
        _req(t, torch.float32, name)
        if t.numel() != n:
            raise ValueError("%s must have %d elements" % (name, n))
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
        if edge_biases.numel() != E * D:
            raise ValueError("edge_biases must be [e,D]")
    out = torch.empty_like(h0)
    _launch("dense_propagate[steps=%d]" % steps, lambda: lib.ggnn_dense_propagate_f32(
        _ptr(h0), _ptr(adjacency), _ptr(edge_packed), _ptr(gru_packed), _ptr(edge_biases), _ptr(bg), _ptr(bc), _ptr(out), b, v, E, D,
        int(steps), int(fmt), _stream()))
    return out


def dense_train_supported(v: int, E: int, D: int) -> bool:
    """Whether the graph-resident training route (dense_propagate_save / dense_propagate_bwd) exists for the shape: the split-form
    forward's shapes on the split matrix path, where the backward kernel's LDS blocks fit."""
    return bool(_lib.load().ggnn_dense_train_supported(int(v), int(E), int(D)))


def dense_propagate_save(h0: torch.Tensor, adjacency: torch.Tensor, edge_packed: torch.Tensor, gru_packed: torch.Tensor,
                         edge_biases: Optional[torch.Tensor], bg: torch.Tensor, bc: torch.Tensor, steps: int,
                         fmt: int = GRU_FMT_EXACT):
    """dense_propagate that also keeps what the backward needs (ggnn_dense_propagate_save_f32) -> (out [b,v,D], saved
    [6, steps, b*v, D]: the entering state h_t, the aggregated messages x_t, r, u, c, r*h_t, each stacked over the timesteps).  `out` is
    dense_propagate's bit for bit in the same format."""
    lib = _lib.load()
    _req(h0, torch.float32, "h0"); _req(adjacency, torch.float32, "adjacency")
    if h0.dim() != 3 or adjacency.dim() != 4:
        raise ValueError("h0 must be [b,v,D] and adjacency [b,e,v,v]")
    b, v, D = h0.shape
    E = adjacency.shape[1]
    if adjacency.shape != (b, E, v, v):
        raise ValueError("adjacency must be [b,e,v,v]")
    for t, n, name in ((bg, 2 * D, "bg"), (bc, D, "bc")):
        _req(t, torch.float32, name)
        if t.numel() != n:
            raise ValueError("%s must have %d elements" % (name, n))
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
        if edge_biases.numel() != E * D:
            raise ValueError("edge_biases must be [e,D]")
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    out = torch.empty_like(h0)
    saved = torch.empty((6, steps, b * v, D), dtype=torch.float32, device=h0.device)
    _launch("dense_propagate_save[steps=%d]" % steps, lambda: lib.ggnn_dense_propagate_save_f32(
        _ptr(h0), _ptr(adjacency), _ptr(edge_packed), _ptr(gru_packed), _ptr(edge_biases), _ptr(bg), _ptr(bc), _ptr(out), b, v, E, D,
        steps, int(fmt), _ptr(saved), saved.numel() * 4, _stream()))
    return out, saved


def dense_bwd_pack(W: torch.Tensor, Wg: torch.Tensor, Wc: torch.Tensor) -> torch.Tensor:
    """The 6 + E transposed split images the graph-resident backward consumes (ggnn_dense_bwd_pack_f32); W [E,D,D], Wg [2D,2D],
    Wc [2D,D].  PackedWeights.dense_bwd caches them per weight version."""
    lib = _lib.load()
    _req(W, torch.float32, "edge_weights"); _req(Wg, torch.float32, "Wg"); _req(Wc, torch.float32, "Wc")
    if W.dim() != 3 or W.shape[1] != W.shape[2]:
        raise ValueError("edge_weights must be [e,D,D]")
    E, D = W.shape[0], W.shape[1]
    if tuple(Wg.shape) != (2 * D, 2 * D) or tuple(Wc.shape) != (2 * D, D):
        raise ValueError("Wg must be [2D,2D] and Wc [2D,D]")
    nbytes = lib.ggnn_dense_bwd_packed_bytes(D, E)
    if not nbytes:
        raise ValueError("no graph-resident dense backward for hidden size %d" % D)
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=W.device)
    check(lib.ggnn_dense_bwd_pack_f32(_ptr(W), _ptr(Wg), _ptr(Wc), E, D, _ptr(packed), _stream()))
    return packed


def dense_propagate_bwd(d_out: torch.Tensor, adjacency: torch.Tensor, bwd_packed: torch.Tensor, saved: torch.Tensor,
                        need_d_h0: bool = True):
    """The backward of dense_propagate_save in one launch (ggnn_dense_propagate_bwd_f32) -> (d_h0 [b,v,D] or None, dpc [steps,b*v,D],
    dpg = [dpr|dpu] [steps,b*v,2D], dx [steps,b*v,D], dM [steps,b*v,E*D]): the gradient of the initial state and, stacked over the
    timesteps, the operands of the weight-gradient products."""
    lib = _lib.load()
    _req(d_out, torch.float32, "d_out"); _req(adjacency, torch.float32, "adjacency"); _req(saved, torch.float32, "saved")
    if d_out.dim() != 3 or adjacency.dim() != 4:
        raise ValueError("d_out must be [b,v,D] and adjacency [b,e,v,v]")
    b, v, D = d_out.shape
    E = adjacency.shape[1]
    if adjacency.shape != (b, E, v, v):
        raise ValueError("adjacency must be [b,e,v,v]")
    if saved.dim() != 4 or saved.shape[0] != 6 or saved.shape[2:] != (b * v, D):
        raise ValueError("saved must be dense_propagate_save's [6, steps, b*v, D]")
    steps = saved.shape[1]
    dev = d_out.device
    d_h0 = torch.empty_like(d_out) if need_d_h0 else None
    dpc = torch.empty((steps, b * v, D), dtype=torch.float32, device=dev)
    dpg = torch.empty((steps, b * v, 2 * D), dtype=torch.float32, device=dev)
    dx = torch.empty((steps, b * v, D), dtype=torch.float32, device=dev)
    dM = torch.empty((steps, b * v, E * D), dtype=torch.float32, device=dev)
    _launch("dense_propagate_bwd[steps=%d]" % steps, lambda: lib.ggnn_dense_propagate_bwd_f32(
        _ptr(d_out), _ptr(adjacency), _ptr(bwd_packed), _ptr(saved), b, v, E, D, steps, _ptr(d_h0), _ptr(dpc), _ptr(dpg), _ptr(dx),
        _ptr(dM), _stream()))
    return d_h0, dpc, dpg, dx, dM


def dense_edge_grad_supported(E: int, D: int) -> bool:
    """The shapes ggnn_dense_edge_grad_f32 has kernels for (the graph-resident route's: hidden size 32 / 64 / 100, 2 / 4 / 6 / 8 edge
    types)."""
    return int(D) in (32, 64, 100) and int(E) in (2, 4, 6, 8)


def dense_edge_grad(h: torch.Tensor, dM: torch.Tensor, nin: Optional[torch.Tensor] = None, dx: Optional[torch.Tensor] = None,
                    dW: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False,
                    ws: Optional[torch.Tensor] = None):
    """Edge-weight and edge-bias gradients of the dense model in one deterministic product (ggnn_dense_edge_grad_f32):
    dW [E,D,D] = per edge type h^T dM_e, db [E,D] = nin^T dx with row n of the stack using nin[n % rows_per_step].
    h, dx [N,D] and dM [N,E*D] are dense_propagate_save's saved[0] and dense_propagate_bwd's dx / dM stacked over the timesteps
    (N = steps*b*v); nin [b*v, E] the in-degrees of ONE timestep, or None for a model without edge biases (then dx and db are unused).
    dW / db given: the results go there (contiguous float32, E*D*D / E*D elements), ADDED to their contents with accumulate.
    ws: a uint8 workspace of at least ggnn_dense_edge_grad_workspace_bytes(N, E, D) bytes (allocated when None).  -> (dW, db or None)."""
    lib = _lib.load()
    tensors = [("h", h), ("dM", dM)] + ([("nin", nin), ("dx", dx)] if nin is not None else []) + \
              [(n, t) for n, t in (("dW", dW), ("db", db if nin is not None else None)) if t is not None]
    for name, t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 CUDA/HIP tensor (the GGNN hot path has no CPU implementation)" % name)
        if t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned" % name)
    if h.dim() != 2 or dM.dim() != 2 or dM.shape[0] != h.shape[0] or h.shape[1] == 0 or dM.shape[1] % h.shape[1]:
        raise ValueError("h must be [N,D] and dM [N,E*D]")
    N, D = h.shape
    E = dM.shape[1] // D
    if not dense_edge_grad_supported(E, D):
        raise ValueError("dense_edge_grad: hidden size 32 / 64 / 100 and 2 / 4 / 6 / 8 edge types (got E=%d D=%d)" % (E, D))
    rows_per_step = 1
    if nin is not None:
        if nin.dim() != 2 or nin.shape[1] != E or nin.shape[0] < 1 or tuple(dx.shape) != (N, D):
            raise ValueError("nin must be [rows_per_step, E] with at least one row and dx [N, D]")
        rows_per_step = nin.shape[0]
    dev = h.device
    if dW is None:
        if accumulate:
            raise ValueError("accumulate needs the destination dW")
        dW = torch.empty((E, D, D), dtype=torch.float32, device=dev)
    elif dW.numel() != E * D * D:
        raise ValueError("dW must have E*D*D elements")
    if nin is None:
        db = None
    elif db is None:
        if accumulate:
            raise ValueError("accumulate needs the destination db")
        db = torch.empty((E, D), dtype=torch.float32, device=dev)
    elif db.numel() != E * D:
        raise ValueError("db must have E*D elements")
    ws_bytes = lib.ggnn_dense_edge_grad_workspace_bytes(N, E, D)
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < ws_bytes or ws.data_ptr() % 16:
        raise ValueError("ws must be a contiguous, 16-byte aligned uint8 CUDA/HIP tensor of at least %d bytes" % ws_bytes)
    _launch("dense_edge_grad[E=%d,D=%d]" % (E, D), lambda: lib.ggnn_dense_edge_grad_f32(
        _ptr(h), _ptr(dM), _ptr(nin), _ptr(dx), N, rows_per_step, E, D, _ptr(dW), _ptr(db), 1 if accumulate else 0, _ptr(ws), ws.numel(),
        _stream()))
    return dW, db


# ---- source-compacted message transform -----------------------------------------------------------------
@dataclass
class CompactSources:
    """Active (source node, edge type) pairs of a batch, type-major / node-ascending (built once per batch).

    pair_node     [R] int32   compact row -> source node
    type_row_off  list[T+1]   host: rows of type t are type_row_off[t] .. type_row_off[t+1]-1
    gather_row    [M] int32   message slot (MessageIndex order) -> compact row
    """
    pair_node: torch.Tensor
    type_row_off: List[int]
    gather_row: torch.Tensor

    @property
    def num_rows(self) -> int:
        return int(self.type_row_off[-1])


def compact_supported(D: int) -> bool:
    return bool(_lib.load().ggnn_msg_transform_compact_supported(D))


def gru_is_fused(D: int) -> bool:
    return bool(_lib.load().ggnn_gru_is_fused(D))


def gru_gather_fused(D: int) -> bool:
    """True when the fused GRU of this hidden size has the variant that gathers the segment sum inside the kernel
    (ggnn_gru_is_fused == 1: the whole-block kernels; the column-panel kernels of D = 128/192/256 report 2)."""
    return _lib.load().ggnn_gru_is_fused(D) == 1


def build_compact_sources(index: MessageIndex, type_row_off: Optional[Sequence[int]] = None) -> CompactSources:
    """Enumerate the (node, type) pairs that emit at least one message and re-target the segment-sum's
    gather rows at them.  index: the by-target MessageIndex of the batch (build_message_index).
    type_row_off (host ints [T+1]): the per-type row ranges, when the caller knows them (data_device sums per-molecule
    tables); otherwise they are read back from the device (one device->host sync)."""
    lib = _lib.load()
    T, V, M = index.num_edge_types, index.num_nodes, index.num_messages
    dev = index.adj.device
    lists = [index.adj[index.type_off[t]:index.type_off[t + 1]] for t in range(T)]
    src_index = build_source_index(lists, V)
    index._source_index = src_index                       # the backward pass wants the same structure
    pair_node = torch.empty(max(min(M, V * T), 1), dtype=torch.int32, device=dev)
    pair_id = torch.empty(max(V * T, 1), dtype=torch.int32, device=dev)
    off = torch.zeros(T + 1, dtype=torch.int32, device=dev)
    ws_bytes = lib.ggnn_compact_workspace_bytes(V, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(lib.ggnn_build_compact_sources(_ptr(src_index.row_ptr), V, T, _ptr(pair_node), _ptr(pair_id), _ptr(off), _ptr(ws),
                                         ws_bytes, _stream()))
    gather_c = torch.empty(M, dtype=torch.int32, device=dev)
    check(lib.ggnn_remap_gather_rows(_ptr(index.gather_row), _ptr(pair_id), _ptr(gather_c), M, _stream()))
    if type_row_off is None:
        type_row_off = [int(x) for x in off.cpu().tolist()]   # one device->host sync, once per batch
    else:
        type_row_off = [int(x) for x in type_row_off]
        if len(type_row_off) != T + 1:
            raise ValueError("type_row_off needs T + 1 entries")
        if os.environ.get("GGNN_CHECK_HOST_COUNTS", "0") != "0" and type_row_off != [int(x) for x in off.cpu().tolist()]:
            raise AssertionError("host-side pair counts %s differ from the device's %s" % (type_row_off, off.cpu().tolist()))
    return CompactSources(pair_node[:max(type_row_off[-1], 1)], type_row_off, gather_c)


def prepare_message_index(index: MessageIndex, hidden_size: int, compact: bool = True, training: bool = False,
                          type_row_off: Optional[Sequence[int]] = None) -> MessageIndex:
    """Everything the propagation derives from a batch's message index, built EAGERLY when the batch is packed (it
    used to be built lazily on the first forward of each batch, which put a cold pass -- three small launches and a
    device->host sync -- inside whatever region timed that forward): the active (source node, edge type) pairs of the
    compacted message transform for the hidden sizes that have one; training: also the transpose structures of the backward
    pass (CompactBackward and the slot heads of its segment sums) -- ~25 small launches that would otherwise run inside the
    first backward pass of every fresh batch, on the training stream, instead of on the packer's."""
    if compact and index.num_messages and compact_supported(hidden_size) and getattr(index, "_compact", None) is None:
        index._compact = build_compact_sources(index, type_row_off)
        slot_heads(index._compact, index.row_ptr, index._compact.gather_row, index.num_nodes)
    comp = getattr(index, "_compact", None)
    if training and comp is not None and comp.num_rows:
        bwd = compact_backward(index, comp)
        slot_heads(index, index.row_ptr, index.gather_row, index.num_nodes)
        for si in (bwd.rows_index, bwd.node_index, bwd.source_node_index):
            slot_heads(si, si.row_ptr, si.gather_row, si.num_nodes)
    return index


class SegmentIndex:
    """row_ptr / gather_row pair for segment_sum_rows_by_index (the fields of MessageIndex that kernel reads)."""

    def __init__(self, row_ptr: torch.Tensor, gather_row: torch.Tensor, num_nodes: int, msg: Optional[torch.Tensor] = None):
        self.row_ptr, self.gather_row, self.num_nodes = row_ptr, gather_row, num_nodes
        self.msg = msg                     # slot -> original message id (for per-message weights), where known


class CompactBackward:
    """Index structures of the compacted transform's backward pass (built once per batch, torch index arithmetic):

    rows_index   segments = compact rows (type-major): the message slots leaving (node,type) pair r, gather_row = dst
                 -> dHc[r] = sum of d_incoming[dst]            (the transpose of the forward gather)
    node_index   segments = nodes: the compact rows of node v (type ascending)
                 -> dh[v] += sum_t (dHc W_t^T)[row(v,t)]
    identity     CompactSources whose pair_node is arange(R): runs the compact transform kernel on [R,D] rows as they are
    """

    def __init__(self, index: MessageIndex, comp: CompactSources):
        V, T, M = index.num_nodes, index.num_edge_types, index.num_messages
        R = comp.num_rows
        dev = index.adj.device
        src = getattr(index, "_source_index", None)
        if src is None:
            lists = [index.adj[index.type_off[t]:index.type_off[t + 1]] for t in range(T)]
            src = index._source_index = build_source_index(lists, V)
        pn = comp.pair_node[:R].long()
        typ = torch.repeat_interleave(torch.arange(T, device=dev), torch.as_tensor(
            [comp.type_row_off[t + 1] - comp.type_row_off[t] for t in range(T)], device=dev), output_size=R)
        seg = pn * T + typ                                              # segment of the by-(src*T+type) index
        rp = src.row_ptr.long()
        start, length = rp[seg], rp[seg + 1] - rp[seg]
        ends = torch.cumsum(length, 0)
        rp_c = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        rp_c[1:] = ends.to(torch.int32)
        slots = torch.repeat_interleave(start - (ends - length), length, output_size=M) + torch.arange(M, device=dev)
        self.rows_index = SegmentIndex(rp_c, src.gather_row[slots].contiguous(), R, src.msg_perm[slots].contiguous())
        # messages leaving a NODE (all its types: the by-(src,type) segments of a node are consecutive)
        self.source_node_index = SegmentIndex(src.row_ptr[::T].contiguous(), src.gather_row, V, src.msg_perm)
        order = torch.sort(pn, stable=True)[1]                          # rows by node, type ascending inside a node
        rp_n = torch.zeros(V + 1, dtype=torch.int32, device=dev)
        per_node = torch.zeros(V, dtype=torch.int64, device=dev).scatter_add_(0, pn, torch.ones(1, dtype=torch.int64, device=dev).expand(R))
        rp_n[1:] = torch.cumsum(per_node, 0).to(torch.int32)                # (scatter_add, not bincount: no host read-back)
        self.node_index = SegmentIndex(rp_n, order.to(torch.int32).contiguous(), V)
        self.identity = CompactSources(torch.arange(max(R, 1), dtype=torch.int32, device=dev), comp.type_row_off, comp.gather_row)


def compact_backward(index: MessageIndex, comp: CompactSources) -> CompactBackward:
    bwd = getattr(comp, "_bwd", None)
    if bwd is None:
        bwd = comp._bwd = CompactBackward(index, comp)
    return bwd


def msg_transform_compact(h: torch.Tensor, edge_weights: torch.Tensor, comp: CompactSources,
                          out: Optional[torch.Tensor] = None, fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
    """Hc[r] = h[pair_node[r]] @ edge_weights[type(r)] for the active (node,type) pairs only
    (chem_tensorflow_sparse.py:160-164 without the duplicate / unused rows).  -> [R, D].
    fmt: operand format of the products (formats.BF16X3 exact, the default; F16X2 when the caller has proven its range)."""
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(edge_weights, torch.float32, "edge_weights")
    V, D = h.shape
    T = edge_weights.shape[0]
    if edge_weights.shape != (T, D, D) or len(comp.type_row_off) != T + 1:
        raise ValueError("edge_weights must be [T,D,D] matching the compact index")
    R = comp.num_rows
    if out is None:
        out = torch.empty((max(R, 1), D), dtype=torch.float32, device=h.device)
    ws_bytes = lib.ggnn_msg_transform_compact_workspace_bytes(D, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=h.device)
    off = (ctypes.c_int64 * (T + 1))(*comp.type_row_off)
    _launch("msg_transform_compact", lambda: lib.ggnn_msg_transform_compact_f32(
        _ptr(h), _ptr(edge_weights), _ptr(comp.pair_node), off, _ptr(out), _ptr(ws), ws_bytes, V, D, T, int(fmt), _stream()))
    return out


def gather_segment_sum_compact(Hc: torch.Tensor, index: MessageIndex, comp: CompactSources,
                               num_incoming_edges_per_type: Optional[torch.Tensor], edge_biases: Optional[torch.Tensor],
                               use_avg: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gather_segment_sum over compact transformed rows (Hc from msg_transform_compact)."""
    lib = _lib.load()
    _req(Hc, torch.float32, "Hc")
    V, T, D = index.num_nodes, index.num_edge_types, Hc.shape[1]
    nin = num_incoming_edges_per_type
    if nin is not None:
        _req(nin, torch.float32, "num_incoming_edges_per_type")
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
    if out is None:
        out = torch.empty((V, D), dtype=torch.float32, device=Hc.device)
    return _segment_sum("gather_segment_sum", Hc, index.row_ptr, comp.gather_row, slot_heads(comp, index.row_ptr, comp.gather_row, V),
                        nin, edge_biases, use_avg, out, V, D, T)


# ---- pre-packed weights ---------------------------------------------------------------------------------
def _image(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(nbytes // 4, dtype=torch.float32, device=like.device)


class PackedWeights:
    """The kernels' LDS stage images of weight tensors, one per (weight tensors, kind, format) and weight version (derived.Cache):
    the pack pre-pass runs once per weight version instead of once per launch.  Any in-place update of a weight bumps
    tensor._version and repacks; a view with other strides is another key, misses, and is refused by the packer's check."""

    def __init__(self):
        self._images = derived.Cache(1024)

    def gru(self, Wg: torch.Tensor, Wc: torch.Tensor, nx: int, D: int, fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
        """The fused GRU forward's stage images in the operand format `fmt` (formats.F16X2 / BF16X3; the launch that consumes
        them must be given the same format)."""
        def make():
            lib = _lib.load()
            _req(Wg, torch.float32, "Wg"); _req(Wc, torch.float32, "Wc")
            packed = _image(lib.ggnn_gru_packed_bytes(D, nx), Wg)
            check(lib.ggnn_gru_pack_weights_f32(_ptr(Wg), _ptr(Wc), nx, D, int(fmt), _ptr(packed), _stream()))
            return packed
        return self._images.get((Wg, Wc), ("gru", nx, D, int(fmt)), make)

    def dense_edge(self, W: torch.Tensor) -> torch.Tensor:
        """The E f32 stage images of the graph-resident dense kernel (ggnn_dense_edge_pack_f32), once per weight version."""
        def make():
            lib = _lib.load()
            _req(W, torch.float32, "edge_weights")
            T, D = W.shape[0], W.shape[1]
            packed = _image(lib.ggnn_dense_edge_packed_bytes(D, T), W)
            check(lib.ggnn_dense_edge_pack_f32(_ptr(W), T, D, _ptr(packed), _stream()))
            return packed
        return self._images.get((W,), "dense_edge", make)

    def dense_gru(self, Wg: torch.Tensor, Wc: torch.Tensor, D: int) -> torch.Tensor:
        """The six plain stage images of the graph-resident dense kernel (ggnn_dense_gru_pack_f32), once per weight version."""
        def make():
            lib = _lib.load()
            _req(Wg, torch.float32, "Wg"); _req(Wc, torch.float32, "Wc")
            packed = _image(lib.ggnn_dense_gru_packed_bytes(D), Wg)
            check(lib.ggnn_dense_gru_pack_f32(_ptr(Wg), _ptr(Wc), D, _ptr(packed), _stream()))
            return packed
        return self._images.get((Wg, Wc), ("dense_gru", D), make)

    def dense_bwd(self, W: torch.Tensor, Wg: torch.Tensor, Wc: torch.Tensor) -> torch.Tensor:
        """The transposed split images of the graph-resident dense backward (dense_bwd_pack), once per weight version."""
        return self._images.get((W, Wg, Wc), "dense_bwd", lambda: dense_bwd_pack(W, Wg, Wc))

    def gru_bwd(self, Wg: torch.Tensor, Wc: torch.Tensor, nx: int, D: int) -> torch.Tensor:
        """Transposed-block stage images of the fused GRU backward (ggnn_gru_bwd_fused_f32), once per weight version."""
        def make():
            lib = _lib.load()
            _req(Wg, torch.float32, "Wg"); _req(Wc, torch.float32, "Wc")
            packed = _image(lib.ggnn_gru_bwd_packed_bytes(D, nx), Wg)
            check(lib.ggnn_gru_bwd_fused_f32(None, None, None, None, None, _ptr(Wg), _ptr(Wc), _ptr(packed), None, None, None, None,
                                             None, None, 0, 0, nx, 0, D, 0, _stream()))
            return packed
        return self._images.get((Wg, Wc), ("gru_bwd", nx, D), make)

    def rnn(self, W: torch.Tensor, nx: int, D: int) -> torch.Tensor:
        """The nx + 1 exact bf16x3 stage images of the gather-fused BasicRNNCell (ggnn_rnn_pack_weights_f32), once per weight
        version.  (nx, D) must be in the supported set: rnn_fused_supported."""
        return self._images.get((W,), ("rnn", int(nx)), lambda: rnn_pack(W, nx))

    def rnn_panel(self, W: torch.Tensor, nx: int, D: int) -> torch.Tensor:
        """The (nx + 1) D / 64 exact bf16x3 panel images of the panel BasicRNNCell (ggnn_rnn_panel_pack_weights_f32), once per
        weight version.  (nx, D) must be in the supported set: rnn_panel_supported."""
        return self._images.get((W,), ("rnn_panel", int(nx)), lambda: rnn_panel_pack(W, nx))

    def rnn_bwd(self, W: torch.Tensor, nx: int, D: int) -> torch.Tensor:
        """The nx + 1 exact bf16x3 images of W_s^T of the fused BasicRNNCell backward (ggnn_rnn_bwd_pack_weights_f32), once per
        weight version.  (nx, D) must be in the supported set: rnn_bwd_fused_supported."""
        return self._images.get((W,), ("rnn_bwd", int(nx)), lambda: rnn_bwd_pack(W, nx))

    def cudnn(self, Wg: torch.Tensor, Wcx: torch.Tensor, Wch: torch.Tensor, nx: int, D: int) -> torch.Tensor:
        """The 3 (nx + 1) exact bf16x3 stage images of the fused CudnnCompatibleGRUCell (ggnn_cudnn_gru_pack_weights_f32), once per
        weight version.  (nx, D) must be in the supported set: cudnn_gru_fused_supported."""
        return self._images.get((Wg, Wcx, Wch), ("cudnn", int(nx)), lambda: cudnn_gru_pack(Wg, Wcx, Wch, nx))

    def _edge(self, W: torch.Tensor, fmt: int, transposed: bool) -> torch.Tensor:
        def make():
            lib = _lib.load()
            src = _req(W, torch.float32, "edge_weights")
            T, D = W.shape[0], W.shape[1]
            if transposed:
                src = W.transpose(1, 2).contiguous()          # (freed after the pack launch, on the stream that read it)
            packed = _image(lib.ggnn_msg_transform_compact_workspace_bytes(D, T), W)
            check(lib.ggnn_edge_weights_pack_f32(_ptr(src), T, D, int(fmt), _ptr(packed), _stream()))
            return packed
        return self._images.get((W,), ("edge_t" if transposed else "edge", int(fmt)), make)

    def edge(self, W: torch.Tensor, fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
        """The compacted transform's stage images of W [T, D, D] in the operand format `fmt` (the launch that consumes them must be
        given the same format)."""
        return self._edge(W, fmt, False)

    def edge_t(self, W: torch.Tensor, fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
        """The images of W.transpose(1, 2) -- edge(W.transpose(1, 2).contiguous()) byte for byte -- keyed on W itself: the
        backward's transform on W^T keeps no transposed copy and leaves no entry of one behind."""
        return self._edge(W, fmt, True)


# the process-wide images: every route of the package (ops.gru, the autograd path, the native steps) shares them
PACKED = PackedWeights()


def gru_packed(x_segs: Sequence[torch.Tensor], h: torch.Tensor, packed: torch.Tensor, bg: torch.Tensor, bc: torch.Tensor,
               activation: str = "tanh", out: Optional[torch.Tensor] = None,
               tile_counter: Optional[torch.Tensor] = None, fmt: int = GRU_FMT_EXACT, save: Optional[dict] = None) -> torch.Tensor:
    """ops.gru with pre-packed weight images (fused hidden sizes only).  tile_counter: optional int32 device tensor
    holding 0 (one element, consumed by this launch): dynamic tile hand-out, see include/ggnn_hip.h.
    fmt: the operand format `packed` was packed in (PackedWeights.gru).  save: optional dict receiving 'r','u','c'."""
    lib = _lib.load()
    _req(h, torch.float32, "h")
    V, D = h.shape
    nx = len(x_segs)
    for i, x in enumerate(x_segs):
        _req(x, torch.float32, "x_segs[%d]" % i)
        if x.shape != (V, D):
            raise ValueError("x_segs[%d] must be [V,D]" % i)
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    if out is None:
        out = torch.empty_like(h)
    segs = (ctypes.c_void_p * nx)(*[x.data_ptr() for x in x_segs])
    sr = su = sc = None
    if save is not None:
        sr = save["r"] = torch.empty_like(h)
        su = save["u"] = torch.empty_like(h)
        sc = save["c"] = torch.empty_like(h)
    _launch("gru_fused[nx=%d]" % nx, lambda: lib.ggnn_gru_packed_f32(
        segs, nx, _ptr(h), _ptr(packed), _ptr(bg), _ptr(bc), _ptr(out), _ptr(sr), _ptr(su), _ptr(sc), V, D, act, int(fmt),
        _ptr(tile_counter), _stream()))
    return out


def msg_transform_compact_packed(h: torch.Tensor, packed: torch.Tensor, T: int, comp: CompactSources,
                                 out: Optional[torch.Tensor] = None, fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
    """ops.msg_transform_compact with pre-packed edge-weight images (PackedWeights.edge(W, fmt): same fmt here)."""
    lib = _lib.load()
    _req(h, torch.float32, "h")
    V, D = h.shape
    R = comp.num_rows
    if out is None:
        out = torch.empty((max(R, 1), D), dtype=torch.float32, device=h.device)
    off = (ctypes.c_int64 * (T + 1))(*comp.type_row_off)
    _launch("msg_transform_compact", lambda: lib.ggnn_msg_transform_compact_f32(
        _ptr(h), None, _ptr(comp.pair_node), off, _ptr(out), _ptr(packed), packed.numel() * 4, V, D, T, int(fmt), _stream()))
    return out


MSG_TRANSFORM_FAMILIES = ("whole-block", "ring", "stationary")      # GGNN_MSG_TRANSFORM_* of include/ggnn_hip.h


def msg_transform_compact_describe(D: int, type_row_off: Sequence[int], fmt: int = GRU_FMT_EXACT) -> Dict[str, Any]:
    """What ggnn_msg_transform_compact_f32 launches in this process for these rows (the launchers' own selection and schedule; no
    GPU work): {'family': one of MSG_TRANSFORM_FAMILIES, 'fmt': 0 for the f32 MFMA or the GRU_FMT_* multiplied in, 'waves': per
    workgroup, 'workgroups': of the launch, 'types': [(workgroups, most tiles a wave walks, fewest), ...]}."""
    T = len(type_row_off) - 1
    off = (ctypes.c_int64 * (T + 1))(*type_row_off)
    out = (ctypes.c_int32 * (4 + 3 * max(T, 0)))()
    check(_lib.load().ggnn_msg_transform_compact_describe(int(D), T, off, int(fmt), out))
    return {"family": MSG_TRANSFORM_FAMILIES[out[0]], "fmt": out[1], "waves": out[2], "workgroups": out[3],
            "types": [tuple(out[4 + 3 * t:7 + 3 * t]) for t in range(T)]}


def _ptr_array(tensors):
    if tensors is None:
        return None
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def sparse_propagate(h0: torch.Tensor, index: MessageIndex, comp: Optional[CompactSources], nin: torch.Tensor, use_avg: bool,
                     layer_timesteps: Sequence[int], residuals: Sequence[Sequence[int]],
                     edge_w: Sequence[torch.Tensor], edge_packed: Optional[Sequence[torch.Tensor]],
                     edge_bias: Optional[Sequence[Optional[torch.Tensor]]],
                     Wg: Sequence[torch.Tensor], bg: Sequence[torch.Tensor], Wc: Sequence[torch.Tensor], bc: Sequence[torch.Tensor],
                     gru_packed: Optional[Sequence[torch.Tensor]], activation: str,
                     fuse_gather: Optional[bool] = None, gru_fmt: Optional[Sequence[int]] = None,
                     edge_fmt: Optional[Sequence[int]] = None, attn: Optional[Sequence[torch.Tensor]] = None,
                     rnn: Optional[Sequence[Sequence[Optional[torch.Tensor]]]] = None,
                     cudnn: Optional[Sequence[Sequence[Optional[torch.Tensor]]]] = None) -> List[torch.Tensor]:
    """chem_tensorflow_sparse.py:131-218 in ONE native call (ggnn_sparse_propagate_f32): returns
    node_states_per_layer[1:], the last entry being the final node representations.
    gru_fmt / edge_fmt: per layer, the operand format gru_packed[l] / edge_packed[l] was packed in (None: BF16X3 for every layer).
    fuse_gather (default FUSE_GATHER): gather the segment sum inside the GRU kernel where the layer allows it.
    attn: per layer, the [T] edge_type_attention_weights (:94-96): the propagation-attention form of the loop
    (ggnn_sparse_propagate_attn_f32; needs `comp`).
    rnn: (W per layer, b per layer, packed images per layer | None) of the BasicRNNCell: the RNN form of the loop
    (ggnn_sparse_propagate_rnn_f32; needs `comp`; Wg / bg / Wc / bc / gru_packed are not read).
    cudnn: (Wg, bg, Wcx, bcx, Wch, bch, packed images | None), each per layer, of the CudnnCompatibleGRUCell: the Cudnn form of the
    loop (ggnn_sparse_propagate_cudnn_f32; needs `comp`; Wg / bg / Wc / bc / gru_packed / activation are not read)."""
    if fuse_gather is None:
        fuse_gather = FUSE_GATHER
    lib = _lib.load()
    _req(h0, torch.float32, "h0")
    V, D = h0.shape
    T, L = index.num_edge_types, len(layer_timesteps)
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    rows = comp.num_rows if comp is not None else -1
    ws_bytes = lib.ggnn_sparse_propagate_workspace_bytes(V, D, T, rows)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=h0.device)
    outs = [torch.empty_like(h0) for _ in range(L)]
    res_ptr = [0]
    res_idx = []
    for r in residuals:
        res_idx.extend(int(i) for i in r)
        res_ptr.append(len(res_idx))
    i32 = lambda xs: (ctypes.c_int32 * max(len(xs), 1))(*xs)
    off = None if comp is None else (ctypes.c_int64 * (T + 1))(*comp.type_row_off)
    gather = index.gather_row if comp is None else comp.gather_row
    if cudnn is not None:
        if comp is None or attn is not None or rnn is not None or len(cudnn) != 7 or any(len(x) != L for x in cudnn[:6]):
            raise ValueError("the Cudnn cell's one-call form needs the compacted transform, no attention, and six weight lists of one "
                             "entry per layer plus the packed images")
        ws_bytes = lib.ggnn_sparse_propagate_cudnn_workspace_bytes(V, D, T, rows)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=h0.device)
        _launch("sparse_propagate_cudnn", lambda: lib.ggnn_sparse_propagate_cudnn_f32(
            _ptr(h0), V, D, T, _ptr(index.row_ptr), _ptr(gather), _ptr(comp.pair_node), off,
            _ptr(nin), 1 if use_avg else 0, L, i32([int(x) for x in layer_timesteps]), i32(res_ptr), i32(res_idx),
            _ptr_array(edge_w), _ptr_array(edge_packed), _ptr_array(edge_bias), *[_ptr_array(x) for x in cudnn],
            None if edge_fmt is None else i32([int(f) for f in edge_fmt]), _ptr_array(outs), _ptr(ws), ws_bytes, _stream()))
        return outs
    if rnn is not None:
        rnn_w, rnn_b, rnn_packed = rnn
        if comp is None or attn is not None or len(rnn_w) != L or len(rnn_b) != L:
            raise ValueError("the RNN cell's one-call form needs the compacted transform, no attention, and one (W, b) per layer")
        _launch("sparse_propagate_rnn", lambda: lib.ggnn_sparse_propagate_rnn_f32(
            _ptr(h0), V, D, T, _ptr(index.row_ptr), _ptr(gather), gather.numel(), _ptr(comp.pair_node), off,
            _ptr(nin), 1 if use_avg else 0, L, i32([int(x) for x in layer_timesteps]), i32(res_ptr), i32(res_idx),
            _ptr_array(edge_w), _ptr_array(edge_packed), _ptr_array(edge_bias), _ptr_array(rnn_w), _ptr_array(rnn_b),
            _ptr_array(rnn_packed), None if edge_fmt is None else i32([int(f) for f in edge_fmt]), act, int(fuse_gather),
            _ptr_array(outs), _ptr(ws), ws_bytes, _stream()))
        return outs
    if attn is not None:
        if comp is None or len(attn) != L:
            raise ValueError("propagation attention needs the compacted transform and one [T] factor tensor per layer")
        for l, f in enumerate(attn):
            _req(f, torch.float32, "attn[%d]" % l)
            if f.shape != (T,):
                raise ValueError("attn[%d] must be [T]" % l)
        _launch("sparse_propagate_attn", lambda: lib.ggnn_sparse_propagate_attn_f32(
            _ptr(h0), V, D, T, _ptr(index.row_ptr), _ptr(gather), _ptr(comp.pair_node), off,
            _ptr(nin), 1 if use_avg else 0, L, i32([int(x) for x in layer_timesteps]), i32(res_ptr), i32(res_idx),
            _ptr_array(edge_w), _ptr_array(edge_packed), _ptr_array(edge_bias), _ptr_array(Wg), _ptr_array(bg), _ptr_array(Wc),
            _ptr_array(bc), _ptr_array(gru_packed), None if gru_fmt is None else i32([int(f) for f in gru_fmt]),
            None if edge_fmt is None else i32([int(f) for f in edge_fmt]), act, 0,
            _ptr_array(outs), _ptr(ws), ws_bytes, _ptr(index.gather_row), _ptr_array(attn), _stream()))
        return outs
    _launch("sparse_propagate", lambda: lib.ggnn_sparse_propagate_f32(
        _ptr(h0), V, D, T, _ptr(index.row_ptr), _ptr(gather), None if comp is None else _ptr(comp.pair_node), off,
        _ptr(nin), 1 if use_avg else 0, L, i32([int(x) for x in layer_timesteps]), i32(res_ptr), i32(res_idx),
        _ptr_array(edge_w), _ptr_array(edge_packed), _ptr_array(edge_bias), _ptr_array(Wg), _ptr_array(bg), _ptr_array(Wc),
        _ptr_array(bc), _ptr_array(gru_packed), None if gru_fmt is None else i32([int(f) for f in gru_fmt]),
        None if edge_fmt is None else i32([int(f) for f in edge_fmt]), act, int(fuse_gather),
        _ptr_array(outs), _ptr(ws), ws_bytes, _stream()))
    return outs


def gru_packed_gather(residual_segs: Sequence[torch.Tensor], h: torch.Tensor, packed: torch.Tensor, bg: torch.Tensor,
                      bc: torch.Tensor, H: torch.Tensor, index: MessageIndex, gather_row: Optional[torch.Tensor],
                      num_incoming_edges_per_type: Optional[torch.Tensor], activation: str = "tanh",
                      tile_counter: Optional[torch.Tensor] = None, save: Optional[dict] = None,
                      fmt: int = GRU_FMT_EXACT) -> torch.Tensor:
    """chem_tensorflow_sparse.py:198-216 in one launch (ggnn_gru_packed_gather_f32): the GRU whose last input
    segment -- the aggregated messages -- is summed from the transformed rows `H` inside the kernel.
    save (dict): filled with r, u, c and the gathered segment "incoming" (training: what the backward pass needs)."""
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(H, torch.float32, "H")
    V, D = h.shape
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    segs = (ctypes.c_void_p * max(len(residual_segs), 1))(*[s.data_ptr() for s in residual_segs])
    out = torch.empty_like(h)
    nin = num_incoming_edges_per_type
    gather = index.gather_row if gather_row is None else gather_row
    if save is not None:
        for k in ("r", "u", "c", "incoming"):
            save[k] = torch.empty_like(h)
        _launch("gru_fused_gather_train[nx=%d]" % (len(residual_segs) + 1), lambda: lib.ggnn_gru_packed_gather_train_f32(
            segs, len(residual_segs) + 1, _ptr(h), _ptr(packed), _ptr(bg), _ptr(bc), _ptr(out), _ptr(H), _ptr(index.row_ptr),
            _ptr(gather), None if nin is None else _ptr(nin), index.num_edge_types, 0 if nin is None else 1, _ptr(save["r"]),
            _ptr(save["u"]), _ptr(save["c"]), _ptr(save["incoming"]), V, D, act, int(fmt), _ptr(tile_counter), _stream()))
        return out
    _launch("gru_fused_gather[nx=%d]" % (len(residual_segs) + 1), lambda: lib.ggnn_gru_packed_gather_f32(
        segs, len(residual_segs) + 1, _ptr(h), _ptr(packed), _ptr(bg), _ptr(bc), _ptr(out), _ptr(H), _ptr(index.row_ptr),
        _ptr(gather), None if nin is None else _ptr(nin), index.num_edge_types, 0 if nin is None else 1, V, D, act, int(fmt),
        _ptr(tile_counter), _stream()))
    return out


def cudnn_gru_fused_supported(D: int, nx: int) -> bool:
    """True when the CudnnCompatibleGRUCell with nx concatenated inputs (residuals + messages) has the single fused launch at width D
    (ggnn_cudnn_gru_fused_supported: D = 32 / 64 / 100 with nx <= 3)."""
    return bool(_lib.load().ggnn_cudnn_gru_fused_supported(int(D), int(nx)))


def cudnn_gru_fused_launch_geometry(D: int, nx: int) -> Tuple[int, int]:
    """(rows a workgroup of the fused CudnnCompatibleGRUCell covers per pass, the most workgroups a launch starts)."""
    rows, wgs = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().ggnn_cudnn_gru_fused_launch_geometry(int(D), int(nx), ctypes.byref(rows), ctypes.byref(wgs))
    return rows.value, wgs.value


def cudnn_gru_pack(Wg: torch.Tensor, Wcx: torch.Tensor, Wch: torch.Tensor, nx: int) -> torch.Tensor:
    """Wg [(nx+1) D, 2D], Wcx [nx D, D], Wch [D, D] -> the 3 (nx + 1) stage images of ggnn_cudnn_gru_packed_f32, in the pass's stage
    order (PackedWeights.cudnn caches them per weight version)."""
    lib = _lib.load()
    _req(Wg, torch.float32, "Wg"); _req(Wcx, torch.float32, "Wcx"); _req(Wch, torch.float32, "Wch")
    if Wch.dim() != 2 or Wch.shape[0] != Wch.shape[1]:
        raise ValueError("Wch must be [D, D]")
    D = Wch.shape[1]
    if tuple(Wg.shape) != ((nx + 1) * D, 2 * D) or tuple(Wcx.shape) != (nx * D, D):
        raise ValueError("Wg must be [(nx+1)*D, 2*D] and Wcx [nx*D, D]")
    packed = torch.empty(max(lib.ggnn_cudnn_gru_packed_bytes(D, nx) // 4, 4), dtype=torch.float32, device=Wg.device)
    check(lib.ggnn_cudnn_gru_pack_weights_f32(_ptr(Wg), _ptr(Wcx), _ptr(Wch), nx, D, _ptr(packed), _stream()))
    return packed


def cudnn_gru_packed(x_segs: Sequence[torch.Tensor], h: torch.Tensor, packed: torch.Tensor, bg: torch.Tensor, bcx: torch.Tensor,
                     bch: torch.Tensor, save: Optional[dict] = None) -> torch.Tensor:
    """chem_tensorflow_sparse.py:105-108 in one launch (ggnn_cudnn_gru_packed_f32) on cudnn_gru_pack's images; x_segs: the residual
    states first, the aggregated messages last.  save (dict): filled with r, u, c, hc [V, D] (training: what the backward reads);
    h' is bit-identical with and without it."""
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(packed, torch.float32, "packed")
    _req(bg, torch.float32, "bg"); _req(bcx, torch.float32, "bcx"); _req(bch, torch.float32, "bch")
    V, D = h.shape
    for i, x in enumerate(x_segs):
        _req(x, torch.float32, "x_segs[%d]" % i)
        if x.shape != (V, D):
            raise ValueError("x_segs[%d] must be [V,D]" % i)
    nx = len(x_segs)
    if bg.numel() != 2 * D or bcx.numel() != D or bch.numel() != D:
        raise ValueError("bg must be [2D], bcx and bch [D]")
    if packed.numel() * 4 < lib.ggnn_cudnn_gru_packed_bytes(D, nx):
        raise ValueError("packed holds fewer than the 3 (nx + 1) images of cudnn_gru_pack")
    segs = (ctypes.c_void_p * max(nx, 1))(*[s.data_ptr() for s in x_segs])
    out = torch.empty_like(h)
    keep = [None] * 4
    if save is not None:
        keep = [torch.empty_like(h) for _ in range(4)]
        save["r"], save["u"], save["c"], save["hc"] = keep
    _launch("cudnn_gru_packed[nx=%d]" % nx, lambda: lib.ggnn_cudnn_gru_packed_f32(
        segs, nx, _ptr(h), _ptr(packed), _ptr(bg), _ptr(bcx), _ptr(bch), _ptr(out), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
        _ptr(keep[3]), V, D, _stream()))
    return out


def rnn_fused_supported(D: int, nx: int) -> bool:
    """True when the BasicRNNCell with nx concatenated inputs (residuals + messages) has the gather-fused single launch at width D
    (ggnn_rnn_fused_supported: all nx + 1 weight images resident in LDS -- D = 32 / 64 with nx <= 3, D = 100 with nx = 1)."""
    return bool(_lib.load().ggnn_rnn_fused_supported(int(D), int(nx)))


def rnn_fused_launch_geometry(D: int, nx: int) -> Tuple[int, int]:
    """(rows a workgroup of the gather-fused RNN cell covers per round of its tile loop, the most workgroups a launch starts)."""
    rows, wgs = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().ggnn_rnn_fused_launch_geometry(int(D), int(nx), ctypes.byref(rows), ctypes.byref(wgs))
    return rows.value, wgs.value


def rnn_pack(W: torch.Tensor, nx: int) -> torch.Tensor:
    """W [(nx+1) D, D] -> the nx + 1 stage images of ggnn_rnn_packed_gather_f32 (PackedWeights.rnn caches them per weight version)."""
    lib = _lib.load()
    _req(W, torch.float32, "W")
    if W.dim() != 2 or W.shape[0] != (nx + 1) * W.shape[1]:
        raise ValueError("W must be [(nx+1)*D, D]")
    D = W.shape[1]
    packed = torch.empty(max(lib.ggnn_rnn_packed_bytes(D, nx) // 4, 4), dtype=torch.float32, device=W.device)
    check(lib.ggnn_rnn_pack_weights_f32(_ptr(W), nx, D, _ptr(packed), _stream()))
    return packed


def rnn_packed_gather(residual_segs: Sequence[torch.Tensor], h: torch.Tensor, packed: torch.Tensor, b: torch.Tensor,
                      Hc: torch.Tensor, index: MessageIndex, gather_row: Optional[torch.Tensor],
                      num_incoming_edges_per_type: Optional[torch.Tensor], activation: str = "tanh",
                      save: Optional[dict] = None) -> torch.Tensor:
    """chem_tensorflow_sparse.py:198-216 for the BasicRNNCell in one launch (ggnn_rnn_packed_gather_f32): the cell whose last
    input segment -- the aggregated messages -- is summed from the transformed rows `Hc` inside the kernel (no edge bias; the
    mean with num_incoming_edges_per_type, the plain sum with None).  gather_row: message slot -> row of Hc (None: the index's
    own).  save (dict): receives the gathered segment as save["incoming"] (training: an operand of the weight gradient)."""
    return _rnn_gather_launch("ggnn_rnn_packed_gather_f32", "rnn_fused_gather[nx=%d]", residual_segs, h, packed, b, Hc, index,
                              gather_row, num_incoming_edges_per_type, activation, save)


def rnn_panel_supported(D: int, nx: int) -> bool:
    """True when the BasicRNNCell with nx concatenated inputs has the gather-fused COLUMN-PANEL launch at width D
    (ggnn_rnn_panel_supported: D = 128 / 192 / 256 with nx <= 3; disjoint from rnn_fused_supported)."""
    return bool(_lib.load().ggnn_rnn_panel_supported(int(D), int(nx)))


def rnn_panel_launch_geometry(D: int, nx: int) -> Tuple[int, int]:
    """(rows a workgroup of the panel RNN cell covers per pass, the most workgroups a launch starts)."""
    rows, wgs = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().ggnn_rnn_panel_launch_geometry(int(D), int(nx), ctypes.byref(rows), ctypes.byref(wgs))
    return rows.value, wgs.value


def rnn_panel_pack(W: torch.Tensor, nx: int) -> torch.Tensor:
    """W [(nx+1) D, D] -> the (nx + 1) D / 64 panel images of ggnn_rnn_panel_gather_f32 (PackedWeights.rnn_panel caches them per
    weight version)."""
    lib = _lib.load()
    _req(W, torch.float32, "W")
    if W.dim() != 2 or W.shape[0] != (nx + 1) * W.shape[1]:
        raise ValueError("W must be [(nx+1)*D, D]")
    D = W.shape[1]
    packed = torch.empty(max(lib.ggnn_rnn_panel_packed_bytes(D, nx) // 4, 4), dtype=torch.float32, device=W.device)
    check(lib.ggnn_rnn_panel_pack_weights_f32(_ptr(W), nx, D, _ptr(packed), _stream()))
    return packed


def rnn_panel_gather(residual_segs: Sequence[torch.Tensor], h: torch.Tensor, packed: torch.Tensor, b: torch.Tensor,
                     Hc: torch.Tensor, index: MessageIndex, gather_row: Optional[torch.Tensor],
                     num_incoming_edges_per_type: Optional[torch.Tensor], activation: str = "tanh",
                     save: Optional[dict] = None) -> torch.Tensor:
    """rnn_packed_gather at hidden 128 / 192 / 256 (ggnn_rnn_panel_gather_f32; packed: rnn_panel_pack's images): the same
    arguments, the same gather arithmetic and the same save= behaviour."""
    return _rnn_gather_launch("ggnn_rnn_panel_gather_f32", "rnn_panel_gather[nx=%d]", residual_segs, h, packed, b, Hc, index,
                              gather_row, num_incoming_edges_per_type, activation, save)


def _rnn_gather_launch(symbol: str, launch_name: str, residual_segs, h, packed, b, Hc, index, gather_row,
                       num_incoming_edges_per_type, activation, save) -> torch.Tensor:
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(Hc, torch.float32, "Hc"); _req(b, torch.float32, "b")
    V, D = h.shape
    if Hc.dim() != 2 or Hc.shape[1] != D:
        raise ValueError("Hc must be [R, D]")
    for i, x in enumerate(residual_segs):
        _req(x, torch.float32, "residual_segs[%d]" % i)
        if x.shape != (V, D):
            raise ValueError("residual_segs[%d] must be [V,D]" % i)
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    nx = len(residual_segs) + 1
    segs = (ctypes.c_void_p * max(nx - 1, 1))(*[s.data_ptr() for s in residual_segs])
    out = torch.empty_like(h)
    nin = num_incoming_edges_per_type
    if nin is not None:
        _req(nin, torch.float32, "num_incoming_edges_per_type")
    gather = index.gather_row if gather_row is None else gather_row
    inc = None
    if save is not None:
        inc = save["incoming"] = torch.empty_like(h)
    _launch(launch_name % nx, lambda: getattr(lib, symbol)(
        segs, nx, _ptr(h), _ptr(packed), _ptr(b), _ptr(out), _ptr(Hc), Hc.shape[0], _ptr(index.row_ptr), _ptr(gather),
        gather.numel(), None if nin is None else _ptr(nin), index.num_edge_types, 0 if nin is None else 1, _ptr(inc), V, D, act,
        _stream()))
    return out


def rnn_bwd_fused_supported(D: int, nx: int) -> bool:
    """True when the BasicRNNCell backward with nx concatenated inputs has the single fused launch at width D
    (ggnn_rnn_bwd_fused_supported: the forward's set, rnn_fused_supported)."""
    return bool(_lib.load().ggnn_rnn_bwd_fused_supported(int(D), int(nx)))


def rnn_bwd_pack(W: torch.Tensor, nx: int) -> torch.Tensor:
    """W [(nx+1) D, D] -> the nx + 1 images of W_s^T of ggnn_rnn_bwd_fused_f32 (PackedWeights.rnn_bwd caches them per weight version)."""
    lib = _lib.load()
    _req(W, torch.float32, "W")
    if W.dim() != 2 or W.shape[0] != (nx + 1) * W.shape[1]:
        raise ValueError("W must be [(nx+1)*D, D]")
    D = W.shape[1]
    packed = torch.empty(max(lib.ggnn_rnn_bwd_packed_bytes(D, nx) // 4, 4), dtype=torch.float32, device=W.device)
    check(lib.ggnn_rnn_bwd_pack_weights_f32(_ptr(W), nx, D, _ptr(packed), _stream()))
    return packed


def rnn_bwd_fused(g: torch.Tensor, out: torch.Tensor, packed: torch.Tensor, nin: Optional[torch.Tensor], use_avg: bool, nx: int,
                  activation: str, gather=None):
    """The BasicRNNCell backward of one timestep in one launch (ggnn_rnn_bwd_fused_f32) -> (dP, dh, [dx_0 .. dx_{nx-1}]); the last
    dx is d_incoming (already divided by the in-degree for mean aggregation).  gather = (rows, heads): the incoming gradient is
    g[v] + the sum of the rows of `rows` named by the slot-head record heads[v] (ggnn_rnn_bwd_fused_gather_f32)."""
    lib = _lib.load()
    _req(g, torch.float32, "g"); _req(out, torch.float32, "out"); _req(packed, torch.float32, "packed")
    V, D = out.shape
    T = nin.shape[1] if nin is not None else 1
    act = ACT_IDS[activation.lower()]
    dP = torch.empty_like(out); dh = torch.empty_like(out)
    dx = [torch.empty_like(out) for _ in range(nx)]
    dxp = (ctypes.c_void_p * max(nx, 1))(*[t.data_ptr() for t in dx])
    if gather is not None:
        rows, heads = gather
        _req(rows, torch.float32, "rows"); _req(heads, torch.int32, "heads")
        _launch("rnn_bwd_fused_gather[nx=%d]" % nx, lambda: lib.ggnn_rnn_bwd_fused_gather_f32(
            _ptr(g), _ptr(rows), _ptr(heads), rows.shape[0], _ptr(out), _ptr(packed), _ptr(dP), dxp, _ptr(dh), _ptr(nin), T,
            1 if use_avg else 0, nx, V, D, act, _stream()))
    else:
        _launch("rnn_bwd_fused[nx=%d]" % nx, lambda: lib.ggnn_rnn_bwd_fused_f32(
            _ptr(g), _ptr(out), _ptr(packed), _ptr(dP), dxp, _ptr(dh), _ptr(nin), T, 1 if use_avg else 0, nx, V, D, act, _stream()))
    return dP, dh, dx


def gated_readout(last_h: torch.Tensor, h0: torch.Tensor, graph_nodes_list: torch.Tensor, num_graphs: int,
                  gate_W: torch.Tensor, gate_b: torch.Tensor, transform_W: torch.Tensor, transform_b: torch.Tensor) -> torch.Tensor:
    """Fused gated_regression (chem_tensorflow_sparse.py:220-231): per-graph sum of sigmoid(gate)*transform."""
    lib = _lib.load()
    _req(last_h, torch.float32, "last_h"); _req(h0, torch.float32, "h0"); _req(graph_nodes_list, torch.int32, "graph_nodes_list")
    V, D = last_h.shape
    for n, w, numel in (("gate_W", gate_W, 2 * D), ("gate_b", gate_b, 1), ("transform_W", transform_W, D), ("transform_b", transform_b, 1)):
        _req(w, torch.float32, n)
        if w.numel() != numel:
            raise ValueError("%s must have %d elements" % (n, numel))
    out = torch.empty(int(num_graphs), dtype=torch.float32, device=last_h.device)
    _launch("gated_readout", lambda: lib.ggnn_gated_readout_f32(_ptr(last_h), _ptr(h0), _ptr(graph_nodes_list), _ptr(gate_W),
                                                                _ptr(gate_b), _ptr(transform_W), _ptr(transform_b), _ptr(out),
                                                                V, D, int(num_graphs), _stream()))
    return out


def readout_loss_fwd(last_h: torch.Tensor, h0: torch.Tensor, graph_nodes_list: torch.Tensor, graph_ptr: Optional[torch.Tensor],
                     node_mask: Optional[torch.Tensor], num_graphs: int, gate_W: torch.Tensor, gate_b: torch.Tensor,
                     transform_W: torch.Tensor, transform_b: torch.Tensor, target: Optional[torch.Tensor],
                     mask: Optional[torch.Tensor]):
    """Fused gated_regression + masked loss sums (chem_tensorflow_sparse.py:220-231, chem_tensorflow.py:158-170), forward:
    -> (out [G], node_gate [V], node_val [V], stats [3] = (sum 0.5 diff^2, sum |diff|, sum mask) or None without target).
    graph_nodes_list must be non-decreasing (batcher output); deterministic."""
    lib = _lib.load()
    _req(last_h, torch.float32, "last_h"); _req(h0, torch.float32, "h0"); _req(graph_nodes_list, torch.int32, "graph_nodes_list")
    V, D = last_h.shape
    G = int(num_graphs)
    dev = last_h.device
    out = torch.empty(G, dtype=torch.float32, device=dev)
    gate = torch.empty(max(V, 1), dtype=torch.float32, device=dev)
    val = torch.empty(max(V, 1), dtype=torch.float32, device=dev)
    stats = torch.empty(3, dtype=torch.float32, device=dev) if target is not None else None
    ws_bytes = lib.ggnn_readout_workspace_bytes(V, D, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    for n, t in (("gate_W", gate_W), ("gate_b", gate_b), ("transform_W", transform_W), ("transform_b", transform_b)):
        _req(t, torch.float32, n)
    _launch("readout_loss_fwd", lambda: lib.ggnn_readout_loss_fwd_f32(
        _ptr(last_h), _ptr(h0), _ptr(graph_nodes_list), _ptr(graph_ptr), _ptr(node_mask), _ptr(gate_W), _ptr(gate_b), _ptr(transform_W),
        _ptr(transform_b), _ptr(target), _ptr(mask), _ptr(out), _ptr(gate), _ptr(val), _ptr(stats), _ptr(ws), ws_bytes, V, D, G, _stream()))
    return out, gate, val, stats


def readout_loss_bwd(last_h, h0, graph_nodes_list, node_mask, num_graphs, gate_W, transform_W, gate, val, out, target, mask,
                     d_out: Optional[torch.Tensor], d_stats: Optional[torch.Tensor], d_last_h: Optional[torch.Tensor] = None,
                     grad_out: Optional[Sequence[torch.Tensor]] = None):
    """Backward of readout_loss_fwd: -> (d_last_h [V,D], d_gate_W [2D], d_gate_b [1], d_transform_W [D], d_transform_b [1]).
    d_last_h given: the gradient is ADDED to it (further tasks of a multi-task model).
    grad_out: four contiguous float32 buffers (2D, 1, D, 1 elements) that receive the weight gradients (the optimizer's flat
    gradient views) instead of fresh tensors."""
    lib = _lib.load()
    V, D = last_h.shape
    G = int(num_graphs)
    dev = last_h.device
    accumulate = d_last_h is not None
    if d_last_h is None:
        d_last_h = torch.empty_like(last_h) if V and G else torch.zeros_like(last_h)
    if grad_out is not None:
        dgW, dgb, dtW, dtb = grad_out
        for t, n in ((dgW, 2 * D), (dgb, 1), (dtW, D), (dtb, 1)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise TypeError("grad_out buffers must be contiguous float32 CUDA/HIP tensors of 2D, 1, D and 1 elements")
    else:
        dgW = torch.empty(2 * D, dtype=torch.float32, device=dev); dgb = torch.empty(1, dtype=torch.float32, device=dev)
        dtW = torch.empty(D, dtype=torch.float32, device=dev); dtb = torch.empty(1, dtype=torch.float32, device=dev)
    ws_bytes = lib.ggnn_readout_workspace_bytes(V, D, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _launch("readout_loss_bwd", lambda: lib.ggnn_readout_loss_bwd_f32(
        _ptr(last_h), _ptr(h0), _ptr(graph_nodes_list), _ptr(node_mask), _ptr(gate_W), _ptr(transform_W), _ptr(gate), _ptr(val), _ptr(out),
        _ptr(target), _ptr(mask), _ptr(d_out), _ptr(d_stats), _ptr(d_last_h), 1 if accumulate else 0, _ptr(dgW), _ptr(dgb), _ptr(dtW),
        _ptr(dtb), _ptr(ws), ws_bytes, V, D, G, _stream()))
    return d_last_h, dgW, dgb, dtW, dtb


# ---- multi-task readout: every entry of task_ids in one pass over the node states (ggnn_readout_multi_*) ------------
def readout_multi_supported(D: int, K: int) -> bool:
    """True when ggnn_readout_multi_{fwd,bwd}_f32 take kernel width D with K tasks (multiples of 4 up to 256, 1 <= K <= 16)."""
    return bool(_lib.load().ggnn_readout_multi_supported(int(D), int(K)))


def _task_ptrs(tensors: Sequence[torch.Tensor], numel: int, name: str):
    for t in tensors:
        _req(t, torch.float32, name)
        if t.numel() != numel:
            raise ValueError("%s: every task's tensor must have %d elements" % (name, numel))
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def readout_multi_fwd(last_h: torch.Tensor, h0: torch.Tensor, graph_nodes_list: torch.Tensor, graph_ptr: Optional[torch.Tensor],
                      node_mask: Optional[torch.Tensor], num_graphs: int, gate_Ws: Sequence[torch.Tensor],
                      gate_bs: Sequence[torch.Tensor], transform_Ws: Sequence[torch.Tensor], transform_bs: Sequence[torch.Tensor],
                      targets: Optional[torch.Tensor], masks: Optional[torch.Tensor]):
    """readout_loss_fwd for K tasks in one pass: gate_Ws[k] [2D], gate_bs[k] [1], transform_Ws[k] [D], transform_bs[k] [1] (separate
    tensors per task), targets / masks [K,G] -> (out [K,G], node_gv [V,2K] = per node (gate of every task | value of every task),
    stats [K,3] = per task (sum 0.5 diff^2, sum |diff|, sum mask), or None without targets).  Deterministic; graph_nodes_list sorted."""
    lib = _lib.load()
    _req(last_h, torch.float32, "last_h"); _req(h0, torch.float32, "h0"); _req(graph_nodes_list, torch.int32, "graph_nodes_list")
    V, D = last_h.shape
    G, K = int(num_graphs), len(gate_Ws)
    if not (K == len(gate_bs) == len(transform_Ws) == len(transform_bs)) or K < 1:
        raise ValueError("one gate_W, gate_b, transform_W and transform_b per task")
    if h0.shape != last_h.shape:
        raise ValueError("h0 must have the shape of last_h")
    dev = last_h.device
    for n, t in (("targets", targets), ("masks", masks)):
        if t is not None:
            _req(t, torch.float32, n)
            if tuple(t.shape) != (K, G):
                raise ValueError("%s must be [K, G] = [%d, %d]" % (n, K, G))
    gW, gb = _task_ptrs(gate_Ws, 2 * D, "gate_W"), _task_ptrs(gate_bs, 1, "gate_b")
    tW, tb = _task_ptrs(transform_Ws, D, "transform_W"), _task_ptrs(transform_bs, 1, "transform_b")
    out = torch.empty(K, G, dtype=torch.float32, device=dev)
    node_gv = torch.empty(max(V, 1), 2 * K, dtype=torch.float32, device=dev)
    stats = torch.empty(K, 3, dtype=torch.float32, device=dev) if targets is not None else None
    ws_bytes = lib.ggnn_readout_multi_workspace_bytes(V, D, K, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _launch("readout_multi_fwd[K=%d]" % K, lambda: lib.ggnn_readout_multi_fwd_f32(
        _ptr(last_h), _ptr(h0), _ptr(graph_nodes_list), _ptr(graph_ptr), _ptr(node_mask), gW, gb, tW, tb, _ptr(targets), _ptr(masks),
        _ptr(out), _ptr(node_gv), _ptr(stats), _ptr(ws), ws_bytes, V, D, K, G, _stream()))
    return out, node_gv, stats


def readout_multi_bwd(last_h, h0, graph_nodes_list, node_mask, num_graphs, gate_Ws, transform_Ws, node_gv, out, targets, masks,
                      d_out: Optional[torch.Tensor], d_stats: Optional[torch.Tensor], d_last_h: Optional[torch.Tensor] = None,
                      grad_out: Optional[Sequence[Sequence[torch.Tensor]]] = None):
    """Backward of readout_multi_fwd: d_out [K,G] or None, d_stats [K,2] or None -> (d_last_h [V,D], d_gate_W [K,2D], d_gate_b [K],
    d_transform_W [K,D], d_transform_b [K]).  d_last_h given: the gradient is ADDED to it.
    grad_out: four sequences of K contiguous float32 buffers (2D, 1, D, 1 elements: the optimizer's flat gradient views) that
    receive the weight gradients instead; they are returned in place of the stacked tensors."""
    lib = _lib.load()
    V, D = last_h.shape
    G, K = int(num_graphs), len(gate_Ws)
    dev = last_h.device
    accumulate = d_last_h is not None
    if d_last_h is None:
        d_last_h = torch.empty_like(last_h) if V and G else torch.zeros_like(last_h)
    for n, t, shape in (("d_out", d_out, (K, G)), ("d_stats", d_stats, (K, 2))):
        if t is not None:
            _req(t, torch.float32, n)
            if tuple(t.shape) != shape:
                raise ValueError("%s must have shape %r" % (n, shape))
    if grad_out is not None:
        res = tuple(list(g) for g in grad_out)
        if len(res) != 4 or any(len(g) != K for g in res):
            raise ValueError("grad_out: four sequences of K buffers")
        dst = [_task_ptrs(g, n, "grad_out") for g, n in zip(res, (2 * D, 1, D, 1))]
    else:
        res = (torch.empty(K, 2 * D, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.float32, device=dev),
               torch.empty(K, D, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.float32, device=dev))
        dst = [(ctypes.c_void_p * K)(*[t.data_ptr() + k * t.stride(0) * 4 for k in range(K)]) for t in res]
    gW, tW = _task_ptrs(gate_Ws, 2 * D, "gate_W"), _task_ptrs(transform_Ws, D, "transform_W")
    ws_bytes = lib.ggnn_readout_multi_workspace_bytes(V, D, K, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _launch("readout_multi_bwd[K=%d]" % K, lambda: lib.ggnn_readout_multi_bwd_f32(
        _ptr(last_h), _ptr(h0), _ptr(graph_nodes_list), _ptr(node_mask), gW, tW, _ptr(node_gv), _ptr(out), _ptr(targets), _ptr(masks),
        _ptr(d_out), _ptr(d_stats), _ptr(d_last_h), 1 if accumulate else 0, dst[0], dst[1], dst[2], dst[3], _ptr(ws), ws_bytes,
        V, D, K, G, _stream()))
    return (d_last_h,) + tuple(res)


# ---- the remaining switches of the same function: attention, RNN cell, cudnn-compatible GRU cell ------------------
def gather_segment_sum_attn(H: torch.Tensor, h: torch.Tensor, index: MessageIndex, type_factors: torch.Tensor,
                            num_incoming_edges_per_type: Optional[torch.Tensor], edge_biases: Optional[torch.Tensor],
                            use_avg: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """use_propagation_attention (chem_tensorflow_sparse.py:147-149, 170-196) fused into the segment sum.
    H [V, T*D] from msg_transform (dense form), h [V,D] current states, type_factors [T]."""
    lib = _lib.load()
    _req(H, torch.float32, "H"); _req(h, torch.float32, "h"); _req(type_factors, torch.float32, "type_factors")
    V, T = index.num_nodes, index.num_edge_types
    D = h.shape[1]
    if H.shape != (V, T * D) or type_factors.shape != (T,):
        raise ValueError("shape mismatch: H [V,T*D], h [V,D], type_factors [T]")
    nin = num_incoming_edges_per_type
    if out is None:
        out = torch.empty((V, D), dtype=torch.float32, device=h.device)
    _launch("gather_segment_sum_attn", lambda: lib.ggnn_gather_segment_sum_attn_f32(
        _ptr(H), _ptr(h), _ptr(index.row_ptr), _ptr(index.gather_row), _ptr(type_factors), _ptr(nin), _ptr(edge_biases),
        1 if use_avg else 0, _ptr(out), V, D, T, _stream()))
    return out


def gather_segment_sum_attn_compact(Hc: torch.Tensor, h: torch.Tensor, index: MessageIndex, comp: CompactSources,
                                    type_factors: torch.Tensor, num_incoming_edges_per_type: Optional[torch.Tensor],
                                    edge_biases: Optional[torch.Tensor], use_avg: bool,
                                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gather_segment_sum_attn over the compacted transform's rows (ggnn_gather_segment_sum_attn_compact_f32): the message of slot
    e is Hc[comp.gather_row[e]] (Hc [R,D] from msg_transform_compact[_packed]); index.gather_row still names source and type."""
    lib = _lib.load()
    _req(Hc, torch.float32, "Hc"); _req(h, torch.float32, "h"); _req(type_factors, torch.float32, "type_factors")
    V, T = index.num_nodes, index.num_edge_types
    D = h.shape[1]
    if h.shape[0] != V or Hc.dim() != 2 or Hc.shape[1] != D or Hc.shape[0] < comp.num_rows or type_factors.shape != (T,):
        raise ValueError("shape mismatch: Hc [R,D], h [V,D], type_factors [T]")
    nin = num_incoming_edges_per_type
    if nin is not None:
        _req(nin, torch.float32, "num_incoming_edges_per_type")
    if edge_biases is not None:
        _req(edge_biases, torch.float32, "edge_biases")
    if out is None:
        out = torch.empty((V, D), dtype=torch.float32, device=h.device)
    else:
        _req(out, torch.float32, "out")
    _launch("gather_segment_sum_attn_compact", lambda: lib.ggnn_gather_segment_sum_attn_compact_f32(
        _ptr(Hc), _ptr(h), _ptr(index.row_ptr), _ptr(index.gather_row), _ptr(comp.gather_row), _ptr(type_factors), _ptr(nin),
        _ptr(edge_biases), 1 if use_avg else 0, _ptr(out), V, D, T, _stream()))
    return out


def attn_backward_target_compact(Hc: torch.Tensor, h: torch.Tensor, d_att: torch.Tensor, index: MessageIndex, comp: CompactSources,
                                 type_factors: torch.Tensor, dh: torch.Tensor):
    """attn_backward_target over the compacted transform's rows (ggnn_attn_bwd_target_compact_f32): adds the target-side state
    gradient to dh and returns the per-message (coef_a, coef_s, dfac), indexed by message id."""
    lib = _lib.load()
    _req(Hc, torch.float32, "Hc"); _req(h, torch.float32, "h"); _req(d_att, torch.float32, "d_att"); _req(dh, torch.float32, "dh")
    V, D = h.shape
    T, M = index.num_edge_types, index.num_messages
    if Hc.dim() != 2 or Hc.shape[1] != D or Hc.shape[0] < comp.num_rows or d_att.shape != (V, D) or dh.shape != (V, D):
        raise ValueError("shape mismatch: Hc [R,D], h / d_att / dh [V,D]")
    dev = h.device
    ca = torch.empty(max(M, 1), dtype=torch.float32, device=dev); cs = torch.empty_like(ca); df = torch.empty_like(ca)
    _launch("attn_bwd_target_compact", lambda: lib.ggnn_attn_bwd_target_compact_f32(
        _ptr(Hc), _ptr(h), _ptr(d_att), _ptr(index.row_ptr), _ptr(index.gather_row), _ptr(comp.gather_row), _ptr(index.msg_perm),
        _ptr(type_factors), _ptr(ca), _ptr(cs), _ptr(df), _ptr(dh), 1, V, D, T, _stream()))
    return ca, cs, df


def source_slot_rows(index: MessageIndex, comp: CompactSources) -> torch.Tensor:
    """[M] int32: the compact row of every by-(source, type) slot (the slots of CompactBackward.source_node_index), i.e. the row of
    the slot's (source node, type) pair.  Built once per batch (torch index arithmetic, no read-back), kept on the CompactBackward."""
    bwd = compact_backward(index, comp)
    rows = getattr(bwd, "_source_slot_row", None)
    if rows is None:
        ri = bwd.rows_index                                  # segments = compact rows, their slots in by-source order
        R, M = comp.num_rows, index.num_messages
        dev = index.adj.device
        src = index._source_index
        T = index.num_edge_types
        # a pair's by-source slots start at row_ptr[node*T + type]; the pairs of rows_index are in compact-row order
        length = (ri.row_ptr[1:] - ri.row_ptr[:-1]).long()
        typ = torch.repeat_interleave(torch.arange(T, device=dev), torch.as_tensor(
            [comp.type_row_off[t + 1] - comp.type_row_off[t] for t in range(T)], device=dev), output_size=R)
        start = src.row_ptr.long()[comp.pair_node[:R].long() * T + typ]
        slots = torch.repeat_interleave(start - ri.row_ptr[:-1].long(), length, output_size=M) + torch.arange(M, device=dev)
        rows = torch.empty(M, dtype=torch.int32, device=dev)
        rows[slots] = torch.repeat_interleave(torch.arange(R, dtype=torch.int32, device=dev), length, output_size=M)
        bwd._source_slot_row = rows
    return rows


def attn_backward_source_compact(d_att: torch.Tensor, h: torch.Tensor, source_node_index: "SegmentIndex", slot_row: torch.Tensor,
                                 num_rows: int, coef_a: torch.Tensor, coef_s: torch.Tensor, dh: Optional[torch.Tensor],
                                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Source-side pass of the propagation-attention backward over the compacted rows (ggnn_attn_bwd_source_compact_f32), one launch
    for  weighted_segment_sum(d_att, rows_index, .., coef_a)  and  weighted_segment_sum(h, source_node_index, .., coef_s, out=dh,
    accumulate=True)  -- bit for bit.  source_node_index: CompactBackward.source_node_index (segments = nodes, gather_row = target,
    msg = message id); slot_row: source_slot_rows.  Adds the source-side state gradient to dh (None: skipped) and returns
    dHc [num_rows, D]."""
    lib = _lib.load()
    _req(d_att, torch.float32, "d_att"); _req(h, torch.float32, "h")
    _req(coef_a, torch.float32, "coef_a"); _req(coef_s, torch.float32, "coef_s"); _req(slot_row, torch.int32, "slot_row")
    V, D = h.shape
    sni = source_node_index
    _req(sni.row_ptr, torch.int32, "source_node_index.row_ptr"); _req(sni.gather_row, torch.int32, "source_node_index.gather_row")
    if sni.msg is None:
        raise ValueError("source_node_index needs its slot -> message id table")
    _req(sni.msg, torch.int32, "source_node_index.msg")
    M = sni.gather_row.shape[0]
    if d_att.shape != (V, D) or sni.num_nodes != V or sni.row_ptr.shape[0] != V + 1 or slot_row.shape[0] != M or sni.msg.shape[0] != M \
            or coef_a.shape[0] < M or coef_s.shape[0] < M or (dh is not None and dh.shape != (V, D)):
        raise ValueError("shape mismatch: d_att / h / dh [V,D], index over V nodes and M slots, coef_a / coef_s [M]")
    if dh is not None:
        _req(dh, torch.float32, "dh")
    if out is None:
        out = torch.empty((max(int(num_rows), 1), D), dtype=torch.float32, device=h.device)
    else:
        _req(out, torch.float32, "out")
    if out.dim() != 2 or out.shape[1] != D or out.shape[0] < num_rows:
        raise ValueError("out must be [num_rows, D]")
    _launch("attn_bwd_source_compact", lambda: lib.ggnn_attn_bwd_source_compact_f32(
        _ptr(d_att), _ptr(h), _ptr(sni.row_ptr), _ptr(sni.gather_row), _ptr(sni.msg), _ptr(slot_row), _ptr(coef_a), _ptr(coef_s),
        _ptr(out), _ptr(dh), V, D, _stream()))
    return out


def rnn(x_segs: Sequence[torch.Tensor], h: torch.Tensor, W: torch.Tensor, b: torch.Tensor, activation: str = "tanh") -> torch.Tensor:
    """tf.nn.rnn_cell.BasicRNNCell (chem_tensorflow_sparse.py:109-110): act([x|h] W + b)."""
    lib = _lib.load()
    _req(h, torch.float32, "h"); _req(W, torch.float32, "W"); _req(b, torch.float32, "b")
    V, D = h.shape
    nx = len(x_segs)
    if tuple(W.shape) != ((nx + 1) * D, D) or tuple(b.shape) != (D,):
        raise ValueError("W must be [(nx+1)D, D] and b [D]")
    out = torch.empty_like(h)
    segs = (ctypes.c_void_p * nx)(*[_req(x, torch.float32, "x").data_ptr() for x in x_segs])
    act = ACT_IDS.get(activation.lower())
    if act is None:
        raise Exception("Unknown activation function type '%s'." % activation)
    _launch("rnn[nx=%d]" % nx, lambda: lib.ggnn_rnn_f32(segs, nx, _ptr(h), _ptr(W), _ptr(b), _ptr(out), V, D, act, _stream()))
    return out


def cudnn_gru(x_segs: Sequence[torch.Tensor], h: torch.Tensor, Wg, bg, Wcx, bcx, Wch, bch) -> torch.Tensor:
    """tf.contrib.cudnn_rnn.CudnnCompatibleGRUCell (chem_tensorflow_sparse.py:105-108)."""
    lib = _lib.load()
    V, D = h.shape
    nx = len(x_segs)
    for n, w, shp in (("Wg", Wg, ((nx + 1) * D, 2 * D)), ("bg", bg, (2 * D,)), ("Wcx", Wcx, (nx * D, D)), ("bcx", bcx, (D,)),
                      ("Wch", Wch, (D, D)), ("bch", bch, (D,))):
        _req(w, torch.float32, n)
        if tuple(w.shape) != shp:
            raise ValueError("%s must have shape %s, got %s" % (n, shp, tuple(w.shape)))
    out = torch.empty_like(h)
    ws_bytes = lib.ggnn_cudnn_gru_workspace_bytes(V, D)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=h.device)
    segs = (ctypes.c_void_p * nx)(*[_req(x, torch.float32, "x").data_ptr() for x in x_segs])
    _launch("cudnn_gru[nx=%d]" % nx, lambda: lib.ggnn_cudnn_gru_f32(segs, nx, _ptr(h), _ptr(Wg), _ptr(bg), _ptr(Wcx), _ptr(bcx),
                                                                    _ptr(Wch), _ptr(bch), _ptr(out), _ptr(ws), ws_bytes, V, D, _stream()))
    return out


# ---- sparse GCN (chem_tensorflow_gcn.py:62-82; csrc/ggnn_gcn.hip) -----------------------------------------------------------------
class GCNGraph:
    """A_hat of one batch as CSR (row_ptr, col, val) and its transpose (row_ptr_t, col_t, val_t), device tensors.  The backward pass
    multiplies by A_hat^T, which need not equal A_hat for a user feed.  slot_ids / slot_ids_t (0 .. nnz-1) are the per-slot weight ids
    of the composed path's ggnn_weighted_segment_sum_f32."""

    def __init__(self, row_ptr, col, val, row_ptr_t, col_t, val_t, num_nodes: int):
        self.row_ptr, self.col, self.val = row_ptr, col, val
        self.row_ptr_t, self.col_t, self.val_t = row_ptr_t, col_t, val_t
        self.num_nodes = int(num_nodes)
        self.nnz = int(col.numel())
        self._slots = None

    def slot_ids(self) -> torch.Tensor:
        if self._slots is None:
            self._slots = torch.arange(self.nnz, dtype=torch.int32, device=self.col.device)
        return self._slots


def gcn_csr_host(adjacency_list, adjacency_weights, num_nodes: int):
    """NumPy CSR of the sparse matrix with entries (adjacency_list[k] = (i, j), adjacency_weights[k]) and of its transpose:
    -> (row_ptr, col, val, row_ptr_t, col_t, val_t).  Entries keep their feed order inside a row (a stable sort by row; the packer's
    lists are row-major sorted already), so every row is summed in the order tf.sparse_tensor_dense_matmul sees its nonzeros.
    Indices outside [0, num_nodes) raise."""
    import numpy as np
    adj = np.asarray(adjacency_list, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(adjacency_weights, dtype=np.float32).reshape(-1)
    if adj.shape[0] != w.shape[0]:
        raise ValueError("adjacency_list and adjacency_weights differ in length")
    V = int(num_nodes)
    if adj.size and (adj.min() < 0 or adj.max() >= V):
        raise IndexError("adjacency_list holds a node index outside [0, %d)" % V)
    if adj.shape[0] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 nonzeros")

    def csr(rows, cols, vals):
        order = np.argsort(rows, kind="stable")
        ptr = np.zeros(V + 1, np.int32)
        np.cumsum(np.bincount(rows, minlength=V), out=ptr[1:])
        return ptr, cols[order].astype(np.int32), vals[order]

    rp, c, v = csr(adj[:, 0], adj[:, 1], w)
    # transpose of the row-sorted matrix: stable by column, i.e. row-ascending inside each transposed row
    rows_sorted = np.repeat(np.arange(V, dtype=np.int64), np.diff(rp))
    rpt, ct, vt = csr(c.astype(np.int64), rows_sorted, v)
    return rp, c, v, rpt, ct, vt


def gcn_graph(adjacency_list, adjacency_weights, num_nodes: int, device) -> GCNGraph:
    """GCNGraph of a fed (adjacency_list [nnz, 2], adjacency_weights [nnz]) pair (NumPy or tensors), uploaded to `device`."""
    if isinstance(adjacency_list, torch.Tensor):
        adjacency_list = adjacency_list.cpu().numpy()
    if isinstance(adjacency_weights, torch.Tensor):
        adjacency_weights = adjacency_weights.cpu().numpy()
    parts = gcn_csr_host(adjacency_list, adjacency_weights, num_nodes)
    return GCNGraph(*[torch.from_numpy(p).to(device) for p in parts], num_nodes)


def gcn_epoch_table(counts_t: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """Prefix sums of per-graph counts over an epoch's order, on the device (ggnn_pack_batch_tables, one launch per epoch).
    counts_t int32 [2, Gd] (nodes, A_hat entries per graph), order int64 [Ge] -> int32 [Ge | Ge+1 | Ge+1]: the order as int32, then
    node_cum and entry_cum, the totals of the graphs before each epoch position."""
    lib = _lib.load()
    _req(counts_t, torch.int32, "counts_t")
    _req(order, torch.int64, "order")
    if counts_t.dim() != 2 or counts_t.shape[0] != 2 or order.dim() != 1 or order.device != counts_t.device:
        raise ValueError("counts_t must be [2, Gd] and order [Ge] on its device")
    Ge = order.numel()
    tab = torch.empty(3 * Ge + 2, dtype=torch.int32, device=order.device)
    _launch("gcn_epoch_table", lambda: lib.ggnn_pack_batch_tables(_ptr(counts_t), counts_t.shape[1], 2, _ptr(order) if Ge else None, Ge,
                                                                  None, None, 0, None, 0, _ptr(tab), None, None, _stream()))
    return tab


def gcn_assemble_batch(node_ptr: torch.Tensor, feat: torch.Tensor, csr: Sequence[torch.Tensor], csr_t: Sequence[torch.Tensor],
                       targets: torch.Tensor, label_mask: Optional[torch.Tensor], task_ids: torch.Tensor, epoch_tab: torch.Tensor,
                       start: int, num_graphs: int, num_nodes: int, nnz: int, hidden_size: int):
    """One GCN batch, graphs [start, start + num_graphs) of the epoch whose gcn_epoch_table is `epoch_tab`, gathered from dataset-level
    tables in one launch (ggnn_gcn_assemble_batch): node_ptr int32 [Gd+1], feat float32 [Nd, A], csr / csr_t = (row_ptr int32 [Nd+1],
    col int32 [nnz_d], val float32 [nnz_d]) of A_hat and A_hat^T over global node ids, targets float32 [Gd, num_targets], label_mask
    float32 [Gd, K] or None, task_ids int64 [K] (target columns).  num_nodes / nnz are the batch's totals, known on the host.
    -> (GCNGraph, h0 [V, hidden_size], graph_nodes_list int32 [V], graph_ptr int32 [G+1], node_uid int64 [V],
        target_values [K, G], target_mask [K, G]).  Nothing is read back; every argument is checked before the launch."""
    def req(t, dtype, name):                         # (dtype and layout first, the device last: checkable without a GPU)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError("%s must be a %s tensor, got %s" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        return t
    req(node_ptr, torch.int32, "node_ptr")
    req(feat, torch.float32, "feat")
    rp, col, val = [req(t, dt, n) for t, dt, n in zip(csr, (torch.int32, torch.int32, torch.float32), ("row_ptr", "col", "val"))]
    rpt, colt, valt = [req(t, dt, n) for t, dt, n in zip(csr_t, (torch.int32, torch.int32, torch.float32), ("row_ptr_t", "col_t", "val_t"))]
    req(targets, torch.float32, "targets")
    if label_mask is not None:
        req(label_mask, torch.float32, "label_mask")
    req(task_ids, torch.int64, "task_ids")
    req(epoch_tab, torch.int32, "epoch_tab")
    dev = feat.device
    tensors = [node_ptr, rp, col, val, rpt, colt, valt, targets, task_ids, epoch_tab] + ([label_mask] if label_mask is not None else [])
    if any(t.device != dev for t in tensors):
        raise ValueError("gcn_assemble_batch: every table must be on %s" % dev)
    Gd = node_ptr.numel() - 1
    if node_ptr.dim() != 1 or Gd < 0 or feat.dim() != 2:
        raise ValueError("node_ptr must be [Gd+1] and feat [Nd, A]")
    Nd, A = feat.shape
    nnz_d = col.numel()
    if rp.numel() != Nd + 1 or rpt.numel() != Nd + 1 or val.numel() != nnz_d or colt.numel() != nnz_d or valt.numel() != nnz_d:
        raise ValueError("A_hat tables: row_ptr [%d], col/val/col_t/val_t [nnz] expected, got %s" % (
            Nd + 1, [t.numel() for t in (rp, col, val, rpt, colt, valt)]))
    if targets.dim() != 2 or targets.shape[0] != Gd or task_ids.dim() != 1:
        raise ValueError("targets must be [Gd, num_targets] and task_ids [K]")
    K = task_ids.numel()
    if label_mask is not None and tuple(label_mask.shape) != (Gd, K):
        raise ValueError("label_mask must be [%d, %d], got %s" % (Gd, K, tuple(label_mask.shape)))
    if epoch_tab.dim() != 1 or (epoch_tab.numel() - 2) % 3:
        raise ValueError("epoch_tab must be gcn_epoch_table's [3 Ge + 2]")
    Ge = (epoch_tab.numel() - 2) // 3
    s, G, V, E, D = int(start), int(num_graphs), int(num_nodes), int(nnz), int(hidden_size)
    if s < 0 or G < 0 or s + G > Ge:
        raise ValueError("batch [%d, %d) outside the epoch's %d graphs" % (s, s + G, Ge))
    if not 0 <= V <= Nd or not 0 <= E <= nnz_d or (G == 0 and (V or E)):
        raise ValueError("batch totals V=%d nnz=%d outside the dataset's %d nodes / %d entries" % (V, E, Nd, nnz_d))
    if D <= 0 or A > D:
        raise ValueError("hidden_size %d must be positive and >= the annotation size %d" % (D, A))
    if not feat.is_cuda:
        raise TypeError("gcn_assemble_batch needs CUDA/HIP tensors (there is no CPU implementation)")
    lib = _lib.load()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    h0 = f32(V, D)
    g_rp, g_col, g_val, g_rpt, g_colt, g_valt = i32(V + 1), i32(E), f32(E), i32(V + 1), i32(E), f32(E)
    gnl, graph_ptr = i32(V), i32(G + 1)
    uid = torch.empty(V, dtype=torch.int64, device=dev)
    tv, tm = f32(K, G), f32(K, G)
    nz = lambda t: _ptr(t) if t is not None and t.numel() else None
    c_ds = (ctypes.c_void_p * 10)(*[nz(t) for t in (node_ptr, feat, rp, col, val, rpt, colt, valt, targets, label_mask)])
    c_out = (ctypes.c_void_p * 12)(*[nz(t) for t in (h0, g_rp, g_col, g_val, g_rpt, g_colt, g_valt, gnl, graph_ptr, uid, tv, tm)])
    _launch("gcn_assemble_batch", lambda: lib.ggnn_gcn_assemble_batch(c_ds, Gd, A, targets.shape[1], nz(task_ids), K, _ptr(epoch_tab), Ge,
                                                                      s, G, V, E, D, c_out, _stream()))
    return GCNGraph(g_rp, g_col, g_val, g_rpt, g_colt, g_valt, V), h0, gnl, graph_ptr, uid, tv, tm


# ---- dense GGNN batches from dataset-level tables (DenseGGNNChemModel with pack_on_device) --------------------------------------
# data_device.dense_tables_host's device arrays that the assembly reads; the last nine are the compaction tables
DENSE_GRAPH_TABLES = ("node_ptr", "counts_t", "msg_ptr", "msg", "nin", "in_ptr", "slot_msg", "pair_ptr", "pair_node", "msg_crow",
                      "src_ptr", "src_msg", "rows_msg", "pair_rows", "node_pptr", "node_order")


def dense_epoch_table(counts_t: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """Prefix sums of the per-graph message and pair counts over an epoch's order, on the device (ggnn_pack_batch_tables, one launch
    per epoch).  counts_t int32 [2T, Gd] (messages per type, then active (source, type) pairs per type), order int64 [Ge] -> int32
    [Ge | 2T x (Ge+1)]: the order as int32, then per row the totals of the graphs before each epoch position."""
    lib = _lib.load()
    _req(counts_t, torch.int32, "counts_t")
    _req(order, torch.int64, "order")
    rows = counts_t.shape[0] if counts_t.dim() == 2 else 0
    if rows < 2 or rows % 2 or order.dim() != 1 or order.device != counts_t.device:
        raise ValueError("counts_t must be [2T, Gd] and order [Ge] on its device")
    Ge = order.numel()
    tab = torch.empty(Ge + rows * (Ge + 1), dtype=torch.int32, device=order.device)
    _launch("dense_epoch_table", lambda: lib.ggnn_pack_batch_tables(_ptr(counts_t), counts_t.shape[1], rows, _ptr(order) if Ge else None,
                                                                    Ge, None, None, 0, None, 0, _ptr(tab), None, None, _stream()))
    return tab


def dense_assemble_batch(tables, feat: torch.Tensor, targets: torch.Tensor, label_mask: Optional[torch.Tensor], task_ids: torch.Tensor,
                         epoch_tab: torch.Tensor, start: int, num_graphs: int, num_vertices: int, hidden_size: int,
                         type_off: Optional[Sequence[int]] = None, type_row_off: Optional[Sequence[int]] = None, sparse: bool = False,
                         compact: bool = False, arange=None) -> Dict[str, Any]:
    """One dense batch, graphs [start, start + num_graphs) of the epoch whose dense_epoch_table is `epoch_tab`, each padded to
    num_vertices nodes, in one launch (ggnn_dense_assemble_batch) from data_device.dense_tables_host's arrays on the device (`tables`,
    by the names of DENSE_GRAPH_TABLES), feat float32 [Nd, A], targets float32 [Gd, num_targets], label_mask float32 [Gd, K] or None,
    task_ids int64 [K] (target columns).
    -> {'initial_node_representation' [G, v, D], 'adjacency_matrix' [G, T, v, v], 'node_mask' [G, v], 'target_values' [K, G],
        'target_mask' [K, G]}: data.pack_dense_batch's arrays.  sparse: also 'nin' [G*v, T] and 'index', the MessageIndex that
    build_message_index builds from the batch's A.nonzero() (type_off: the batch's per-type message offsets, host ints [T+1]);
    compact: with the CompactSources, source index and CompactBackward that build_compact_sources / compact_backward attach to it
    (type_row_off: per-type pair offsets; arange(n): an int32 ramp for the backward's identity rows, default torch.arange).
    Nothing is read back; every argument is checked before the launch."""
    def req(t, dtype, name):                         # (dtype and layout first, the device last: checkable without a GPU)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError("%s must be a %s tensor, got %s" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        return t
    if compact and not sparse:
        raise ValueError("the compaction structures belong to the sparse form: compact needs sparse")
    names = DENSE_GRAPH_TABLES if compact else DENSE_GRAPH_TABLES[:7]
    tab = {}
    for name in names:
        if tables.get(name) is None:
            raise ValueError("dense table %r missing" % name)
        tab[name] = req(tables[name], torch.float32 if name == "nin" else torch.int32, name)
    req(feat, torch.float32, "feat")
    req(targets, torch.float32, "targets")
    if label_mask is not None:
        req(label_mask, torch.float32, "label_mask")
    req(task_ids, torch.int64, "task_ids")
    req(epoch_tab, torch.int32, "epoch_tab")
    dev = feat.device
    if any(t.device != dev for t in list(tab.values()) + [targets, task_ids, epoch_tab] + ([label_mask] if label_mask is not None else [])):
        raise ValueError("dense_assemble_batch: every table must be on %s" % dev)
    ct = tab["counts_t"]
    if ct.dim() != 2 or ct.shape[0] % 2 or not 1 <= ct.shape[0] // 2 <= 16 or feat.dim() != 2 or tab["msg"].dim() != 2:
        raise ValueError("counts_t must be [2T, Gd] with 1 <= T <= 16, feat [Nd, A] and msg [Md, 2]")
    T, Gd = ct.shape[0] // 2, ct.shape[1]
    Nd, A = feat.shape
    Md = tab["msg"].shape[0]
    shapes = {"node_ptr": (Gd + 1,), "msg_ptr": (Gd + 1,), "msg": (Md, 2), "nin": (Nd, T), "in_ptr": (Nd,), "slot_msg": (Md,)}
    if compact:
        Pd = tab["pair_node"].numel()
        shapes.update(pair_ptr=(Gd + 1,), pair_node=(Pd,), msg_crow=(Md,), src_ptr=(Nd * T,), src_msg=(Md,), rows_msg=(Md,),
                      pair_rows=(Pd,), node_pptr=(Nd,), node_order=(Pd,))
    for name, shape in shapes.items():
        if tuple(tab[name].shape) != shape:
            raise ValueError("dense table %s must be %s, got %s" % (name, shape, tuple(tab[name].shape)))
    if targets.dim() != 2 or targets.shape[0] != Gd or task_ids.dim() != 1:
        raise ValueError("targets must be [%d, num_targets] and task_ids [K]" % Gd)
    K = task_ids.numel()
    if label_mask is not None and tuple(label_mask.shape) != (Gd, K):
        raise ValueError("label_mask must be [%d, %d], got %s" % (Gd, K, tuple(label_mask.shape)))
    if epoch_tab.dim() != 1 or epoch_tab.numel() < 2 * T or (epoch_tab.numel() - 2 * T) % (2 * T + 1):
        raise ValueError("epoch_tab must be dense_epoch_table's [Ge + 2T (Ge + 1)]")
    Ge = (epoch_tab.numel() - 2 * T) // (2 * T + 1)
    s, G, v, D = int(start), int(num_graphs), int(num_vertices), int(hidden_size)
    if s < 0 or G < 0 or s + G > Ge:
        raise ValueError("batch [%d, %d) outside the epoch's %d graphs" % (s, s + G, Ge))
    if v < 1:
        raise ValueError("num_vertices %d: a dense batch has at least one vertex per graph" % v)
    if D <= 0 or A > D:
        raise ValueError("hidden_size %d must be positive and >= the annotation size %d" % (D, A))
    if G * v * T >= 2 ** 31 - 1 or T * v * v >= 2 ** 31 or v * D >= 2 ** 31:
        raise ValueError("batch too large for 32-bit indices: %d graphs of %d vertices, %d edge types, hidden size %d" % (G, v, T, D))

    def offsets(off, name):
        off = [int(x) for x in off] if off is not None else None
        if off is None or len(off) != T + 1 or off[0] != 0 or any(b < a for a, b in zip(off[:-1], off[1:])) or off[-1] >= 2 ** 31 - 1:
            raise ValueError("%s must be T + 1 = %d non-decreasing offsets from 0, got %s" % (name, T + 1, off))
        return off
    type_off = offsets(type_off, "type_off") if sparse else None
    type_row_off = offsets(type_row_off, "type_row_off") if compact else None
    M = type_off[-1] if sparse else 0
    R = type_row_off[-1] if compact else 0
    if not feat.is_cuda:
        raise TypeError("dense_assemble_batch needs CUDA/HIP tensors (there is no CPU implementation)")
    lib = _lib.load()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    V = G * v
    out = {'initial_node_representation': f32(G, v, D), 'adjacency_matrix': f32(G, T, v, v), 'node_mask': f32(G, v),
           'target_values': f32(K, G), 'target_mask': f32(K, G)}
    sp = [None] * 15
    if sparse:
        sp[:5] = [f32(V, T), i32(M, 2), i32(V + 1), i32(M), i32(M)]                  # nin, adj, row_ptr, gather_row, msg_perm
    if compact:
        sp[5:] = [i32(max(R, 1)), i32(M), i32(V * T + 1), i32(M), i32(M), i32(R + 1), i32(M), i32(M), i32(V + 1), i32(R)]
    nz = lambda t: _ptr(t) if t is not None and t.numel() else None
    # (counts_t is not passed: the epoch table holds its prefix sums)
    ds = [tab["node_ptr"], feat, targets, label_mask] + [tab.get(n) for n in DENSE_GRAPH_TABLES[2:]]
    c_ds = (ctypes.c_void_p * 18)(*[nz(t) for t in ds])
    outs = [out[k] for k in ('initial_node_representation', 'adjacency_matrix', 'node_mask', 'target_values', 'target_mask')] + sp
    c_out = (ctypes.c_void_p * 20)(*[nz(t) for t in outs])
    c_to = (ctypes.c_int64 * (T + 1))(*(type_off or [0] * (T + 1)))
    c_tro = (ctypes.c_int64 * (T + 1))(*(type_row_off or [0] * (T + 1)))
    _launch("dense_assemble_batch", lambda: lib.ggnn_dense_assemble_batch(
        c_ds, Gd, A, T, targets.shape[1], nz(task_ids), K, _ptr(epoch_tab), Ge, s, G, v, D, M, R, c_to, c_tro, 1 if sparse else 0, c_out,
        _stream()))
    if sparse:
        nin, adj, row_ptr, gather_row, msg_perm = sp[:5]
        index = MessageIndex(adj, type_off, row_ptr, gather_row, msg_perm, V, T)
        if compact:
            pair_node, gather_c, src_rp, src_g, src_m, rows_rp, rows_g, rows_m, node_rp, node_order = sp[5:]
            comp = index._compact = CompactSources(pair_node[:max(R, 1)], type_row_off, gather_c)
            index._source_index = MessageIndex(adj, type_off, src_rp, src_g, src_m, V * T, T)
            bwd = object.__new__(CompactBackward)
            bwd.rows_index = SegmentIndex(rows_rp, rows_g, R, rows_m)
            bwd.source_node_index = SegmentIndex(src_rp[::T].contiguous(), src_g, V, src_m)
            bwd.node_index = SegmentIndex(node_rp, node_order, V)
            ramp = arange(max(R, 1)) if arange is not None else torch.arange(max(R, 1), dtype=torch.int32, device=dev)
            bwd.identity = CompactSources(ramp, type_row_off, gather_c)
            comp._bwd = bwd
        out.update(nin=nin, index=index)
    return out


def gcn_fused_supported(D: int) -> bool:
    return bool(_lib.load().ggnn_gcn_fused_supported(int(D)))


def gcn_pack(W: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """LDS image of W [D, D] (or of W^T) for the fused GCN layer."""
    lib = _lib.load()
    _req(W, torch.float32, "W")
    D = W.shape[0]
    img = torch.empty(lib.ggnn_gcn_image_bytes(D) // 4, dtype=torch.float32, device=W.device)
    _launch("gcn_pack", lambda: lib.ggnn_gcn_pack_weights_f32(_ptr(W), D, 1 if transpose else 0, _ptr(img), _stream()))
    return img


def gcn_panel_supported(D: int) -> bool:
    """Hidden sizes with the column-panel fused GCN layer (128 / 192 / 256; csrc/ggnn_gcn_panel.hip)."""
    return bool(_lib.load().ggnn_gcn_panel_supported(int(D)))


def gcn_panel_launch_geometry() -> Tuple[int, int]:
    """(rows a workgroup of the panel GCN layer takes per pass, the launcher's cap on workgroups)."""
    rows, cap = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().ggnn_gcn_panel_launch_geometry(ctypes.byref(rows), ctypes.byref(cap))
    return rows.value, cap.value


def gcn_panel_pack(W: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """The D / 64 column-panel images of W [D, D] (or of W^T) for the panel GCN layer."""
    lib = _lib.load()
    _req(W, torch.float32, "W")
    D = W.shape[0]
    if tuple(W.shape) != (D, D) or not gcn_panel_supported(D):
        raise ValueError("gcn_panel_pack: W must be [D, D] with D in 128 / 192 / 256 (got %s)" % (tuple(W.shape),))
    img = torch.empty(lib.ggnn_gcn_panel_image_bytes(D) // 4, dtype=torch.float32, device=W.device)
    _launch("gcn_panel_pack", lambda: lib.ggnn_gcn_panel_pack_weights_f32(_ptr(W), D, 1 if transpose else 0, _ptr(img), _stream()))
    return img


def gcn_layer(x: torch.Tensor, graph: GCNGraph, W: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
              keep_prob: float = 1.0, seed: int = 0, row_key: Optional[torch.Tensor] = None, transpose: bool = False,
              save_s: bool = False, fused: Optional[bool] = None, img: Optional[torch.Tensor] = None, panel: bool = False):
    """One GCN layer  out = dropout(relu(M x W' + bias))  with M = A_hat, W' = W, or (transpose=True, the backward's
    dx = A_hat^T (dP W^T)) M = A_hat^T, W' = W^T.  -> (out, S = M x if save_s else None).
    Fused single launch for hidden sizes 32 / 64 / 100 (ggnn_gcn_layer_f32); otherwise (or fused=False) the composition
    ggnn_weighted_segment_sum_f32 -> ggnn_gemm_f32 -> ggnn_gcn_epilogue_f32.  panel=True (opt-in): hidden sizes 128 / 192 / 256 take
    ONE ggnn_gcn_panel_layer_f32 launch instead of the composition (img: gcn_panel_pack's images; packed here when None); at any
    other size the argument changes nothing.  The dropout mask is ggnn_dropout_f32's for (seed, row key, column)."""
    lib = _lib.load()
    _req(x, torch.float32, "x")
    V, D = x.shape
    if V != graph.num_nodes:
        raise ValueError("x has %d rows, the graph %d nodes" % (V, graph.num_nodes))
    if tuple(W.shape) != (D, D):
        raise ValueError("W must be [%d, %d]" % (D, D))
    if bias is not None:
        _req(bias, torch.float32, "bias")
    if row_key is not None:
        _req(row_key, torch.int64, "row_key")
    rp, col, val = (graph.row_ptr_t, graph.col_t, graph.val_t) if transpose else (graph.row_ptr, graph.col, graph.val)
    out = torch.empty_like(x)
    S = torch.empty_like(x) if save_s else None
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if panel and gcn_panel_supported(D):
        if img is None:
            img = gcn_panel_pack(W.contiguous(), transpose)
        _launch("gcn_panel_layer[D=%d]" % D, lambda: lib.ggnn_gcn_panel_layer_f32(
            _ptr(x), _ptr(rp), _ptr(col), _ptr(val), graph.nnz, _ptr(img), _ptr(bias), 1 if relu else 0, _ptr(row_key), 0, seed,
            float(keep_prob), _ptr(out), _ptr(S), V, D, _stream()))
        return out, S
    if fused is None:
        fused = gcn_fused_supported(D)
    if fused:
        if img is None:
            img = gcn_pack(W.contiguous(), transpose)
        _launch("gcn_layer[D=%d]" % D, lambda: lib.ggnn_gcn_layer_f32(
            _ptr(x), _ptr(rp), _ptr(col), _ptr(val), graph.nnz, _ptr(img), _ptr(bias), 1 if relu else 0, _ptr(row_key), 0, seed,
            float(keep_prob), _ptr(out), _ptr(S), V, D, _stream()))
        return out, S
    Wm = (W.t() if transpose else W).contiguous()
    Dk = kernel_width(D)
    if Dk == D:
        agg = weighted_segment_sum(x, SegmentIndex(rp, col, V), graph.slot_ids(), val, out=S)
        P = gemm([agg], Wm)
    else:
        # (the GEMM takes K = 32 / 64 / 100 / multiples: the aggregate and W's rows zero-padded to kernel_width(D))
        import torch.nn.functional as F
        agg = weighted_segment_sum(F.pad(x, (0, Dk - D)), SegmentIndex(rp, col, V), graph.slot_ids(), val)
        P = gemm([agg], F.pad(Wm, (0, 0, 0, Dk - D)))
        if save_s:
            S.copy_(agg[:, :D])
            agg = S
    _launch("gcn_epilogue", lambda: lib.ggnn_gcn_epilogue_f32(_ptr(P), _ptr(bias), 1 if relu else 0, _ptr(row_key), 0, seed,
                                                               float(keep_prob), _ptr(out), V, D, _stream()))
    return out, agg if save_s else None


def gcn_layer_bwd(dP: torch.Tensor, graph: GCNGraph, W: torch.Tensor, gate_out: torch.Tensor, keep_prob: float = 1.0, seed: int = 0,
                  row_key: Optional[torch.Tensor] = None, img: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of one fused GCN layer with the gate of the layer below in its epilogue, one launch (ggnn_gcn_layer_bwd_f32):
    -> [gate_out > 0] * dropout(A_hat^T (dP W^T)), the dP of the layer below, whose forward output dropout(relu(P)) is gate_out and
    whose dropout is (keep_prob, seed, row_key).  Bit-identical to act_bwd(dropout(gcn_layer(dP, graph, W, transpose=True)[0], ...),
    gate_out, "relu").  Hidden sizes 32 / 64 / 100 only; img: the image of W^T (gcn_pack(W, True)) when the caller has it."""
    lib = _lib.load()
    _req(dP, torch.float32, "dP")
    _req(gate_out, torch.float32, "gate_out")
    V, D = dP.shape
    if V != graph.num_nodes:
        raise ValueError("dP has %d rows, the graph %d nodes" % (V, graph.num_nodes))
    if tuple(W.shape) != (D, D) or tuple(gate_out.shape) != (V, D):
        raise ValueError("W must be [%d, %d], gate_out [%d, %d]" % (D, D, V, D))
    if row_key is not None:
        _req(row_key, torch.int64, "row_key")
    if not gcn_fused_supported(D):
        raise ValueError("gcn_layer_bwd: hidden size %d has no fused GCN kernel" % D)
    if img is None:
        img = gcn_pack(W.contiguous(), True)
    out = torch.empty_like(dP)
    _launch("gcn_layer_bwd[D=%d]" % D, lambda: lib.ggnn_gcn_layer_bwd_f32(
        _ptr(dP), _ptr(graph.row_ptr_t), _ptr(graph.col_t), _ptr(graph.val_t), graph.nnz, _ptr(img), _ptr(gate_out), _ptr(row_key), 0,
        int(seed) & 0xFFFFFFFFFFFFFFFF, float(keep_prob), _ptr(out), V, D, _stream()))
    return out


def gcn_train_pack(weights: Sequence[torch.Tensor]) -> torch.Tensor:
    """Every weight image of a GCN training step in one launch (ggnn_gcn_train_pack_f32) -> float32 [2L - 1, slot]: row l the image
    of W_l, row L + l - 1 the image of W_l^T for l >= 1; a row's first ggnn_gcn_image_bytes(D) / 4 floats are gcn_pack's."""
    lib = _lib.load()
    Ws = [_req(w, torch.float32, "W") for w in weights]
    L, D = len(Ws), Ws[0].shape[0]
    slot = (lib.ggnn_gcn_image_bytes(D) + 255) // 256 * 256 // 4
    images = torch.empty((2 * L - 1, slot), dtype=torch.float32, device=Ws[0].device)
    w_arr = _ptr_array(Ws)
    _launch("gcn_train_pack[D=%d,L=%d]" % (D, L), lambda: lib.ggnn_gcn_train_pack_f32(w_arr, L, D, _ptr(images), _stream()))
    return images


def gcn_panel_layer_bwd(dP: torch.Tensor, graph: GCNGraph, W: torch.Tensor, gate_out: torch.Tensor, keep_prob: float = 1.0,
                        seed: int = 0, row_key: Optional[torch.Tensor] = None, img: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gcn_layer_bwd at hidden sizes 128 / 192 / 256, one launch of the panel kernel (ggnn_gcn_panel_layer_bwd_f32):
    -> [gate_out > 0] * dropout(A_hat^T (dP W^T)).  Bit-identical to act_bwd(dropout(gcn_layer(dP, graph, W, transpose=True,
    panel=True)[0], ...), gate_out, "relu").  img: the panel images of W^T (gcn_panel_pack(W, True)) when the caller has them."""
    lib = _lib.load()
    _req(dP, torch.float32, "dP")
    _req(gate_out, torch.float32, "gate_out")
    V, D = dP.shape
    if V != graph.num_nodes:
        raise ValueError("dP has %d rows, the graph %d nodes" % (V, graph.num_nodes))
    if tuple(W.shape) != (D, D) or tuple(gate_out.shape) != (V, D):
        raise ValueError("W must be [%d, %d], gate_out [%d, %d]" % (D, D, V, D))
    if row_key is not None:
        _req(row_key, torch.int64, "row_key")
    if not gcn_panel_supported(D):
        raise ValueError("gcn_panel_layer_bwd: hidden size %d has no panel GCN kernel" % D)
    if img is None:
        img = gcn_panel_pack(W.contiguous(), True)
    out = torch.empty_like(dP)
    _launch("gcn_panel_layer_bwd[D=%d]" % D, lambda: lib.ggnn_gcn_panel_layer_bwd_f32(
        _ptr(dP), _ptr(graph.row_ptr_t), _ptr(graph.col_t), _ptr(graph.val_t), graph.nnz, _ptr(img), _ptr(gate_out), _ptr(row_key), 0,
        int(seed) & 0xFFFFFFFFFFFFFFFF, float(keep_prob), _ptr(out), V, D, _stream()))
    return out


def gcn_panel_train_pack(weights: Sequence[torch.Tensor]) -> torch.Tensor:
    """Every panel image of a GCN training step in one launch (ggnn_gcn_panel_train_pack_f32) -> float32 [2L - 1, slot]: row l the
    images of W_l, row L + l - 1 those of W_l^T for l >= 1; a row's first ggnn_gcn_panel_image_bytes(D) / 4 floats are gcn_panel_pack's."""
    lib = _lib.load()
    Ws = [_req(w, torch.float32, "W") for w in weights]
    L, D = len(Ws), Ws[0].shape[0]
    if not gcn_panel_supported(D) or any(tuple(w.shape) != (D, D) for w in Ws):
        raise ValueError("gcn_panel_train_pack: every W must be [D, D] with D in 128 / 192 / 256")
    slot = (lib.ggnn_gcn_panel_image_bytes(D) + 255) // 256 * 256 // 4
    images = torch.empty((2 * L - 1, slot), dtype=torch.float32, device=Ws[0].device)
    w_arr = _ptr_array(Ws)
    _launch("gcn_panel_train_pack[D=%d,L=%d]" % (D, L), lambda: lib.ggnn_gcn_panel_train_pack_f32(w_arr, L, D, _ptr(images), _stream()))
    return images


def _gcn_propagate(name: str, workspace_bytes, entry, h0: torch.Tensor, graph: GCNGraph, weights: Sequence[torch.Tensor],
                   biases: Optional[Sequence[torch.Tensor]]) -> torch.Tensor:
    """One whole-stack inference call: `entry` is ggnn_gcn_propagate_f32 or its panel form, `workspace_bytes` its size query."""
    _req(h0, torch.float32, "h0")
    V, D = h0.shape
    L = len(weights)
    ws_bytes = workspace_bytes(V, D, L)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=h0.device)
    out = torch.empty_like(h0)
    Ws = [_req(w, torch.float32, "W") for w in weights]
    bs = None if biases is None else [_req(b, torch.float32, "bias") for b in biases]
    w_arr = _ptr_array(Ws)
    b_arr = None if bs is None else _ptr_array(bs)
    _launch("%s[D=%d,L=%d]" % (name, D, L), lambda: entry(
        _ptr(h0), V, D, L, _ptr(graph.row_ptr), _ptr(graph.col), _ptr(graph.val), graph.nnz, w_arr, b_arr, _ptr(out), _ptr(ws),
        ws_bytes, _stream()))
    return out


def gcn_propagate(h0: torch.Tensor, graph: GCNGraph, weights: Sequence[torch.Tensor],
                  biases: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """Inference forward of all layers (ReLU on all but the last) in one native call, ggnn_gcn_propagate_f32 (fused sizes only)."""
    lib = _lib.load()
    return _gcn_propagate("gcn_propagate", lib.ggnn_gcn_workspace_bytes, lib.ggnn_gcn_propagate_f32, h0, graph, weights, biases)


def gcn_panel_propagate(h0: torch.Tensor, graph: GCNGraph, weights: Sequence[torch.Tensor],
                        biases: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """gcn_propagate at hidden sizes 128 / 192 / 256: all layers on the panel kernel in one native call (ggnn_gcn_panel_propagate_f32)."""
    lib = _lib.load()
    return _gcn_propagate("gcn_panel_propagate", lib.ggnn_gcn_panel_workspace_bytes, lib.ggnn_gcn_panel_propagate_f32, h0, graph,
                          weights, biases)
