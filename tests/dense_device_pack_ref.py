"""NumPy restatement of the dense device packer (ggnn_dense_assemble_batch): per-graph tables in local node ids, built once for the
dataset (data_device.dense_tables_host), then a batch as its graphs' pieces shifted by slot * v and by their offsets in the batch's
type-major lists.  sparse_form_from_dense is an independent construction of what the training step builds from A.
test_dense_device_pack_host.py pins the restatement to data.pack_dense_batch and to sparse_form_from_dense; the GPU tests hold the
kernel to it."""
import numpy as np

DENSE_KEYS = (("initial_node_representation", "h0"), ("adjacency_matrix", "A"), ("node_mask", "mask"), ("target_values", "tv"),
              ("target_mask", "tm"))
INDEX_KEYS = ("adj", "row_ptr", "gather_row", "msg_perm")
COMPACT_KEYS = ("pair_node", "gather_c", "src_rp", "src_gather", "src_msg", "rows_rp", "rows_gather", "rows_msg", "node_rp",
                "node_order")


def batch_offsets(tab, ids):
    """The batch's per-type message and pair offsets (host ints [T+1]), from the per-graph count tables."""
    ids = np.asarray(ids, np.int64)
    T = tab["mc"].shape[1]
    mc = tab["mc"][ids].reshape(-1, T).sum(axis=0)
    pc = tab["pc"][ids].reshape(-1, T).sum(axis=0)
    return [0] + [int(x) for x in np.cumsum(mc)], [0] + [int(x) for x in np.cumsum(pc)]


def assemble(tab, feat, targets, label_mask, task_ids, ids, v, D):
    """The batch of graphs `ids` (slot k holds ids[k]) with v vertices per graph, as ggnn_dense_assemble_batch writes it in training
    form (the dense feeds and the whole sparse form, compaction structures included)."""
    ids = np.asarray(ids, np.int64)
    T = tab["mc"].shape[1]
    G, V = len(ids), len(ids) * v
    mc, pc = tab["mc"][ids].reshape(G, T), tab["pc"][ids].reshape(G, T)
    type_off, type_row_off = (np.asarray(o, np.int64) for o in batch_offsets(tab, ids))
    M, R = int(type_off[-1]), int(type_row_off[-1])
    mo, po = np.cumsum(mc, axis=0) - mc, np.cumsum(pc, axis=0) - pc        # graph k's first entry in the batch's type-t lists
    mtot = np.cumsum(mc.sum(axis=1)) - mc.sum(axis=1)                       # graph k's first by-target slot
    ptot = np.cumsum(pc.sum(axis=1)) - pc.sum(axis=1)                       # graph k's first compact row in node order
    i32 = lambda *shape: np.zeros(shape, np.int32)
    out = {"h0": np.zeros((G, v, D), np.float32), "A": np.zeros((G, T, v, v), np.float32), "mask": np.zeros((G, v), np.float32),
           "nin": np.zeros((V, T), np.float32), "adj": i32(M, 2), "row_ptr": i32(V + 1), "gather_row": i32(M), "msg_perm": i32(M),
           "pair_node": i32(R), "gather_c": i32(M), "src_rp": i32(V * T + 1), "src_gather": i32(M), "src_msg": i32(M),
           "rows_rp": i32(R + 1), "rows_gather": i32(M), "rows_msg": i32(M), "node_rp": i32(V + 1), "node_order": i32(R)}
    for k, g in enumerate(ids):
        n0, n = int(tab["node_ptr"][g]), int(tab["node_ptr"][g + 1] - tab["node_ptr"][g])
        m0, Mg = int(tab["msg_ptr"][g]), int(tab["msg_ptr"][g + 1] - tab["msg_ptr"][g])
        q0, Pg = int(tab["pair_ptr"][g]), int(tab["pair_ptr"][g + 1] - tab["pair_ptr"][g])
        assert n <= v
        base = k * v
        cm, cp = np.cumsum(mc[k]) - mc[k], np.cumsum(pc[k]) - pc[k]
        msg = tab["msg"][m0:m0 + Mg].astype(np.int64)                       # (src, dst), local
        t_of = np.repeat(np.arange(T), mc[k])
        pos = type_off[t_of] + mo[k, t_of] + np.arange(Mg) - cm[t_of]      # batch message id of every local message
        out["h0"][k, :n, :feat.shape[1]] = feat[n0:n0 + n]
        out["mask"][k, :n] = 1.0
        out["A"][k, t_of, msg[:, 1], msg[:, 0]] = 1.0
        out["nin"][base:base + n] = tab["nin"][n0:n0 + n]
        out["adj"][pos] = msg + base
        out["row_ptr"][base:base + v] = mtot[k] + np.concatenate([tab["in_ptr"][n0:n0 + n], np.full(v - n, Mg)])
        slots = mtot[k] + np.arange(Mg)
        j = tab["slot_msg"][m0:m0 + Mg]
        out["gather_row"][slots] = (base + msg[j, 0]) * T + t_of[j]
        out["msg_perm"][slots] = pos[j]
        out["gather_c"][slots] = type_row_off[t_of[j]] + po[k, t_of[j]] + tab["msg_crow"][m0 + j]
        p_t = np.repeat(np.arange(T), pc[k])
        rows = type_row_off[p_t] + po[k, p_t] + np.arange(Pg) - cp[p_t]    # batch compact row of every local pair
        out["pair_node"][rows] = base + tab["pair_node"][q0:q0 + Pg]
        out["rows_rp"][rows] = type_off[p_t] + mo[k, p_t] + tab["pair_rows"][q0:q0 + Pg]
        out["src_rp"][base * T:(base + v) * T] = mtot[k] + np.concatenate([tab["src_ptr"][n0 * T:(n0 + n) * T], np.full((v - n) * T, Mg)])
        j = tab["src_msg"][m0:m0 + Mg]
        out["src_gather"][slots] = base + msg[j, 1]
        out["src_msg"][slots] = pos[j]
        j = tab["rows_msg"][m0:m0 + Mg]                                     # (compact-row order has the type ranges of the messages)
        out["rows_gather"][pos] = base + msg[j, 1]
        out["rows_msg"][pos] = pos[j]
        out["node_rp"][base:base + v] = ptot[k] + np.concatenate([tab["node_pptr"][n0:n0 + n], np.full(v - n, Pg)])
        out["node_order"][ptot[k] + np.arange(Pg)] = rows[tab["node_order"][q0:q0 + Pg]]
    out["row_ptr"][V] = out["src_rp"][V * T] = out["rows_rp"][R] = M
    out["node_rp"][V] = R
    K = len(task_ids)
    lm = np.ones((len(targets), K), np.float32) if label_mask is None else np.asarray(label_mask, np.float32)
    out["tm"] = lm[ids].T.astype(np.float32).copy()
    out["tv"] = np.asarray(targets)[ids][:, list(task_ids)].T.astype(np.float32) * out["tm"]
    out.update(type_off=[int(x) for x in type_off], type_row_off=[int(x) for x in type_row_off], M=M, R=R)
    return out


def sparse_form_from_dense(A):
    """What DenseGGNNChemModel._compute_for_training derives from A (A.nonzero(), build_message_index) and what
    build_compact_sources / compact_backward build from that, restated independently: stable sorts by target, by (source, type)
    and by node over the nonzero entries of A."""
    b, T, v, _ = A.shape
    V = b * v
    nz = np.stack(np.nonzero(A), axis=1).astype(np.int64)                   # (b, e, dst, src), lexicographic
    src, dst, et = nz[:, 0] * v + nz[:, 3], nz[:, 0] * v + nz[:, 2], nz[:, 1]
    o = np.argsort(et, kind="stable")                                       # type-major lists, nonzero order inside a type
    src, dst, et = src[o], dst[o], et[o]
    slots = np.argsort(dst, kind="stable")
    out = {"adj": np.stack([src, dst], axis=1).astype(np.int32),
           "type_off": [0] + [int(x) for x in np.cumsum(np.bincount(et, minlength=T))],
           "row_ptr": np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=V))]).astype(np.int32),
           "gather_row": (src[slots] * T + et[slots]).astype(np.int32), "msg_perm": slots.astype(np.int32),
           "nin": A.sum(axis=3).transpose(0, 2, 1).reshape(V, T).astype(np.float32)}
    key = src * T + et
    by_src = np.argsort(key, kind="stable")
    src_rp = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=V * T))]).astype(np.int64)
    out.update(src_rp=src_rp.astype(np.int32), src_gather=dst[by_src].astype(np.int32), src_msg=by_src.astype(np.int32))
    pkey = np.unique(et * V + src)                                          # active (source, type) pairs, type-major, node ascending
    pn, pt = pkey % V, pkey // V
    out.update(pair_node=pn.astype(np.int32), type_row_off=[0] + [int(x) for x in np.cumsum(np.bincount(pt, minlength=T))],
               gather_c=np.searchsorted(pkey, (et * V + src)[slots]).astype(np.int32))
    seg = pn * T + pt
    start, length = src_rp[seg], src_rp[seg + 1] - src_rp[seg]
    rslots = np.concatenate([np.arange(a, a + n) for a, n in zip(start, length)] + [np.zeros(0, np.int64)]).astype(np.int64)
    out.update(rows_rp=np.concatenate([[0], np.cumsum(length)]).astype(np.int32), rows_gather=out["src_gather"][rslots],
               rows_msg=out["src_msg"][rslots], node_rp=np.concatenate([[0], np.cumsum(np.bincount(pn, minlength=V))]).astype(np.int32),
               node_order=np.argsort(pn, kind="stable").astype(np.int32))
    return out


def as_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def assert_bits_equal(got, want, name):
    got, want = as_np(got), as_np(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), name


def device_sparse_arrays(index, nin, compact):
    """The arrays of a device batch's sparse form under the names of assemble() (CompactSources' pair_node cut to its R rows)."""
    out = {"adj": index.adj, "row_ptr": index.row_ptr, "gather_row": index.gather_row, "msg_perm": index.msg_perm, "nin": nin}
    if compact:
        comp, src = index._compact, index._source_index
        bwd = comp._bwd
        R = comp.num_rows
        out.update(pair_node=comp.pair_node[:R], gather_c=comp.gather_row, src_rp=src.row_ptr, src_gather=src.gather_row,
                   src_msg=src.msg_perm, rows_rp=bwd.rows_index.row_ptr, rows_gather=bwd.rows_index.gather_row,
                   rows_msg=bwd.rows_index.msg, node_rp=bwd.node_index.row_ptr, node_order=bwd.node_index.gather_row)
    return out
