"""NumPy restatement of the GCN device packer (ggnn_gcn_assemble_batch): dataset-level A_hat tables built once by
ops.gcn_csr_host over all graphs with global node ids, then a batch as per-graph slices of them, shifted by the batch's node and
entry offsets.  test_gcn_device_pack_host.py pins it to pack_batch + gcn_csr_host; the GPU tests hold the kernel to it."""
import numpy as np


def dataset_tables(ops, node_ptr, entry_ptr, adjacency_list, adjacency_weights):
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    ne = np.diff(np.asarray(entry_ptr, dtype=np.int64))
    glob = np.asarray(adjacency_list, dtype=np.int64) + np.repeat(node_ptr[:-1], ne)[:, None]
    parts = ops.gcn_csr_host(glob, adjacency_weights, int(node_ptr[-1]))
    return {"node_ptr": node_ptr, "npg": np.diff(node_ptr), "ne": ne, "csr": parts[:3], "csr_t": parts[3:]}


def _slice_csr(csr, n0, n, no, eo):
    rp, col, val = csr
    e0, e1 = int(rp[n0]), int(rp[n0 + n])
    return rp[n0:n0 + n] - e0 + eo, col[e0:e1] - n0 + no, val[e0:e1]


def assemble(tab, feat, targets, label_mask, task_ids, order, s, e, D):
    """The batch of epoch positions [s, e) of `order`, as ggnn_gcn_assemble_batch writes it."""
    ids = np.asarray(order[s:e], dtype=np.int64)
    G = len(ids)
    npg = tab["npg"][ids]
    ne = tab["ne"][ids]
    V, E = int(npg.sum()), int(ne.sum())
    node_off = np.concatenate([[0], np.cumsum(npg)])
    entry_off = np.concatenate([[0], np.cumsum(ne)])
    h0 = np.zeros((V, D), np.float32)
    out = {k: [] for k in ("row_ptr", "col", "val", "row_ptr_t", "col_t", "val_t")}
    for k, g in enumerate(ids):
        n0, n, no, eo = int(tab["node_ptr"][g]), int(npg[k]), int(node_off[k]), int(entry_off[k])
        h0[no:no + n, :feat.shape[1]] = feat[n0:n0 + n]
        for suffix, csr in (("", tab["csr"]), ("_t", tab["csr_t"])):
            rp, col, val = _slice_csr(csr, n0, n, no, eo)
            out["row_ptr" + suffix].append(rp)
            out["col" + suffix].append(col)
            out["val" + suffix].append(val)
    for key in out:
        dt = np.float32 if key.startswith("val") else np.int32
        out[key] = np.concatenate(out[key]).astype(dt) if out[key] else np.zeros(0, dt)
    out["row_ptr"] = np.append(out["row_ptr"], E).astype(np.int32)
    out["row_ptr_t"] = np.append(out["row_ptr_t"], E).astype(np.int32)
    mask = (np.ones((G, len(task_ids)), np.float32) if label_mask is None else np.asarray(label_mask, np.float32)[ids]).T
    y = np.asarray(targets, np.float32)[ids][:, np.asarray(task_ids, np.int64)].T
    local = np.arange(V, dtype=np.int64) - np.repeat(node_off[:-1], npg)
    out.update({
        "initial_node_representation": h0,
        "graph_nodes_list": np.repeat(np.arange(G, dtype=np.int32), npg),
        "graph_ptr": node_off.astype(np.int32),
        "node_uid": (np.repeat(ids, npg) << 20) + local,
        "target_values": np.where(mask > 0, y, 0.0).astype(np.float32),
        "target_mask": mask.astype(np.float32),
        "num_graphs": G, "V": V, "nnz": E,
    })
    return out


GRAPH_KEYS = ("row_ptr", "col", "val", "row_ptr_t", "col_t", "val_t")
FEED_KEYS = ("initial_node_representation", "graph_nodes_list", "graph_ptr", "node_uid", "target_values", "target_mask")


def as_np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def assert_bits_equal(got, want, name):
    got, want = as_np(got), as_np(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), name


def assert_batch_equal(graph, feed, want):
    """A GCNGraph + feed dict (device or host) against assemble()'s arrays, bit for bit."""
    for key in GRAPH_KEYS:
        assert_bits_equal(getattr(graph, key), want[key], key)
    for key in FEED_KEYS:
        assert_bits_equal(feed[key], want[key], key)
    assert int(feed["num_graphs"]) == want["num_graphs"]
