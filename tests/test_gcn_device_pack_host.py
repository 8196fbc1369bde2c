"""GCN device packer on the host: the NumPy restatement of "dataset-level tables, then slice and offset" (gcn_device_pack_ref.py)
equals pack_batch + gcn_csr_host bit for bit, the pack_on_device option refuses a CPU device, and the ops wrapper and the C entry
point reject bad arguments before any launch.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_device_pack_ref as R


def _dataset(pkg):
    """Synthetic molecules with two tasks plus the edge cases: a one-atom graph without bonds, a self-bond (A = 2 on the diagonal),
    a duplicate bond, a two-atom graph."""
    raw = pkg.synthetic_qm9(70, mean_nodes=9, seed=4, num_tasks=2).to_json()
    f = len(raw[0]["node_features"][0])
    one_hot = lambda n: [[1.0] + [0.0] * (f - 1)] * n
    raw[3] = {"targets": [[0.25], [-1.5]], "graph": [], "node_features": one_hot(1)}
    raw[10] = {"targets": [[1.0], [2.0]], "graph": [[0, 1, 1], [1, 2, 2], [1, 1, 1]], "node_features": one_hot(3)}
    raw[11] = {"targets": [[3.0], [4.0]], "graph": [[0, 1, 1], [1, 2, 0], [0, 1, 1], [1, 1, 2]], "node_features": one_hot(3)}
    raw[40] = {"targets": [[5.0], [6.0]], "graph": [[0, 2, 1]], "node_features": one_hot(2)}
    return raw


def _model(pkg, raw, device="cpu", **config):
    params = {"hidden_size": 36, "num_timesteps": 2, "random_seed": 3, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5},
              "batch_size": 60, "graph_state_dropout_keep_prob": 0.75}
    params.update(config)
    return pkg.SparseGCNChemModel({"--quiet": True, "--device": device, "train_data": raw, "valid_data": raw, "--config": params})


def _tables(pkg, data):
    ms = data["molecules"]
    return R.dataset_tables(pkg.ops, ms.node_ptr, data["entry_ptr"], data["adjacency_list"], data["adjacency_weights"])


def _host_batch(m, data, ids):
    feed = m.pack_batch(data, ids, 0.75)
    return feed["gcn_graph"], feed


def test_restatement_equals_host_packer(pkg):
    m = _model(pkg, _dataset(pkg))
    data = m.train_data
    ms = data["molecules"]
    tab = _tables(pkg, data)
    G = ms.num_graphs
    # the edge cases really are in the set: a one-atom graph with no entries but its diagonal, a diagonal weight from A = 2
    assert (tab["npg"] == 1).any() and (tab["ne"][tab["npg"] == 1] == 1).all()
    rng = np.random.default_rng(11)
    order = rng.permutation(G)
    bounds = pkg.data.batch_boundaries(tab["npg"][order], m.params["batch_size"])
    slices = list(zip(bounds[:-1], bounds[1:]))                                  # every batch of the epoch, first and last included
    pos = {int(g): int(p) for p, g in enumerate(order)}
    special = [int(g) for g in np.nonzero(tab["npg"] <= 3)[0]]                 # (training order is shuffled: the hand-made graphs
    assert len(special) >= 4                                                    #  3, 10, 11, 40 are among these)
    slices += [(pos[g], pos[g] + 1) for g in special]                          # single-graph batches
    slices += [(p, p + 1) for p in rng.choice(G, 8, replace=False)]
    for _ in range(10):
        s = int(rng.integers(0, G - 1))
        slices.append((s, int(rng.integers(s + 1, G + 1))))
    for s, e in slices:
        graph, feed = _host_batch(m, data, order[s:e])
        want = R.assemble(tab, ms.node_feat, ms.targets, data["label_mask"], m.params["task_ids"], order, s, e, 36)
        R.assert_batch_equal(graph, feed, want)
        assert graph.nnz == want["nnz"] and graph.num_nodes == want["V"]
    # the self-bond: A[1, 1] = 2 before the normalisation, row sum 4 (two neighbours), so the diagonal weight is 2 / 4 (+ O(1e-7))
    tab_v = _tables(pkg, m.valid_data)                                          # (unshuffled: graph 10 is raw[10])
    n0 = int(tab_v["node_ptr"][10])
    rp, col, val = tab_v["csr"]
    diag = [float(val[j]) for j in range(rp[n0 + 1], rp[n0 + 2]) if col[j] == n0 + 1]
    assert len(diag) == 1 and abs(diag[0] - 2.0 / 4.0) < 1e-5, diag


def test_restatement_keeps_transpose_separate(pkg):
    """A_hat^T comes from the transposed tables, not from val: with an asymmetric matrix the two differ."""
    ops = pkg.ops
    node_ptr = np.array([0, 3])
    entry_ptr = np.array([0, 3])
    adj = np.array([[0, 1], [0, 2], [2, 1]])
    w = np.array([0.5, 0.25, 2.0])
    tab = R.dataset_tables(ops, node_ptr, entry_ptr, adj, w)
    want = R.assemble(tab, np.zeros((3, 1), np.float32), np.zeros((1, 1), np.float32), None, [0], np.array([0]), 0, 1, 4)
    rp, col, val, rpt, colt, valt = ops.gcn_csr_host(adj, w, 3)
    for k, a in zip(R.GRAPH_KEYS, (rp, col, val, rpt, colt, valt)):
        R.assert_bits_equal(want[k], a, k)
    np.testing.assert_array_equal(want["col_t"], [0, 2, 0])
    np.testing.assert_array_equal(want["val_t"], np.float32([0.5, 2.0, 0.25]))


def test_pack_on_device_needs_a_gpu_device(pkg):
    raw = _dataset(pkg)
    with pytest.raises(ValueError, match="pack_on_device"):
        _model(pkg, raw, pack_on_device=True)
    m = _model(pkg, raw)                                                       # the default packs on the host, as before
    assert not m.params.get("pack_on_device", False)
    assert "adjacency_list" in next(iter(m.make_minibatch_iterator(m.valid_data, is_training=False)))


def _wrapper_args(pkg):
    m = _model(pkg, _dataset(pkg))
    data = m.train_data
    ms = data["molecules"]
    tab = _tables(pkg, data)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    G = ms.num_graphs
    order = np.arange(G)
    epoch_tab = np.concatenate([order, np.concatenate([[0], np.cumsum(tab["npg"])]), np.concatenate([[0], np.cumsum(tab["ne"])])])
    V, E = int(tab["npg"][:5].sum()), int(tab["ne"][:5].sum())
    return dict(node_ptr=t(ms.node_ptr, torch.int32), feat=t(ms.node_feat, torch.float32),
                csr=[t(tab["csr"][0], torch.int32), t(tab["csr"][1], torch.int32), t(tab["csr"][2], torch.float32)],
                csr_t=[t(tab["csr_t"][0], torch.int32), t(tab["csr_t"][1], torch.int32), t(tab["csr_t"][2], torch.float32)],
                targets=t(ms.targets, torch.float32), label_mask=t(data["label_mask"], torch.float32),
                task_ids=torch.tensor([0, 1], dtype=torch.int64), epoch_tab=t(epoch_tab, torch.int32),
                start=0, num_graphs=5, num_nodes=V, nnz=E, hidden_size=36)


def test_wrapper_rejects_bad_arguments_before_launch(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops._lib, "load", no_launch)
    good = _wrapper_args(pkg)
    bad = [
        ("node_ptr", good["node_ptr"].long(), TypeError),
        ("feat", good["feat"].double(), TypeError),
        ("csr", [good["csr"][0], good["csr"][1].long(), good["csr"][2]], TypeError),
        ("csr_t", [good["csr_t"][0], good["csr_t"][1], good["csr_t"][2].half()], TypeError),
        ("targets", good["targets"].double(), TypeError),
        ("label_mask", good["label_mask"].double(), TypeError),
        ("task_ids", good["task_ids"].int(), TypeError),
        ("epoch_tab", good["epoch_tab"].long(), TypeError),
        ("csr", [good["csr"][0][:-1], good["csr"][1], good["csr"][2]], ValueError),
        ("csr_t", [good["csr_t"][0], good["csr_t"][1][:-1], good["csr_t"][2]], ValueError),
        ("targets", good["targets"][:-1], ValueError),
        ("label_mask", good["label_mask"][:, :1].contiguous(), ValueError),
        ("epoch_tab", good["epoch_tab"][:-1], ValueError),
        ("start", len(good["node_ptr"]) - 3, ValueError),
        ("num_nodes", 10 ** 9, ValueError),
        ("nnz", -1, ValueError),
        ("hidden_size", 4, ValueError),
        ("feat", good["feat"].t(), ValueError),
    ]
    for key, value, exc in bad:
        with pytest.raises(exc):
            ops.gcn_assemble_batch(**dict(good, **{key: value}))
    with pytest.raises(TypeError, match="CUDA"):                 # a well-formed call on CPU tensors: refused, nothing launched
        ops.gcn_assemble_batch(**good)


def test_entry_point_validates_arguments(pkg):
    lib = pkg._lib.load()
    tabs = (ctypes.c_void_p * 10)(*([16] * 8 + [16, None]))     # (never dereferenced: every call below fails its argument checks)
    out = (ctypes.c_void_p * 12)(*([16] * 12))
    ep = ctypes.c_void_p(16)
    call = lambda **kw: lib.ggnn_gcn_assemble_batch(tabs, kw.get("Gd", 4), kw.get("A", 5), 2, ctypes.c_void_p(16), 2, kw.get("ep", ep),
                                                     kw.get("Ge", 4), kw.get("s", 0), kw.get("G", 2), kw.get("V", 10), kw.get("nnz", 30),
                                                     kw.get("D", 8), kw.get("out", out), None)
    assert call(s=3) != 0                                        # [3, 5) outside an epoch of 4 graphs
    assert call(D=4) != 0                                        # A = 5 > D
    assert call(D=0) != 0
    assert call(G=0) != 0                                        # an empty batch with nodes
    assert call(V=-1) != 0
    assert call(ep=None) != 0
    assert call(out=None) != 0
    assert call(V=1 << 30, D=8) != 0                             # V * D beyond 32-bit
    assert call(s=3) != 0 and b"outside" in lib.ggnn_last_error()
