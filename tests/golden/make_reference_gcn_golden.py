"""Generates tests/golden/gcn_reference_*.npz by RUNNING THE REFERENCE'S OWN GCN SOURCE (chem_tensorflow_gcn.py with
chem_tensorflow.py and utils.py, imported from where they lie, unmodified) over the TF-1.3 op shim in oracle/tf13_shim,
the way make_reference_golden.py does for the GGNN models.

The shim has no sparse tensors.  This script adds tf.SparseTensor and tf.sparse_tensor_dense_matmul to the imported shim
module at run time (nothing under oracle/ changes), written from TF-1.3's documented semantics: float32, every output row
accumulated in the order of the nonzeros (SparseTensorDenseMatMul's CPU kernel: out[i, :] += a_value * b[j, :] per nonzero).

    python tests/golden/make_reference_gcn_golden.py          # only works where /root/reference exists

The files are named gcn_reference_* (not reference_*) so that the GGNN fixture loader's reference_*.npz glob does not
take them for GGNN cases.  As for the GGNN fixtures, the variables are overwritten by golden_weights() after construction
and the reference's own initial values are kept as checksums (init_stats).
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"

_spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(HERE, "make_reference_golden.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
golden_weights, stats, WEIGHT_SEED = _gen.golden_weights, _gen.stats, _gen.WEIGHT_SEED

CASES = {
    # name: (params, Adam steps recorded)
    "default": ({"batch_size": 250, "random_seed": 0}, 2),                                   # 4 layers, h = 100, no bias
    "bias_h64": ({"gcn_use_bias": True, "hidden_size": 64, "num_timesteps": 2, "batch_size": 250, "random_seed": 1}, 3),
    "multitask": ({"task_ids": [0, 1], "task_sample_ratios": {"1": 0.5}, "batch_size": 150, "random_seed": 2}, 2),
    "h48": ({"hidden_size": 48, "gcn_use_bias": True, "batch_size": 250, "random_seed": 3}, 2),   # composed path
}
EDGE_GRAPHS = [(1, []), (3, [(0, 1, 1), (0, 2, 1), (1, 1, 0)]), (2, [(1, 1, 1), (0, 1, 1)]), (4, [])]
LOOP_PARAMS = {"batch_size": 100, "num_epochs": 3, "random_seed": 4, "hidden_size": 64}


def patch_sparse(tf):
    """tf.SparseTensor / tf.sparse_tensor_dense_matmul for the shim (float32; row i of the product accumulates the nonzeros
    of row i in their order).  Differentiable in the dense operand through torch, like every shim op."""
    import torch

    class SparseTensor:
        def __init__(self, indices, values, dense_shape):
            self.indices, self.values, self.dense_shape = indices, values, dense_shape

    def sparse_tensor_dense_matmul(sp_a, b, name=None):
        def run(idx, vals, shape, dense):
            rows, cols = idx[:, 0].long(), idx[:, 1].long()
            n = int(shape[0])
            out = torch.zeros((n, dense.shape[1]), dtype=dense.dtype)
            if rows.numel() == 0:
                return out
            # occurrence rank of each nonzero inside its row: round r adds the r-th nonzero of every row (rows are distinct
            # inside a round), so each row sums its nonzeros in their order
            order = torch.argsort(rows, stable=True)
            first = torch.zeros(n + 1, dtype=torch.long)
            first[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
            rank = torch.empty_like(rows)
            rank[order] = torch.arange(rows.numel()) - first[rows[order]]
            for r in range(int(rank.max()) + 1):
                k = torch.nonzero(rank == r).reshape(-1)
                out = out.index_add(0, rows[k], vals[k, None].to(dense.dtype) * dense[cols[k]])
            return out
        return tf.Tensor(run, (sp_a.indices, sp_a.values, list(sp_a.dense_shape), b), op="SparseTensorDenseMatMul")

    tf.SparseTensor = SparseTensor
    tf.sparse_tensor_dense_matmul = sparse_tensor_dense_matmul


def write_data(pkg, tmp, train, valid, num_tasks):
    train_ms = pkg.synthetic_qm9(train[0], mean_nodes=train[1], seed=train[2], num_tasks=num_tasks)
    valid_ms = pkg.synthetic_qm9(valid[0], mean_nodes=valid[1], seed=valid[2], num_tasks=num_tasks)
    for fn, ms in (("molecules_train.json", train_ms), ("molecules_valid.json", valid_ms)):
        with open(os.path.join(tmp, fn), "w") as f:
            json.dump(ms.to_json(), f)
    return train_ms, valid_ms


def run_case(name, params, train_steps, pkg, tf, Model):
    tmp = tempfile.mkdtemp(prefix="gcn_ref_")
    num_tasks = max(params.get("task_ids", [0])) + 1
    train_ms, valid_ms = write_data(pkg, tmp, (40, 9, 11), (24, 9, 12), num_tasks)
    model = Model({"--data_dir": tmp, "--log_dir": tmp, "--config": json.dumps(params)})
    g = model.sess.graph
    trainable = g.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES)
    out = {"params": np.array(json.dumps(model.params)), "weight_seed": WEIGHT_SEED,
           "train_molecules": np.array(json.dumps(train_ms.to_json())),
           "valid_molecules": np.array(json.dumps(valid_ms.to_json())),
           "trainable_names": np.array([v.name for v in trainable]),
           "trainable_shapes": np.array([json.dumps(list(v.value.shape)) for v in trainable])}
    out["init_stats"] = np.stack([stats(model.sess.run(v)) for v in trainable])
    # the packer's lists per graph of the training set, in the order process_raw_graphs left it (after its shuffle)
    out["train_adjacency_list"] = np.concatenate([np.asarray(d["adjacency_list"]).reshape(-1, 2) for d in model.train_data])
    out["train_adjacency_weights"] = np.concatenate([np.asarray(d["adjacency_weights"], np.float64) for d in model.train_data])
    out["train_entries_per_graph"] = np.array([len(d["adjacency_weights"]) for d in model.train_data])
    # the reference's per-graph packer on edge cases: a single atom, a duplicate bond, a self-bond, a graph without bonds
    for i, (n, bonds) in enumerate(EDGE_GRAPHS):
        adj, w = model._SparseGCNChemModel__graph_to_adjacency_list(bonds, n)
        out["edge%d_adjacency_list" % i] = np.asarray(adj).reshape(-1, 2)
        out["edge%d_adjacency_weights" % i] = np.asarray(w, np.float64)
    model.sess.run([v.assign(golden_weights(v.name, v.value.shape, WEIGHT_SEED)) for v in trainable])

    ph = model.placeholders
    # (the GCN's gated_regression keeps no handle on the per-graph outputs: the reference's own method is applied once more to
    # the final states with the LAST task's readout weights -- the same ops make_model built last, what the GGNN models keep
    # as `output`)
    last = model.params["task_ids"][-1]
    output = model.gated_regression(model.ops["final_node_representations"], model.weights["regression_gate_task%d" % last],
                                    model.weights["regression_transform_task%d" % last])
    fetch = [model.ops["final_node_representations"], output, model.ops["loss"]] + \
            [model.ops["accuracy_task%d" % t] for t in model.params["task_ids"]]

    def record(prefix, feed):
        feed[ph["out_layer_dropout_keep_prob"]] = 1.0
        for key, p in ph.items():
            if p in feed:
                out["%s_feed_%s" % (prefix, key)] = np.asarray(feed[p])
        return feed

    nb = 0
    for nb, feed in enumerate(model.make_minibatch_iterator(model.valid_data, False)):
        record("valid%d" % nb, feed)
        h, per_graph, loss, *mae = model.sess.run(fetch, feed_dict=feed)
        out["valid%d_final_node_representations" % nb] = h
        out["valid%d_output" % nb] = np.atleast_1d(per_graph)
        out["valid%d_loss" % nb] = loss
        out["valid%d_accuracy" % nb] = np.array(mae)
    out["num_valid_batches"] = nb + 1

    batches = list(model.make_minibatch_iterator(model.train_data, False))
    losses = []
    for s in range(train_steps):
        feed = record("train%d" % s, batches[s % len(batches)])
        loss, _ = model.sess.run([model.ops["loss"], model.ops["train_step"]], feed_dict=feed)
        losses.append(loss)
    out["train_losses"] = np.array(losses)
    out["num_train_batches"] = len(batches)
    final = [model.sess.run(v) for v in trainable]
    out["trained_stats"] = np.stack([stats(a) for a in final])
    for v, a in zip(trainable, final):
        if a.size <= 400:
            out["trained/" + v.name] = a
    np.savez_compressed(os.path.join(HERE, "gcn_reference_%s.npz" % name), **out)
    print("%-10s %d valid batches, %d variables, loss %.6f" % (name, nb + 1, len(trainable), out["valid0_loss"]))


def run_loop(pkg, tf, Model):
    import pickle
    import types
    tmp = tempfile.mkdtemp(prefix="gcn_ref_")
    train_ms, valid_ms = write_data(pkg, tmp, (60, 9, 21), (24, 9, 22), 1)
    model = Model({"--data_dir": tmp, "--log_dir": tmp, "--config": json.dumps(LOOP_PARAMS)})
    import chem_tensorflow                      # (json that writes numpy scalars: see make_reference_golden.run_loop_case)
    chem_tensorflow.json = types.SimpleNamespace(
        dump=lambda o, f, **kw: json.dump(o, f, default=float, **kw), dumps=json.dumps, load=json.load, loads=json.loads)
    model.train()
    with open(model.log_file) as f:
        log = json.load(f)
    with open(model.best_model_file, "rb") as f:
        best = pickle.load(f)
    names = sorted(best["weights"])
    out = {"params": np.array(json.dumps(model.params)),
           "train_molecules": np.array(json.dumps(train_ms.to_json())),
           "valid_molecules": np.array(json.dumps(valid_ms.to_json())),
           "train_loss": np.array([e["train_results"][0] for e in log]),
           "train_accuracy": np.array([e["train_results"][1] for e in log]),
           "valid_loss": np.array([e["valid_results"][0] for e in log]),
           "valid_accuracy": np.array([e["valid_results"][1] for e in log]),
           "best_train_step": best["train_step"], "best_valid_step": best["valid_step"],
           "best_names": np.array(names), "best_stats": np.stack([stats(best["weights"][n]) for n in names])}
    np.savez_compressed(os.path.join(HERE, "gcn_reference_loop.npz"), **out)
    print("loop       %d epochs, train loss %s, valid loss %s" % (len(log), out["train_loss"], out["valid_loss"]))


def main():
    import importlib
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("gated-graph-neural-network-samples_amd")     # only its synthetic molecule generator
    sys.path[:0] = [os.path.join(ROOT, "oracle", "tf13_shim"), REFERENCE]
    import tensorflow as tf
    assert tf.__version__.endswith("shim")
    patch_sparse(tf)
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp(prefix="gcn_ref_cwd_"))
    try:
        from chem_tensorflow_gcn import SparseGCNChemModel
        only = sys.argv[1:]
        for name, (params, steps) in CASES.items():
            if not only or name in only:
                run_case(name, params, steps, pkg, tf, SparseGCNChemModel)
        if not only or "loop" in only:
            run_loop(pkg, tf, SparseGCNChemModel)
    finally:
        os.chdir(cwd)


if __name__ == "__main__":
    main()
