"""Dense GGNN batches assembled on the GPU (pack_on_device, ggnn_dense_assemble_batch) against the NumPy restatement and against the
host path: the kernel's arrays bit for bit, a full-size batch against what the training step builds from A, the model's feeds over
two training epochs and the validation pass, a seeded train() run (same log and checkpoint as host packing, and the reference's
golden log), and no host synchronisation while packing, in the training-mode propagation or in its backward."""
import json
import pickle
from importlib import import_module

import numpy as np
import pytest
import torch

import dense_device_pack_ref as R
import reference_golden as RG
from test_dense_device_pack_host import _dataset

pytestmark = pytest.mark.gpu


def _dd(pkg):
    return import_module(pkg.__name__ + ".data_device")


def _device_batch(pkg, dms, tab, ep, order, s, G, v, D, task_ids, sparse, compact):
    type_off, type_row_off = R.batch_offsets(tab, order[s:s + G])
    return pkg.ops.dense_assemble_batch(tab, dms.node_feat, dms.targets, dms.label_mask, dms.task_ids_dev(task_ids), ep, s, G, v, D,
                                        type_off, type_row_off if compact else None, sparse=sparse, compact=compact)


def _check(out, want, sparse, compact):
    for key, name in R.DENSE_KEYS:
        R.assert_bits_equal(out[key], want[name], key)
    if not sparse:
        assert "index" not in out
        return
    assert out["index"].type_off == want["type_off"] and out["index"].num_nodes == want["h0"].shape[0] * want["h0"].shape[1]
    got = R.device_sparse_arrays(out["index"], out["nin"], compact)
    for key in R.INDEX_KEYS + ("nin",) + (R.COMPACT_KEYS if compact else ()):
        R.assert_bits_equal(got[key], want[key], key)
    if compact:
        assert out["index"]._compact.type_row_off == want["type_row_off"]


@pytest.mark.parametrize("D", [32, 100, 50])
@pytest.mark.parametrize("tie", [True, False])
def test_kernel_matches_restatement(pkg, cuda, D, tie):
    ms = pkg.data.MoleculeSet.from_json(_dataset(pkg))
    F = ms.num_fwd_edge_types
    T = F if tie else 2 * F
    rng = np.random.default_rng(D + tie)
    mask = (rng.random((ms.num_graphs, 2)) < 0.7).astype(np.float32)
    dms = _dd(pkg).DeviceMoleculeSet(ms, "cuda:0", mask)
    tab = dms.dense_tables(T, tie)
    host = _dd(pkg).dense_tables_host(ms, T, tie)
    n = ms.nodes_per_graph()
    for v in (4, 12, 29, 7):
        fit = np.nonzero(n <= v)[0]
        order = np.concatenate([rng.permutation(fit), [g for g in (3, 7, 8, 9) if n[g] <= v]]).astype(np.int64)
        ep = pkg.ops.dense_epoch_table(tab["counts_t"], dms.upload_order(order))
        Ge = len(order)
        for s, G in ((0, min(Ge, 8)), (3, Ge - 3), (Ge - 1, 1), (max(Ge - 5, 0), min(Ge, 5))):
            want = R.assemble(host, ms.node_feat, ms.targets, mask, (0, 3), order[s:s + G], v, D)
            for sparse, compact in ((False, False), (True, False), (True, True)):
                _check(_device_batch(pkg, dms, tab, ep, order, s, G, v, D, (0, 3), sparse, compact), want, sparse, compact)
    torch.cuda.synchronize()


def test_full_size_batch_equals_host_path(pkg, cuda):
    """256 graphs of v = 29, D = 100, from 20 000 synthetic molecules: every field equals the host path's, the sparse form equals
    what _compute_for_training builds from A.nonzero() with ops.build_message_index / build_compact_sources / compact_backward."""
    ms = pkg.synthetic_qm9(20000, mean_nodes=18, seed=0)
    T, D, v = 4, 100, 29
    dms = _dd(pkg).DeviceMoleculeSet(ms, "cuda:0", None)
    tab = dms.dense_tables(T, True)
    order = np.random.default_rng(0).permutation(ms.num_graphs)
    ep = pkg.ops.dense_epoch_table(tab["counts_t"], dms.upload_order(order))
    s = 2560
    out = _device_batch(pkg, dms, tab, ep, order, s, 256, v, D, (0,), True, True)
    db = pkg.data.pack_dense_batch(ms, order[s:s + 256], v, T, D, True, (0,))
    for key, _ in R.DENSE_KEYS:
        R.assert_bits_equal(out[key], getattr(db, key), key)
    A = torch.from_numpy(db.adjacency_matrix).to("cuda:0")
    ops = pkg.ops
    nz = A.nonzero()                                                    # exactly DenseGGNNChemModel._compute_for_training's derivation
    base = nz[:, 0] * v
    pairs = torch.stack([base + nz[:, 3], base + nz[:, 2]], dim=1).to(torch.int32)
    lists = [pairs[nz[:, 1] == t].contiguous() for t in range(T)]
    nin = A.sum(dim=3).permute(0, 2, 1).reshape(256 * v, T).to(torch.float32).contiguous()
    index = ops.build_message_index(lists, 256 * v)
    comp = index._compact = ops.build_compact_sources(index)
    ops.compact_backward(index, comp)
    want = {k: R.as_np(t) for k, t in R.device_sparse_arrays(index, nin, True).items()}
    got = R.device_sparse_arrays(out["index"], out["nin"], True)
    assert out["index"].type_off == index.type_off and out["index"]._compact.type_row_off == comp.type_row_off
    assert index.num_messages > 8000 and comp.num_rows > 4000
    for key in want:
        R.assert_bits_equal(got[key], want[key], key)
    sn_d, sn_h = out["index"]._compact._bwd.source_node_index, comp._bwd.source_node_index
    R.assert_bits_equal(sn_d.row_ptr, sn_h.row_ptr, "source_node_index.row_ptr")
    R.assert_bits_equal(out["index"]._compact._bwd.identity.pair_node, comp._bwd.identity.pair_node, "identity")


def _model(pkg, raw, on_device, **config):
    params = {"hidden_size": 32, "num_timesteps": 2, "random_seed": 3, "task_ids": [0, 3], "task_sample_ratios": {"3": 0.5},
              "batch_size": 4, "pack_on_device": on_device}
    params.update(config)
    return pkg.DenseGGNNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": raw, "valid_data": raw, "--config": params})


def _feeds(m):
    out = []
    for _ in range(2):
        out.append(list(m.make_minibatch_iterator(m.train_data, is_training=True)))
    out.append(list(m.make_minibatch_iterator(m.valid_data, is_training=False)))
    out.append(list(m.make_minibatch_iterator(m.valid_data, is_training=False)))     # (resident: the same batches again)
    return out


def test_model_feeds_equal_host_feeds(pkg, cuda):
    raw = _dataset(pkg)
    host = _feeds(_model(pkg, raw, False))            # (each model reseeds NumPy: the two runs draw the same shuffles)
    dev = _feeds(_model(pkg, raw, True))
    assert [len(p) for p in dev] == [len(p) for p in host] and len(host[0]) > 4
    for i, (part_h, part_d) in enumerate(zip(host, dev)):
        for fh, fd in zip(part_h, part_d):
            assert set(fh) <= set(fd)
            for key in fh:
                if isinstance(fh[key], torch.Tensor):
                    assert fd[key].is_cuda
                    R.assert_bits_equal(fd[key], fh[key], key)
                else:
                    assert fd[key] == fh[key], key
            if i < 2:                                 # training feeds carry the sparse form of their own A
                A, index, nin = fd["_sparse_form"]
                assert A is fd["adjacency_matrix"]
                want = R.sparse_form_from_dense(R.as_np(A))
                R.assert_bits_equal(nin, want["nin"], "nin")
                for key in R.INDEX_KEYS:
                    R.assert_bits_equal(getattr(index, key), want[key], key)
            else:
                assert "_sparse_form" not in fd
            assert fd["adjacency_absmax"] == (1.0 if R.as_np(fd["adjacency_matrix"]).any() else 0.0)
    assert dev[0][0]["graph_state_keep_prob"] == 1.0 and dev[2][0]["adjacency_matrix"] is dev[3][0]["adjacency_matrix"]


def test_training_matches_host_packing_and_reference_log(pkg, cuda, tmp_path):
    g = RG.GoldenLoop("loop_dense")
    runs = {}
    for on_device in (False, True):
        params = dict(g.params, pack_on_device=on_device)
        m = pkg.DenseGGNNChemModel({"--device": str(cuda), "--log_dir": str(tmp_path / str(on_device)), "--config": json.dumps(params),
                                    "train_data": g.train_molecules, "valid_data": g.valid_molecules})
        log = m.train()
        with open(m.best_model_file, "rb") as f:
            runs[on_device] = (log, pickle.load(f))
    (log_h, best_h), (log_d, best_d) = runs[False], runs[True]
    assert len(log_d) == len(log_h) == len(g.z["train_loss"])
    for eh, ed in zip(log_h, log_d):
        for part in ("train_results", "valid_results"):
            assert float(eh[part][0]) == float(ed[part][0]), part
            np.testing.assert_array_equal(np.asarray(eh[part][1]), np.asarray(ed[part][1]))
            np.testing.assert_array_equal(np.asarray(eh[part][2]), np.asarray(ed[part][2]))
    assert set(best_h["weights"]) == set(best_d["weights"])
    for n in best_h["weights"]:
        assert np.asarray(best_h["weights"][n]).tobytes() == np.asarray(best_d["weights"][n]).tobytes(), n
    assert {k: v for k, v in best_d["params"].items() if k != "pack_on_device"} == g.params
    # the reference's own run, at test_train_loop_reproduces_reference_log's tolerances
    np.testing.assert_allclose([e["train_results"][0] for e in log_d], g.z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][1] for e in log_d], g.z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][2] for e in log_d], g.z["train_error_ratio"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][0] for e in log_d], g.z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][1] for e in log_d], g.z["valid_accuracy"], rtol=1e-3)
    assert (best_d["train_step"], best_d["valid_step"]) == (int(g.z["best_train_step"]), int(g.z["best_valid_step"]))
    for i, n in enumerate(g.best_names):
        a = np.asarray(best_d["weights"][n], dtype=np.float64)
        ref = g.z["best_stats"][i]
        np.testing.assert_allclose(RG.stats(a)[1:], ref[1:], rtol=2e-3, atol=1e-6, err_msg=n)
        assert abs(RG.stats(a)[0] - ref[0]) <= 2e-3 * max(ref[1], 1e-3), n


def _sync_debug_honoured() -> bool:
    x = torch.ones(1, device="cuda:0")
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


def _forward_backward(m, feed):
    """The training-mode propagation of a packed batch (_compute_for_training) and the backward of its output."""
    variables = list(m.trainable_variables.values())
    for t in variables:
        t.requires_grad_(True)
        t.grad = None
    try:
        m.feed(dict(feed, out_layer_dropout_keep_prob=1.0))
        m.training = True
        h = m._compute_for_training()
        h.sum().backward()
    finally:
        m.training = False
        for t in variables:
            t.requires_grad_(False)
            t.grad = None
    return h


@pytest.mark.parametrize("D", [100, 128])       # (the training step with and without the compacted transform)
def test_packing_and_training_propagation_do_not_synchronise(pkg, cuda, D):
    if not _sync_debug_honoured():
        pytest.skip("torch.cuda.set_sync_debug_mode is not honoured by this build")
    m = _model(pkg, _dataset(pkg), True, hidden_size=D)
    m.prepare_resident_data(m.train_data, True)
    warm = list(m.make_minibatch_iterator(m.train_data, is_training=True))   # (first epoch: staging buffer, weight images)
    _forward_backward(m, warm[0])
    torch.cuda.synchronize()
    it = m.make_minibatch_iterator(m.train_data, is_training=True)
    first = next(it)                  # the epoch start: one upload of the order through the pinned buffer on its own stream
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [first] + list(it)
        h = _forward_backward(m, batches[1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(batches) > 3 and torch.isfinite(h).all()
    torch.cuda.synchronize()
