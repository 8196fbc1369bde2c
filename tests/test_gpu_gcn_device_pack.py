"""GCN batches assembled on the GPU (pack_on_device, ggnn_gcn_assemble_batch) against the NumPy restatement and against the host
packer: the kernel's arrays bit for bit, the model's feeds field by field over two training epochs and the validation pass, a seeded
train() run (same log and weights as host packing, and the reference's golden log), and no host synchronisation while packing."""
import json

import numpy as np
import pytest
import torch

import gcn_device_pack_ref as R
import gcn_golden as GG
from test_gcn_device_pack_host import _dataset

pytestmark = pytest.mark.gpu


def _processed(pkg, ms, task_ids=(0,), ratios=None):
    """process_raw_graphs' arrays of a training set (shuffled, label mask) and its device copy with the GCN tables."""
    from importlib import import_module
    gm = import_module(pkg.__name__ + ".gcn_model")
    dd = import_module(pkg.__name__ + ".data_device")
    entry_ptr, adj, w = gm.gcn_adjacency(ms)
    K = len(task_ids)
    mask = np.ones((ms.num_graphs, K), np.float32)
    if ratios:
        mask[int(ms.num_graphs * ratios):, K - 1] = 0.0
    dms = dd.DeviceMoleculeSet(ms, "cuda:0", mask)
    return dms, dms.gcn_tables(entry_ptr, adj, w), R.dataset_tables(pkg.ops, ms.node_ptr, entry_ptr, adj, w), mask


def _assemble(pkg, dms, tab, order, ep, task_ids, s, e, host, D):
    V = int(host["npg"][order[s:e]].sum())
    E = int(host["ne"][order[s:e]].sum())
    graph, h0, gnl, gp, uid, tv, tm = pkg.ops.gcn_assemble_batch(
        tab["node_ptr"], dms.node_feat, tab["csr"], tab["csr_t"], dms.targets, dms.label_mask, dms.task_ids_dev(task_ids), ep, s, e - s,
        V, E, D)
    return graph, {"initial_node_representation": h0, "graph_nodes_list": gnl, "graph_ptr": gp, "node_uid": uid, "target_values": tv,
                   "target_mask": tm, "num_graphs": e - s}


@pytest.mark.parametrize("D,annotation", [(32, 5), (48, 5), (48, 47), (100, 5), (100, 13), (128, 5), (30, 7)])
def test_kernel_matches_restatement(pkg, cuda, D, annotation):
    ms = pkg.synthetic_qm9(300, mean_nodes=14, seed=D + annotation, num_tasks=3, annotation_size=annotation)
    task_ids = (2, 0)
    dms, tab, host, mask = _processed(pkg, ms, task_ids, ratios=0.6)
    rng = np.random.default_rng(D)
    order = rng.permutation(ms.num_graphs)
    order_dev = dms.upload_order(order)
    ep = pkg.ops.gcn_epoch_table(tab["counts_t"], order_dev)
    npg_o, ne_o = host["npg"][order], host["ne"][order]
    want_ep = np.concatenate([order, np.concatenate([[0], np.cumsum(npg_o)]), np.concatenate([[0], np.cumsum(ne_o)])]).astype(np.int32)
    R.assert_bits_equal(ep, want_ep, "epoch table")
    bounds = pkg.data.batch_boundaries(npg_o, 1000)
    slices = list(zip(bounds[:-1], bounds[1:])) + [(0, 1), (ms.num_graphs - 1, ms.num_graphs), (0, ms.num_graphs), (17, 17), (0, 0),
                                                   (ms.num_graphs, ms.num_graphs)]
    for s, e in slices:
        graph, feed = _assemble(pkg, dms, tab, order, ep, task_ids, s, e, host, D)
        want = R.assemble(host, ms.node_feat, ms.targets, mask, task_ids, order, s, e, D)
        R.assert_batch_equal(graph, feed, want)
        assert graph.num_nodes == want["V"] and graph.nnz == want["nnz"]
    torch.cuda.synchronize()


def test_kernel_full_size_batch(pkg, cuda):
    """A 100k-node batch built like tools/gcn_bench.py's (synthetic QM9, mean 18 atoms, batch_size 100000)."""
    ms = pkg.synthetic_qm9(5600, mean_nodes=18, seed=0)
    dms, tab, host, mask = _processed(pkg, ms)
    order = np.random.default_rng(0).permutation(ms.num_graphs)
    order_dev = dms.upload_order(order)
    ep = pkg.ops.gcn_epoch_table(tab["counts_t"], order_dev)
    bounds = pkg.data.batch_boundaries(host["npg"][order], 100000)
    s, e = bounds[0], bounds[1]
    graph, feed = _assemble(pkg, dms, tab, order, ep, (0,), s, e, host, 100)
    want = R.assemble(host, ms.node_feat, ms.targets, mask, (0,), order, s, e, 100)
    assert want["V"] > 95000 and want["nnz"] > 250000
    R.assert_batch_equal(graph, feed, want)


def _model(pkg, raw, on_device, **config):
    params = {"hidden_size": 36, "num_timesteps": 2, "random_seed": 3, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5},
              "batch_size": 120, "graph_state_dropout_keep_prob": 0.75, "pack_on_device": on_device}
    params.update(config)
    return pkg.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "train_data": raw, "valid_data": raw, "--config": params})


def _feeds(m):
    out = []
    for _ in range(2):
        out.append(list(m.make_minibatch_iterator(m.train_data, is_training=True)))
    out.append(list(m.make_minibatch_iterator(m.valid_data, is_training=False)))
    out.append(list(m.make_minibatch_iterator(m.valid_data, is_training=False)))     # (resident: the same batches again)
    return out


def test_model_feeds_equal_host_feeds(pkg, cuda):
    raw = _dataset(pkg)
    host = _feeds(_model(pkg, raw, False))            # (each model reseeds NumPy: the two runs draw the same epoch orders)
    dev = _feeds(_model(pkg, raw, True))
    assert [len(p) for p in dev] == [len(p) for p in host] and len(host[0]) > 2
    for part_h, part_d in zip(host, dev):
        for fh, fd in zip(part_h, part_d):
            assert "adjacency_list" not in fd and "adjacency_weights" not in fd
            assert set(fd) == set(fh) - {"adjacency_list", "adjacency_weights"}
            for key in R.GRAPH_KEYS:
                R.assert_bits_equal(getattr(fd["gcn_graph"], key), getattr(fh["gcn_graph"], key), key)
            assert fd["gcn_graph"].num_nodes == fh["gcn_graph"].num_nodes and fd["gcn_graph"].nnz == fh["gcn_graph"].nnz
            for key in fh:
                if key in ("adjacency_list", "adjacency_weights", "gcn_graph"):
                    continue
                if isinstance(fh[key], torch.Tensor):
                    assert fd[key].is_cuda
                    R.assert_bits_equal(fd[key], fh[key], key)
                else:
                    assert fd[key] == fh[key], key
    assert dev[0][0]["graph_state_keep_prob"] == 0.75 and dev[2][0]["graph_state_keep_prob"] == 1.0
    assert dev[2][0]["gcn_graph"] is dev[3][0]["gcn_graph"]


def _golden_loop_model(pkg, tmp_path, on_device):
    z = np.load(GG.path("loop"), allow_pickle=False)
    params = dict(json.loads(str(z["params"])), pack_on_device=on_device)
    m = pkg.SparseGCNChemModel({"--quiet": True, "--device": "cuda:0", "--log_dir": str(tmp_path / str(on_device)),
                                "--config": json.dumps(params), "train_data": json.loads(str(z["train_molecules"])),
                                "valid_data": json.loads(str(z["valid_molecules"]))})
    return m, z


def test_training_matches_host_packing_and_reference_log(pkg, cuda, tmp_path):
    runs = {}
    for on_device in (False, True):
        m, z = _golden_loop_model(pkg, tmp_path, on_device)
        log = m.train()
        runs[on_device] = ([(e["train_results"][:2], e["valid_results"][:2]) for e in log],
                           {n: t.detach().cpu().numpy().copy() for n, t in m.named_variables().items()})
    (log_h, w_h), (log_d, w_d) = runs[False], runs[True]
    assert len(log_d) == len(z["train_loss"]) == len(log_h)
    for (th, vh), (td, vd) in zip(log_h, log_d):
        assert float(th[0]) == float(td[0]) and float(vh[0]) == float(vd[0])
        np.testing.assert_array_equal(np.asarray(th[1]), np.asarray(td[1]))
        np.testing.assert_array_equal(np.asarray(vh[1]), np.asarray(vd[1]))
    assert set(w_h) == set(w_d)
    for n in w_h:
        assert w_h[n].tobytes() == w_d[n].tobytes(), n
    # the reference's own run, at test_gpu_gcn_reference_golden.py's tolerances
    np.testing.assert_allclose([t[0] for t, _ in log_d], z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([t[1] for t, _ in log_d], z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([v[0] for _, v in log_d], z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([v[1] for _, v in log_d], z["valid_accuracy"], rtol=1e-3)


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


def test_packing_does_not_synchronise(pkg, cuda):
    m = _model(pkg, _dataset(pkg), True, batch_size=40)
    m.prepare_resident_data(m.train_data, True)
    for _ in m.make_minibatch_iterator(m.train_data, is_training=True):     # (first epoch: the order's staging buffer is allocated)
        pass
    torch.cuda.synchronize()
    it = m.make_minibatch_iterator(m.train_data, is_training=True)
    first = next(it)                  # the epoch start: one upload of the order through the pinned buffer on its own stream
    batches = [first]
    if _sync_debug_honoured():
        torch.cuda.set_sync_debug_mode("error")
        try:
            batches += list(it)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            batches += list(it)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()]
        assert not [n for n in names if "DtoH" in n or "DeviceToHost" in n], names
    assert len(batches) > 3
    torch.cuda.synchronize()
