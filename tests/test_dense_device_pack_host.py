"""Dense device packer on the host: the NumPy restatement of "per-graph tables, then shift into the batch" (dense_device_pack_ref.py)
equals data.pack_dense_batch and an independent construction of the sparse form from A, bit for bit; the pack_on_device option
refuses a CPU device and stays out of default_params; the ops wrapper and the C entry point reject bad arguments before any launch.
No GPU needed."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import dense_device_pack_ref as R


def _dataset(pkg):
    """Synthetic molecules with four tasks plus the edge cases: a bondless graph, duplicate bonds (one also given in the other
    direction), a self-loop bond, and graphs of exactly 4, 12 and 29 atoms (n = v for those buckets)."""
    raw = pkg.synthetic_qm9(90, mean_nodes=9, seed=5, num_tasks=4).to_json()
    f = len(raw[0]["node_features"][0])
    one_hot = lambda n: [[0.0] * (f - 1) + [1.0]] * n
    chain = lambda n, t: [[i, 1 + (i + t) % 4, i + 1] for i in range(n - 1)]
    y = lambda a: [[a], [a + 1.0], [-a], [2.0 * a]]
    raw[3] = {"targets": y(0.5), "graph": [], "node_features": one_hot(2)}
    raw[7] = {"targets": y(1.5), "graph": [[0, 1, 1], [1, 2, 2], [0, 1, 1], [1, 1, 0]], "node_features": one_hot(3)}
    raw[8] = {"targets": y(-2.5), "graph": [[0, 2, 1], [2, 1, 2], [1, 3, 2]], "node_features": one_hot(3)}
    raw[9] = {"targets": y(3.0), "graph": chain(4, 0), "node_features": one_hot(4)}
    raw[10] = {"targets": y(4.0), "graph": chain(12, 1), "node_features": one_hot(12)}
    raw[11] = {"targets": y(5.0), "graph": chain(29, 2) + [[28, 4, 0]], "node_features": one_hot(29)}
    return raw


def _model(pkg, raw, device="cpu", **config):
    params = {"hidden_size": 32, "num_timesteps": 2, "random_seed": 3, "task_ids": [0, 3], "task_sample_ratios": {"3": 0.5},
              "batch_size": 8}
    params.update(config)
    return pkg.DenseGGNNChemModel({"--quiet": True, "--device": device, "train_data": raw, "valid_data": raw, "--config": params})


def _dd(pkg):
    return import_module(pkg.__name__ + ".data_device")


def _check_batch(pkg, ms, tab, ids, v, T, D, tie, task_ids, label_mask):
    db = pkg.data.pack_dense_batch(ms, ids, v, T, D, tie, task_ids, label_mask=label_mask)
    want = R.assemble(tab, ms.node_feat, ms.targets, label_mask, task_ids, ids, v, D)
    for key, name in R.DENSE_KEYS:
        R.assert_bits_equal(want[name], getattr(db, key), key)
    sf = R.sparse_form_from_dense(db.adjacency_matrix)
    for key in R.INDEX_KEYS + R.COMPACT_KEYS + ("nin",):
        R.assert_bits_equal(want[key], sf[key], key)
    assert want["type_off"] == sf["type_off"] and want["type_row_off"] == sf["type_row_off"]
    return want


@pytest.mark.parametrize("tie", [True, False])
def test_restatement_equals_host_packer_and_sparse_form(pkg, tie):
    ms = pkg.data.MoleculeSet.from_json(_dataset(pkg))
    F = ms.num_fwd_edge_types
    T = F if tie else 2 * F
    tab = _dd(pkg).dense_tables_host(ms, T, tie)
    n = ms.nodes_per_graph()
    rng = np.random.default_rng(7)
    mask = (rng.random((ms.num_graphs, 2)) < 0.7).astype(np.float32)
    special = [3, 7, 8, 9, 10, 11]
    seen_self_loop = seen_dup = False
    for v in (4, 12, 29):
        fit = np.nonzero(n <= v)[0]
        ids = np.concatenate([[g for g in special if n[g] <= v], rng.permutation(fit)[:9]]).astype(np.int64)
        assert (n[ids] == v).any()                                           # a graph that fills its bucket
        for D in (32, 50):
            want = _check_batch(pkg, ms, tab, ids, v, T, D, tie, (0, 3), mask)
        one = _check_batch(pkg, ms, tab, [3], v, T, 8, tie, (1,), None)      # a bondless graph alone: no message at all
        assert one["M"] == 0 and not one["A"].any()
        sl = _check_batch(pkg, ms, tab, [8], v, T, 8, tie, (0,), None)
        seen_self_loop |= sl["A"][0, 0, 2, 2] == 1.0 and int((sl["adj"][:, 0] == sl["adj"][:, 1]).sum()) == (1 if tie else 2)
        dup = _check_batch(pkg, ms, tab, [7], v, T, 8, tie, (0,), None)
        seen_dup |= dup["M"] == (4 if tie else 6)                            # (0,1,1) twice and (1,1,0): one pair of messages
    assert seen_self_loop and seen_dup


def test_model_buckets_and_custom_bucket_sizes(pkg):
    """Batches as the model forms them: its buckets and shuffled bucket lists, task_ids [0, 3] with the task_sample_ratios mask, and
    a custom bucket_sizes (process_raw_graphs' argument)."""
    m = _model(pkg, _dataset(pkg))
    data = m.train_data
    ms = data["molecules"]
    assert (data["label_mask"] == 0).any()
    T, tie = m.num_edge_types, m.params["tie_fwd_bkwd"]
    tab = _dd(pkg).dense_tables_host(ms, T, tie)
    custom = m.process_raw_graphs(ms, True, bucket_sizes=np.array([5, 9, 30]))
    checked = set()
    for d in (data, custom):
        for bucket, graphs in d["bucketed"].items():
            v = int(d["bucket_sizes"][bucket])
            ids = np.asarray(graphs[:m.params["batch_size"]], np.int64)
            _check_batch(pkg, ms, tab, ids, v, T, 32, tie, m.params["task_ids"], d["label_mask"])
            checked.add(v)
    assert {4, 12, 29, 5, 9, 30} <= checked


def test_epoch_order_matches_the_iterator(pkg):
    """The epoch order the device path uploads is the concatenation of the host iterator's batches, in step order."""
    m = _model(pkg, _dataset(pkg), batch_size=4)
    data = m.train_data
    order, starts = m._epoch_order(data["bucketed"], data["bucket_at_step"])
    ids = []
    counters = {}
    for bucket in data["bucket_at_step"]:
        c = counters.get(bucket, 0)
        ids.append(list(data["bucketed"][bucket][c * 4:(c + 1) * 4]))
        counters[bucket] = c + 1
    assert [list(order[s:e]) for s, e in zip(starts[:-1], starts[1:])] == ids


def test_pack_on_device_needs_a_gpu_device(pkg):
    raw = _dataset(pkg)
    with pytest.raises(ValueError, match="pack_on_device"):
        _model(pkg, raw, pack_on_device=True)
    assert "pack_on_device" not in pkg.DenseGGNNChemModel.default_params()
    assert pkg.DenseGGNNChemModel.default_params() == dict(pkg.ChemModel.default_params(), batch_size=256,
                                                           graph_state_dropout_keep_prob=1., task_sample_ratios={},
                                                           use_edge_bias=True, edge_weight_dropout_keep_prob=1)
    m = _model(pkg, raw)                                                       # the default packs on the host, as before
    feed = next(iter(m.make_minibatch_iterator(m.valid_data, is_training=False)))
    assert "_sparse_form" not in feed and "adjacency_absmax" not in feed


def test_tables_reject_bad_input(pkg):
    dd = _dd(pkg)
    ms = pkg.data.MoleculeSet.from_json(_dataset(pkg))
    with pytest.raises(ValueError):
        dd.dense_tables_host(ms, 17, True)
    with pytest.raises(IndexError):
        dd.dense_tables_host(ms, 2, True)                                     # bond types up to 4 do not fit 2 tied types


def _wrapper_args(pkg, compact=True):
    ms = pkg.data.MoleculeSet.from_json(_dataset(pkg))
    tab = _dd(pkg).dense_tables_host(ms, 4, True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tables = {k: t(v) for k, v in tab.items() if k not in ("mc", "pc")}
    order = np.arange(ms.num_graphs)
    pre = np.concatenate([np.concatenate([[0], np.cumsum(row)]) for row in tab["counts_t"]])
    epoch_tab = t(np.concatenate([order, pre]).astype(np.int32))
    ids = order[:5]
    type_off, type_row_off = R.batch_offsets(tab, ids)
    return dict(tables=tables, feat=t(ms.node_feat.astype(np.float32)), targets=t(ms.targets.astype(np.float32)),
                label_mask=torch.ones((ms.num_graphs, 2)), task_ids=torch.tensor([0, 3], dtype=torch.int64), epoch_tab=epoch_tab,
                start=0, num_graphs=5, num_vertices=29, hidden_size=32, type_off=type_off, type_row_off=type_row_off, sparse=True,
                compact=compact)


def test_wrapper_rejects_bad_arguments_before_launch(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops._lib, "load", no_launch)
    good = _wrapper_args(pkg)
    tabs = good["tables"]
    with_table = lambda name, value: dict(tabs, **{name: value})
    bad = [
        ("tables", with_table("msg", tabs["msg"].long()), TypeError),
        ("tables", with_table("nin", tabs["nin"].double()), TypeError),
        ("tables", with_table("node_order", None), ValueError),
        ("tables", with_table("slot_msg", tabs["slot_msg"][:-1]), ValueError),
        ("tables", with_table("src_ptr", tabs["src_ptr"][:-1]), ValueError),
        ("tables", with_table("counts_t", torch.zeros((34, 3), dtype=torch.int32)), ValueError),      # T = 17
        ("feat", good["feat"].double(), TypeError),
        ("feat", good["feat"].t(), ValueError),
        ("targets", good["targets"][:-1], ValueError),
        ("label_mask", good["label_mask"][:, :1].contiguous(), ValueError),
        ("task_ids", good["task_ids"].int(), TypeError),
        ("epoch_tab", good["epoch_tab"].long(), TypeError),
        ("epoch_tab", good["epoch_tab"][:-1], ValueError),
        ("start", -1, ValueError),
        ("num_graphs", 10 ** 6, ValueError),
        ("num_vertices", 0, ValueError),
        ("num_vertices", 1 << 16, ValueError),                               # T v v beyond 32-bit
        ("hidden_size", 4, ValueError),                                      # below the annotation size
        ("type_off", good["type_off"][:-1], ValueError),
        ("type_off", [1] + good["type_off"][1:], ValueError),
        ("type_row_off", None, ValueError),
    ]
    for key, value, exc in bad:
        with pytest.raises(exc):
            ops.dense_assemble_batch(**dict(good, **{key: value}))
    with pytest.raises(ValueError):                                          # the compaction structures need the sparse form
        ops.dense_assemble_batch(**dict(good, sparse=False))
    with pytest.raises(TypeError, match="CUDA"):                             # a well-formed call on CPU tensors: refused, nothing launched
        ops.dense_assemble_batch(**good)
    with pytest.raises(TypeError, match="CUDA"):
        ops.dense_assemble_batch(**dict(good, sparse=False, compact=False))


def test_entry_point_validates_arguments(pkg):
    lib = pkg._lib.load()
    tabs = (ctypes.c_void_p * 18)(*([16] * 18))                             # (never dereferenced: every call below fails its checks)
    out = (ctypes.c_void_p * 20)(*([16] * 20))
    ep = ctypes.c_void_p(16)
    off = (ctypes.c_int64 * 17)(*([0] * 17))

    def call(**kw):
        return lib.ggnn_dense_assemble_batch(kw.get("tabs", tabs), kw.get("Gd", 4), 5, kw.get("T", 4), 2, ctypes.c_void_p(16), 2,
                                             kw.get("ep", ep), kw.get("Ge", 4), kw.get("s", 0), kw.get("G", 2), kw.get("v", 8),
                                             kw.get("D", 8), kw.get("M", 0), kw.get("R", 0), off, off, 1, kw.get("out", out), None)
    assert call(tabs=None) != 0                                             # null tables
    assert call(out=None) != 0
    assert call(ep=None) != 0
    assert call(G=-1) != 0 and call(Gd=-1) != 0 and call(M=-1) != 0          # negative sizes
    assert call(v=0) != 0                                                   # v < 1
    assert call(T=17) != 0 and call(T=0) != 0                               # T outside [1, 16]
    assert call(s=3) != 0                                                   # [3, 5) outside an epoch of 4 graphs
    assert call(D=4) != 0                                                   # annotation size 5 > D
    assert call(v=1 << 15, D=8) != 0                                        # T v v beyond 32-bit
    assert call(M=5) != 0                                                   # type_off does not add up to M
    nulls = (ctypes.c_void_p * 18)(*([16] * 4 + [None] * 14))
    assert call(tabs=nulls) != 0                                            # null message tables
    assert call(T=17) != 0 and b"num_edge_types" in lib.ggnn_last_error()
