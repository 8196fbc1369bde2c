"""The GCN's host side against the reference's own run (tests/golden/gcn_reference_*.npz): the packer's lists and f32 weights
bit for bit, the training-set shuffle, the seeded initial values, the minibatch feeds.  No GPU needed."""
import json

import numpy as np
import pytest

import gcn_golden as GG
import reference_golden as RG


def _model(pkg, g):
    return pkg.SparseGCNChemModel(g.model_args("cpu"))


@pytest.mark.parametrize("case", GG.CASES)
def test_packer_and_shuffle_equal_reference(pkg, case):
    g = GG.GCNGolden(case)
    m = _model(pkg, g)
    d = m.train_data
    np.testing.assert_array_equal(np.diff(d["entry_ptr"]), g.z["train_entries_per_graph"])
    np.testing.assert_array_equal(d["adjacency_list"], g.z["train_adjacency_list"])
    np.testing.assert_array_equal(d["adjacency_weights"], g.z["train_adjacency_weights"])
    np.testing.assert_array_equal(d["adjacency_weights"].astype(np.float32), g.z["train_adjacency_weights"].astype(np.float32))


def test_packer_edge_cases_equal_reference(pkg):
    """Single atom, duplicate bond, self-bond (diagonal 2), no bonds: the reference's per-graph packer on each."""
    g = GG.GCNGolden("default")
    graphs = [(1, []), (3, [(0, 1, 1), (0, 2, 1), (1, 1, 0)]), (2, [(1, 1, 1), (0, 1, 1)]), (4, [])]
    raw = [{"targets": [[0.0]], "graph": [list(b) for b in bonds], "node_features": [[1, 0, 0, 0, 0]] * n} for n, bonds in graphs]
    entry_ptr, adj, w = pkg.gcn_model.gcn_adjacency(pkg.MoleculeSet.from_json(raw))
    for i in range(len(graphs)):
        e = slice(entry_ptr[i], entry_ptr[i + 1])
        np.testing.assert_array_equal(adj[e], g.z["edge%d_adjacency_list" % i])
        np.testing.assert_array_equal(w[e], g.z["edge%d_adjacency_weights" % i])


@pytest.mark.parametrize("case", GG.CASES)
def test_variables_and_init_equal_reference(pkg, case):
    g = GG.GCNGolden(case)
    m = _model(pkg, g)
    nv = m.named_variables()
    assert sorted(nv) == sorted(g.names)
    for i, n in enumerate(g.names):
        assert tuple(nv[n].shape) == g.shapes[i], n
        np.testing.assert_allclose(RG.stats(nv[n].numpy()), g.z["init_stats"][i], rtol=1e-6, atol=1e-9, err_msg=n)


@pytest.mark.parametrize("case", GG.CASES)
def test_minibatch_feeds_equal_reference(pkg, case):
    g = GG.GCNGolden(case)
    m = _model(pkg, g)
    batches = list(m.make_minibatch_iterator(m.valid_data, False))
    assert len(batches) == int(g.z["num_valid_batches"])
    for k, b in enumerate(batches):
        GG.assert_feed_equal(b, g.feed("valid%d" % k))
    train = list(m.make_minibatch_iterator(m.train_data, False))
    assert len(train) == int(g.z["num_train_batches"])
    for s in range(len(g.z["train_losses"])):
        GG.assert_feed_equal(train[s % len(train)], g.feed("train%d" % s))


def test_restore_reference_checkpoint(pkg, tmp_path):
    g = GG.GCNGolden("bias_h64")
    m = pkg.SparseGCNChemModel(g.model_args("cpu", **{"--restore": g.write_checkpoint(str(tmp_path / "ref.pickle"))}))
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.numpy().reshape(g.weights[n].shape), g.weights[n])
    assert json.loads(json.dumps(m.params)) == g.params
