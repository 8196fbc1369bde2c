"""SparseGCNChemModel on the GPU against the reference's own run (tests/golden/gcn_reference_*.npz): forward states,
per-graph outputs, loss and MAE after restoring a reference-schema checkpoint; the Adam trajectory of the reference's train
op; the whole 3-epoch train() log and best checkpoint.  Tolerances are test_gpu_reference_golden.py's."""
import json
import pickle

import numpy as np
import pytest
import torch

import gcn_golden as GG
import reference_golden as RG

pytestmark = pytest.mark.gpu
STATE_TOL = dict(rtol=1e-4, atol=1e-5)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _restored(pkg, g, tmp_path, cuda):
    m = pkg.SparseGCNChemModel(g.model_args(str(cuda), **{"--restore": g.write_checkpoint(str(tmp_path / "ref.pickle"))}))
    for n, t in m.named_variables().items():
        assert t.is_cuda
        np.testing.assert_array_equal(_np(t).reshape(g.weights[n].shape), g.weights[n])
    return m


@pytest.mark.parametrize("case", GG.CASES)
def test_forward_matches_reference_run(pkg, cuda, tmp_path, case):
    g = GG.GCNGolden(case)
    m = _restored(pkg, g, tmp_path, cuda)
    batches = list(m.make_minibatch_iterator(m.valid_data, False))
    assert len(batches) == int(g.z["num_valid_batches"])
    for k, b in enumerate(batches):
        GG.assert_feed_equal(b, g.feed("valid%d" % k))
        with torch.no_grad():
            loss = m.forward_batch(b)
        pre = "valid%d" % k
        np.testing.assert_allclose(_np(m.ops["final_node_representations"]), g.z[pre + "_final_node_representations"], **STATE_TOL)
        np.testing.assert_allclose(_np(m.output).reshape(-1), g.z[pre + "_output"], rtol=2e-4, atol=5e-5)
        np.testing.assert_allclose(float(loss), g.z[pre + "_loss"], rtol=5e-4)
        for i, t in enumerate(g.params["task_ids"]):
            np.testing.assert_allclose(float(m.ops["accuracy_task%d" % t]), g.z[pre + "_accuracy"][i], rtol=5e-4)


@pytest.mark.parametrize("case", GG.CASES)
def test_training_follows_reference_run(pkg, cuda, tmp_path, case):
    g = GG.GCNGolden(case)
    m = _restored(pkg, g, tmp_path, cuda)
    batches = list(m.make_minibatch_iterator(m.train_data, False))
    losses = []
    for s in range(len(g.z["train_losses"])):
        b = batches[s % len(batches)]
        GG.assert_feed_equal(b, g.feed("train%d" % s))
        losses.append(float(m.train_batch(b)))
    np.testing.assert_allclose(losses, g.z["train_losses"], rtol=5e-4)
    nv = m.named_variables()
    for i, n in enumerate(g.names):
        a = _np(nv[n])
        np.testing.assert_allclose(RG.stats(a), g.z["trained_stats"][i], rtol=1e-3, atol=5e-3, err_msg=n)
        if "trained/" + n in g.z.files:
            np.testing.assert_allclose(a.reshape(g.z["trained/" + n].shape), g.z["trained/" + n], rtol=1e-2, atol=3e-3, err_msg=n)


def test_train_loop_reproduces_reference_log(pkg, cuda, tmp_path):
    z = np.load(GG.path("loop"), allow_pickle=False)
    params = json.loads(str(z["params"]))
    m = pkg.SparseGCNChemModel({"--device": str(cuda), "--log_dir": str(tmp_path), "--config": json.dumps(params),
                                "train_data": json.loads(str(z["train_molecules"])),
                                "valid_data": json.loads(str(z["valid_molecules"]))})
    log = m.train()
    assert len(log) == len(z["train_loss"])
    np.testing.assert_allclose([e["train_results"][0] for e in log], z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][1] for e in log], z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][0] for e in log], z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][1] for e in log], z["valid_accuracy"], rtol=1e-3)
    with open(m.best_model_file, "rb") as f:
        best = pickle.load(f)
    assert best["params"] == params
    assert (best["train_step"], best["valid_step"]) == (int(z["best_train_step"]), int(z["best_valid_step"]))
    names = [str(n) for n in z["best_names"]]
    assert set(best["weights"]) - {"ggnn_amd/adam_step:0"} == set(names)
    for i, n in enumerate(names):
        a = np.asarray(best["weights"][n], dtype=np.float64)
        ref = z["best_stats"][i]
        np.testing.assert_allclose(RG.stats(a)[1:], ref[1:], rtol=2e-3, atol=1e-6, err_msg=n)
        assert abs(RG.stats(a)[0] - ref[0]) <= 2e-3 * max(ref[1], 1e-3), n


@pytest.mark.parametrize("case", ["bias_h64", "h48"])
def test_gradient_sink_equals_direct_gradients(pkg, cuda, tmp_path, case, monkeypatch):
    """One optimisation step with the weight gradients added into the optimiser's flat buffer on the side stream
    (backward.weight_gradient_sink) against the same step with the gradients returned through autograd."""
    g = GG.GCNGolden(case)
    after = []
    for use_sink in (True, False):
        monkeypatch.setattr(pkg.backward, "USE_WGRAD_STREAM", use_sink)
        m = _restored(pkg, g, tmp_path, cuda)
        b = list(m.make_minibatch_iterator(m.train_data, False))[0]
        used = []
        if use_sink:
            orig = pkg.backward._SINK.add
            monkeypatch.setattr(pkg.backward._SINK, "add", lambda p, t, v: (used.append(p), orig(p, t, v))[1])
        m.train_batch(b)
        if use_sink:
            graph_vars = m.graph_model_variables()
            assert {t.data_ptr() for t in graph_vars.values()} <= set(used)      # every W and b went through the sink
            monkeypatch.setattr(pkg.backward._SINK, "add", orig)
        after.append({n: _np(t).copy() for n, t in m.named_variables().items()})
    for n in after[0]:
        moved = np.abs(after[0][n] - g.weights[n].reshape(after[0][n].shape)).max()
        assert moved > 0, n
        np.testing.assert_allclose(after[0][n], after[1][n], rtol=0, atol=1e-7, err_msg=n)
