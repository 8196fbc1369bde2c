"""Checkpoint interchange with the reference's own code (CPU; nothing here runs under `-m gpu`), against what the reference's
source did when it was run over the TF-1.3 op shim (tests/golden/checkpoint_interchange_*.npz, recorded by
tests/golden/make_reference_live_golden.py on this file's data and configs):

  * a checkpoint written by the package's save_progress is restorable BY THE REFERENCE (chem_tensorflow.py:330-359): it
    passes the params assertion of restore_progress and holds a value, of the variable's shape, for every global variable
    -- weights, Adam slots, beta powers -- that the reference's restore assigns by name;
  * a best-model pickle written by the reference's own train() is restored by the package: same weights, Adam state
    and step counters.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "golden", "reference_live.py")          # (runs the reference: used by the fixtures' generator only)

CONFIGS = {
    "sparse": {"layer_timesteps": [2, 1], "residual_connections": {"1": [0]}, "use_edge_bias": True, "batch_size": 150,
               "num_epochs": 1, "edge_weight_dropout_keep_prob": 1.0, "random_seed": 9, "hidden_size": 16},
    "dense": {"batch_size": 4, "num_epochs": 1, "random_seed": 9, "hidden_size": 16},
}


def _write_data(pkg, d, kind):
    train, valid = pkg.synthetic_qm9(30, mean_nodes=8, seed=31), pkg.synthetic_qm9(16, mean_nodes=8, seed=32)
    with open(os.path.join(d, "molecules_train.json"), "w") as f:
        f.write(json.dumps(train.to_json()))
    with open(os.path.join(d, "molecules_valid.json"), "w") as f:
        f.write(json.dumps(valid.to_json()))
    with open(os.path.join(d, "config.json"), "w") as f:
        f.write(json.dumps(CONFIGS[kind]))
    return str(d), train.to_json(), valid.to_json()


def _golden(kind):
    z = np.load(os.path.join(HERE, "golden", "checkpoint_interchange_%s.npz" % kind))
    blob = pickle.loads(z["best_pickle"].tobytes())
    return blob, z["best_pickle"].tobytes(), [str(n) for n in z["restore_names"]], json.loads(str(z["restore_shapes"]))


def _model(pkg, kind, train, valid, **extra):
    cls = pkg.SparseGGNNChemModel if kind == "sparse" else pkg.DenseGGNNChemModel
    args = {"--quiet": True, "--device": "cpu", "--config": json.dumps(CONFIGS[kind]), "train_data": train, "valid_data": valid}
    args.update(extra)
    return cls(args)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_reference_restores_package_checkpoint(pkg, tmp_path, kind):
    _, train, valid = _write_data(pkg, tmp_path, kind)
    m = _model(pkg, kind, train, valid)
    m.optimizer.apply_gradients([torch.randn_like(v) * 0.1 for v in m.trainable_variables.values()])   # non-trivial Adam state
    m.optimizer.apply_gradients([torch.randn_like(v) * 0.1 for v in m.trainable_variables.values()])
    ckpt = str(tmp_path / "pkg.pickle")
    m.save_progress(ckpt, 11, 5)
    data = pickle.load(open(ckpt, "rb"))
    ref_blob, _, names, shapes = _golden(kind)
    # restore_progress (chem_tensorflow.py:335-340): the same configuration, task_ids and num_epochs aside
    ref_params = ref_blob["params"]
    assert len(ref_params) == len(data["params"])
    for par, par_value in ref_params.items():
        if par not in ["task_ids", "num_epochs"]:
            assert par_value == data["params"][par], par
    assert (data["train_step"], data["valid_step"]) == (11, 5)
    saved = data["weights"]
    assert set(names) == set(saved) - {"ggnn_amd/adam_step:0"}          # the reference finds a value for EVERY variable
    for n, shape in zip(names, shapes):                                 # ... that its assign takes
        assert np.asarray(saved[n], dtype=np.float32).reshape(shape).shape == tuple(shape), n
    assert float(saved["beta1_power:0"]) == pytest.approx(0.9 ** 3) and float(saved["beta2_power:0"]) == pytest.approx(0.999 ** 3)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_package_restores_reference_checkpoint(pkg, tmp_path, kind):
    _, train, valid = _write_data(pkg, tmp_path, kind)
    blob, raw, _, _ = _golden(kind)
    best = tmp_path / "reference_model_best.pickle"
    best.write_bytes(raw)
    m = _model(pkg, kind, train, valid, **{"--restore": str(best)})
    assert (m.train_step_id, m.valid_step_id) == (blob["train_step"], blob["valid_step"])
    nv = m.named_variables()
    assert set(nv) | set(m.optimizer.state_variables(m.trainable_variables)) - {"ggnn_amd/adam_step:0"} == set(blob["weights"])
    for n, t in nv.items():
        np.testing.assert_array_equal(t.numpy().reshape(np.shape(blob["weights"][n])), blob["weights"][n], err_msg=n)
    state = m.optimizer.state_variables(m.trainable_variables)
    steps = blob["train_step"]
    assert m.optimizer.t == steps                                        # recovered from beta1_power
    for n, a in state.items():
        if n != "ggnn_amd/adam_step:0":
            np.testing.assert_allclose(a, blob["weights"][n], rtol=1e-6, err_msg=n)
