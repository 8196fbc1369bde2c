"""params['multitask_readout'] on the three models: three train_batch steps from the same weights with and without the key -- losses,
step-1 gradients of every variable (both routes against float64 at the project's gradient bound, 2e-4 of the gradient's largest
entry), no per-task readout call under the key, the per-task entries of model.ops -- on the autograd routes and on the native steps;
read-out weight dropout; a validation forward_batch."""
import json

import numpy as np
import pytest
import torch

import gcn_train_reference as GR
import test_gpu_dense_train as DT
import test_gpu_gcn_native as GN
import train_reference as TR

pytestmark = pytest.mark.gpu
KEY = "multitask_readout"
TASKS = {"task_ids": [0, 1, 2], "task_sample_ratios": {"1": 0.5}}


@pytest.fixture(scope="module")
def molecules(pkg):
    return pkg.synthetic_qm9(300, mean_nodes=10, num_tasks=3)


def _config(kind, hidden, native, multi):
    cfg = dict(TASKS, hidden_size=hidden, random_seed=3, batch_size={"sparse": 1200, "dense": 16, "gcn": 1200}[kind])
    if kind == "dense" and native:
        cfg["graph_resident_training"] = "native"
    if kind == "gcn":
        cfg["gcn_use_bias"] = True
        if native:
            cfg["native_training"] = True
    if multi:
        cfg[KEY] = True
    return cfg


def _model(pkg, oracle, cuda, ms, kind, hidden, native, multi):
    cls = {"sparse": pkg.SparseGGNNChemModel, "dense": pkg.DenseGGNNChemModel, "gcn": pkg.SparseGCNChemModel}[kind]
    m = cls({"--quiet": True, "--device": str(cuda), "train_data": ms, "valid_data": ms,
             "--config": json.dumps(_config(kind, hidden, native, multi))})
    if kind == "sparse":
        m._test_layers = oracle.make_sparse_layers(np.random.default_rng(4), m.params, m.num_edge_types, random_bias=True)
        m.set_graph_weights(m._test_layers)
    elif kind == "dense":
        DT._randomise(m, oracle)
    else:
        GN._randomise(m)
    rng = np.random.default_rng(9)                                # non-zero read-out biases (the fresh model's are zero)
    with torch.no_grad():
        for n, t in m.named_variables().items():
            if n.startswith("out_layer_task") and "MLP_b_" in n:
                t.copy_(torch.from_numpy(rng.normal(0, 0.1, tuple(t.shape)).astype(np.float32)).to(t.device))
    return m


def _fp64(pkg, oracle, oracle_torch, m, kind, feed):
    if kind == "sparse":
        masks = TR.dropout_masks(oracle, m, feed["edge_weight_dropout_keep_prob"], 1.0)
        return TR.oracle_loss_and_grads(oracle_torch, m, m._test_layers, feed, masks)
    if kind == "dense":
        return DT._fp64_step(oracle_torch, m, feed)
    return GR.model_fp64_step(oracle_torch, m, feed, None)


class _Calls:
    def __init__(self, pkg, monkeypatch):
        self.n = {"readout_loss_fwd": 0, "readout_loss_bwd": 0, "readout_multi_fwd": 0, "readout_multi_bwd": 0}
        for name in self.n:
            monkeypatch.setattr(pkg.ops, name, self._count(name, getattr(pkg.ops, name)))

    def _count(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted


def _three_steps(pkg, oracle, oracle_torch, cuda, monkeypatch, ms, kind, hidden, native, multi, out_keep=1.0, fp64=True):
    m = _model(pkg, oracle, cuda, ms, kind, hidden, native, multi)
    np.random.seed(11)
    feeds = [dict(f) for f in list(m.make_minibatch_iterator(m.train_data, True))[:3]]
    assert len(feeds) == 3
    for f in feeds:
        f["out_layer_dropout_keep_prob"] = out_keep
    want = _fp64(pkg, oracle, oracle_torch, m, kind, feeds[0]) if fp64 else None
    calls = _Calls(pkg, monkeypatch)
    with TR.capture_step_gradients(m) as steps:
        losses = [float(m.train_batch(f)) for f in feeds]
    entries = {n % t: float(m.ops[n % t]) for t in TASKS["task_ids"]
               for n in ("accuracy_task%i", "loss_numerator_task%i", "abs_error_sum_task%i", "loss_denominator_task%i")}
    assert len(m.ops["losses"]) == 3 and abs(sum(float(x) for x in m.ops["losses"]) - float(m.ops["loss"])) <= 1e-5 * abs(losses[-1])
    assert float(m.ops["loss"]) == losses[-1] and m.output.numel() == int(feeds[-1]["num_graphs"])
    return losses, steps, want, calls.n, entries


CASES = [("sparse", 32, True), ("sparse", 100, True)] + [(k, h, n) for k in ("dense", "gcn") for h in (32, 100) for n in (True, False)]


@pytest.mark.parametrize("kind,hidden,native", CASES)
def test_three_steps_with_and_without_the_key(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules, kind, hidden, native):
    """(The sparse model has no key for its native step: it takes it whenever train_native.eligible says so, as here.)"""
    runs = {}
    for multi in (False, True):
        runs[multi] = _three_steps(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules, kind, hidden, native, multi)
        monkeypatch.undo()
    (lt, st, want, ct, et), (lm, sm, _, cm, em) = runs[False], runs[True]
    print("losses per-task", lt, "multi", lm, "float64 step 1", float(want[0]))
    np.testing.assert_allclose(lm, lt, rtol=1e-5)
    assert abs(lm[0] - float(want[0])) <= 1e-5 * abs(float(want[0])) and abs(lt[0] - float(want[0])) <= 1e-5 * abs(float(want[0]))
    # under the key the per-task ops are not called: one multi forward and one multi backward per step
    assert cm == {"readout_loss_fwd": 0, "readout_loss_bwd": 0, "readout_multi_fwd": 3, "readout_multi_bwd": 3}, cm
    assert ct == {"readout_loss_fwd": 9, "readout_loss_bwd": 9, "readout_multi_fwd": 0, "readout_multi_bwd": 0}, ct
    # step-1 gradients of every variable: both routes against float64 at 2e-4 max|want| + 1e-7
    assert set(sm[0]) == set(st[0]) == set(want[1])
    for name, steps in (("multi", sm), ("per-task", st)):
        errs = TR.normwise_errors({k: t.cpu() for k, t in steps[0].items()}, want[1])
        worst = max(errs, key=lambda k: errs[k][1])
        print("%s: worst max-abs error / max|want| %.1e (%s)" % (name, errs[worst][1], worst))
        TR.assert_gradients_match(steps[0], want[1])
    assert set(em) == set(et) and len(em) == 12
    for k in em:
        assert np.isfinite(em[k]) and abs(em[k] - et[k]) <= 1e-5 * max(1.0, abs(et[k])), (k, em[k], et[k])


def test_readout_weight_dropout_keeps_its_per_task_masks(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules):
    """out_layer_dropout_keep_prob = 0.9 on the GCN's native step: the forward's dropped weights and the masks on the two weight
    gradients are the per-task route's -- losses to 1e-5, every step-1 gradient within 2e-4 of the per-task route's largest entry,
    and the same entries of the read-out weight gradients exactly zero."""
    runs = {}
    for multi in (False, True):
        runs[multi] = _three_steps(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules, "gcn", 32, True, multi, out_keep=0.9, fp64=False)
        monkeypatch.undo()
    (lt, st, _, ct, _), (lm, sm, _, cm, _) = runs[False], runs[True]
    np.testing.assert_allclose(lm, lt, rtol=1e-5)
    assert cm["readout_loss_fwd"] == cm["readout_loss_bwd"] == 0 and cm["readout_multi_fwd"] == cm["readout_multi_bwd"] == 3
    TR.assert_gradients_match(sm[0], {k: t.cpu().double() for k, t in st[0].items()})
    dropped = 0
    for k in st[0]:
        if "MLP_W_" in k:
            assert torch.equal(sm[0][k] == 0, st[0][k] == 0), k
            dropped += int((st[0][k] == 0).sum())
    assert dropped > 0


@pytest.mark.parametrize("kind", ["sparse", "dense", "gcn"])
def test_validation_forward_takes_the_multi_route(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules, kind):
    """forward_batch under torch.no_grad(): one forward-only multi call, model.output and the loss against the per-task route at the
    read-out's bounds (out: atol 2e-5, rtol 1e-5; loss 1e-5)."""
    res = {}
    for multi in (False, True):
        m = _model(pkg, oracle, cuda, molecules, kind, 100, False, multi)
        feed = next(iter(m.make_minibatch_iterator(m.valid_data, False)))
        calls = _Calls(pkg, monkeypatch)
        m.training = False
        with torch.no_grad():
            loss = float(m.forward_batch(feed))
        res[multi] = (loss, m.output.detach().cpu().numpy(), dict(calls.n), [float(m.ops["accuracy_task%i" % t]) for t in (0, 1, 2)])
        monkeypatch.undo()
    assert res[True][2] == {"readout_loss_fwd": 0, "readout_loss_bwd": 0, "readout_multi_fwd": 1, "readout_multi_bwd": 0}
    assert res[False][2]["readout_loss_fwd"] == 3 and res[False][2]["readout_multi_fwd"] == 0
    assert abs(res[True][0] - res[False][0]) <= 1e-5 * abs(res[False][0])
    np.testing.assert_allclose(res[True][1], res[False][1], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(res[True][3], res[False][3], rtol=1e-5)
    assert res[True][1].shape == res[False][1].shape and np.isfinite(res[True][1]).all()


def test_models_fall_back_without_error(pkg, oracle, oracle_torch, cuda, monkeypatch, molecules):
    """With the key set but one task only, the step is the per-task step bit for bit (no multi call)."""
    out = {}
    for multi in (False, True):
        cfg = {"task_ids": [1], "hidden_size": 32, "random_seed": 3, "batch_size": 1200, "native_training": True}
        if multi:
            cfg[KEY] = True
        m = pkg.SparseGCNChemModel({"--quiet": True, "--device": str(cuda), "train_data": molecules, "valid_data": molecules,
                                    "--config": json.dumps(cfg)})
        GN._randomise(m)
        np.random.seed(11)
        feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
        calls = _Calls(pkg, monkeypatch)
        with TR.capture_step_gradients(m) as steps:
            loss = float(m.train_batch(feed))
        out[multi] = (loss, steps[0], dict(calls.n))
        monkeypatch.undo()
    assert out[True][2] == out[False][2] == {"readout_loss_fwd": 1, "readout_loss_bwd": 1, "readout_multi_fwd": 0, "readout_multi_bwd": 0}
    assert out[True][0] == out[False][0]
    for k in out[False][1]:
        assert torch.equal(out[True][1][k], out[False][1][k]), k
