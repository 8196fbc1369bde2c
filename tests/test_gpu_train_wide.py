"""Training at hidden sizes 128 / 192 / 256 on the compacted route with the column-panel GRU backward (one launch per timestep,
csrc/ggnn_gru_bwd_panel.hip): the gradient the optimiser consumes against float64 autograd of the oracle, proof that the fused
launch -- not the three-launch route -- ran, the fused route against the unfused one on the same transform route, and one step
at size (50k nodes / 400k edges / h = 256)."""
import numpy as np
import pytest
import torch

import train_reference as tr
from test_gpu_fullsize import _large_model
from test_gpu_train import NATIVE_VS_AUTOGRAD_GRAD_RTOL
from test_gpu_train_gradients import MAX_TOL, NORM_TOL, _check_masked_entries, _small

pytestmark = pytest.mark.gpu

WIDE_CONFIGS = [
    ({"hidden_size": 128}, (1.0, 1.0)),
    ({"hidden_size": 192, "layer_timesteps": [2, 1], "residual_connections": {"1": [0]}, "graph_rnn_activation": "ReLU",
      "use_edge_msg_avg_aggregation": False}, (1.0, 1.0)),
    ({"hidden_size": 256, "use_edge_bias": True, "task_ids": [0, 1], "task_sample_ratios": {"1": 0.5, 1: 0.5}}, (0.8, 0.9)),
    ({"hidden_size": 116}, (1.0, 1.0)),                          # zero-padded to 128 inside the engine (ops.kernel_width)
]
WIDE_IDS = ["h128", "h192-sum-relu-residual", "h256-edge-bias-dropout-two-tasks", "h116-padded"]
UNFUSED_LAUNCHES = ("gru_bwd_stage1", "gru_bwd_dx_cand", "gru_bwd_dx_gates")


def _count_gru_backward_routes(pkg, monkeypatch):
    calls = {"fused": 0, "unfused": 0}
    fused, unfused = pkg.ops.gru_bwd_fused, pkg.backward._gru_backward_unfused

    def fused_counted(*a, **k):
        calls["fused"] += 1
        return fused(*a, **k)

    def unfused_counted(*a, **k):
        calls["unfused"] += 1
        return unfused(*a, **k)

    monkeypatch.setattr(pkg.ops, "gru_bwd_fused", fused_counted)
    monkeypatch.setattr(pkg.backward, "_gru_backward_unfused", unfused_counted)
    return calls


def _oracle_feed(feed, hidden_size):
    """The oracle sees the states at the model's own width (a padded engine width is the engine's business)."""
    return dict(feed, initial_node_representation=feed["initial_node_representation"][:, :hidden_size])


@pytest.mark.parametrize("config,keeps", WIDE_CONFIGS, ids=WIDE_IDS)
def test_wide_train_step_gradients_match_fp64(pkg, oracle, oracle_torch, cuda, config, keeps, monkeypatch):
    """One train_batch per configuration: loss to 1e-5 relative, every variable's gradient to the project's bound (2e-4 of its
    largest entry) against the fp64 oracle, dropped weights without gradient -- and the step's GRU backward was the fused launch."""
    monkeypatch.setattr(pkg.backward, "USE_WGRAD_STREAM", True)
    calls = _count_gru_backward_routes(pkg, monkeypatch)
    model, layers, feed = _small(pkg, oracle, config, keeps)
    D = config["hidden_size"]
    assert model._kw == pkg.ops.kernel_width(D) and pkg.ops.gru_bwd_is_fused(model._kw) and pkg.backward.compact_training(model._kw)
    assert not pkg.train_native.eligible(model, feed)            # (the two-call native step keeps refusing the panel sizes)
    masks = tr.dropout_masks(oracle, model, *keeps)
    want_loss, want = tr.oracle_loss_and_grads(oracle_torch, model, layers, _oracle_feed(feed, D), masks, device=cuda)
    with tr.capture_step_gradients(model) as steps:
        loss = float(model.train_batch(feed))
    torch.cuda.synchronize()
    assert len(steps) == 1
    got = steps[0]
    timesteps = sum(model.params["layer_timesteps"])
    assert calls == {"fused": timesteps, "unfused": 0}, calls
    assert abs(loss - want_loss) < 1e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    tr.assert_gradients_match(got, want)
    _check_masked_entries(got, masks)
    tr.assert_comparison_has_teeth(got, want)

    # the launches of one more forward + backward, by name: the fused kernel's, none of the three-launch route's
    variables = model.trainable_variables
    for v in variables.values():
        v.requires_grad_(True); v.grad = None
    model.training = True
    try:
        with pkg.ops.kernel_timing() as kt:
            model.forward_batch(feed).backward()
        names = set(kt.results())
    finally:
        model.training = False
        for v in variables.values():
            v.requires_grad_(False); v.grad = None
    assert any(n.startswith("gru_bwd_fused[nx=") or n.startswith("gru_bwd_fused_gather[nx=") for n in names), sorted(names)
    assert not [n for n in names if n.startswith(UNFUSED_LAUNCHES)], sorted(names)


@pytest.mark.parametrize("config,keeps", WIDE_CONFIGS[:3], ids=WIDE_IDS[:3])
def test_fused_and_unfused_gru_backward_agree_on_the_same_route(pkg, oracle, cuda, config, keeps, monkeypatch):
    """The same step with ops.gru_bwd_is_fused switched off (test_gpu_train.py's switch), the compacted transform kept on both
    sides: only the GRU backward's launches differ, and the gradients agree to the bound of the native-vs-autograd comparison
    (2e-6 of a variable's largest entry; measured worst 2.9e-7 / 2.7e-7 / 4.1e-7 for the three configurations)."""
    monkeypatch.setattr(pkg.backward, "compact_training", lambda D: bool(pkg.ops.compact_supported(D)))
    results = []
    for fused in (True, False):
        with monkeypatch.context() as mp:
            if not fused:
                mp.setattr(pkg.ops, "gru_bwd_is_fused", lambda D: False)
            calls = _count_gru_backward_routes(pkg, mp)
            model, _, feed = _small(pkg, oracle, config, keeps)
            with tr.capture_step_gradients(model) as steps:
                loss = float(model.train_batch(feed))
            torch.cuda.synchronize()
            timesteps = sum(model.params["layer_timesteps"])
            assert calls == ({"fused": timesteps, "unfused": 0} if fused else {"fused": 0, "unfused": timesteps}), calls
            results.append((loss, steps[0]))
    (l1, g1), (l0, g0) = results
    assert l1 == l0                                              # (the forward is the same launches)
    assert set(g1) == set(g0)
    worst = 0.0
    for k in g0:
        err, scale = float((g1[k] - g0[k]).abs().max()), float(g0[k].abs().max())
        worst = max(worst, err / max(scale, 1e-300))
        assert err <= NATIVE_VS_AUTOGRAD_GRAD_RTOL * scale, (k, err, scale)
    print("fused vs unfused GRU backward, %s: worst max|dg| / max|g| = %.3g" % (config, worst))


def _step_at_size(pkg, oracle, cuda):
    V, M, D, G = 50000, 400000, 256, 500
    model, layers, feed, *_ = _large_model(pkg, oracle, cuda, V, M, D, False, seed=5)
    feed = dict(feed)
    gen = torch.Generator(device="cpu").manual_seed(77)
    # (readout: G segments of V / G consecutive nodes each; the messages do not care where a "graph" ends)
    feed.update({"graph_nodes_list": (torch.arange(V, device=cuda) // (V // G)).to(torch.int32), "num_graphs": G,
                 "graph_ptr": torch.arange(0, V + 1, V // G, device=cuda).to(torch.int32), "graph_nodes_sorted": True,
                 "target_values": torch.randn((1, G), generator=gen).to(cuda), "target_mask": torch.ones((1, G), device=cuda),
                 "edge_weight_dropout_keep_prob": 1.0, "out_layer_dropout_keep_prob": 1.0})
    return model, layers, feed


def test_wide_train_step_at_size(pkg, oracle, oracle_torch, cuda, monkeypatch):
    """50,000 nodes / 400,000 edges / 4 edge types / h = 256 / 8 timesteps (the model of test_large_graph_kernel_paths_agree), read
    out as 500 graphs: one training step with finite gradients, loss and gradients bit-identical across two runs from the same
    weights, eight fused GRU backward launches per step, and -- the fp64 oracle's autograd fits on the device (~20 GB) -- every
    variable's gradient within the normwise / max-abs bounds of test_bench_size_native_step_gradients_match_fp64 (3e-6 / 4e-6:
    8x what the h = 100 native step measured over twice as many rows; K = 256 instead of 100 summands per product element widens
    an fp32 sum's error by at most sqrt(2.56) = 1.6).  Measured on the MI355X: worst normwise 7.3e-7, worst max-abs 8.7e-7, loss
    1.9e-7 relative."""
    calls = _count_gru_backward_routes(pkg, monkeypatch)
    runs = []
    for i in range(2):
        model, layers, feed = _step_at_size(pkg, oracle, cuda)
        if i == 0:                                               # (before the step moves the weights)
            want_loss, want = tr.oracle_loss_and_grads(oracle_torch, model, layers, feed, None, device=cuda)
        with tr.capture_step_gradients(model) as steps:
            loss = float(model.train_batch(feed))
        torch.cuda.synchronize()
        runs.append((loss, steps[0]))
        del model, layers, feed
    assert calls == {"fused": 16, "unfused": 0}, calls
    (l1, g1), (l2, g2) = runs
    assert np.isfinite(l1) and l1 == l2
    for k in g1:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g1[k], g2[k]), k
    errs = tr.normwise_errors(g1, want)
    print("at size: loss %.9g vs %.9g; worst normwise %.3g, worst max-abs %.3g" % (
        l1, want_loss, max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    assert abs(l1 - want_loss) <= 1e-5 * max(1.0, abs(want_loss)), (l1, want_loss)
    bad = {k: e for k, e in errs.items() if not (e[0] <= NORM_TOL and e[1] <= MAX_TOL)}
    assert not bad, bad
    tr.assert_comparison_has_teeth(g1, want, rtol=MAX_TOL, atol=0.0)
