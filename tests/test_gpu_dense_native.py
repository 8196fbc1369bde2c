"""GPU tests of the dense model's native training step (params['graph_resident_training'] == 'native'): the edge-weight / edge-bias
gradient kernel (ggnn_dense_edge_grad_f32) against float64 with ggnn_gemm_tn_f32 as the yardstick, its determinism and accumulation,
and the step on ggnn_dense_train_forward_f32 / ggnn_dense_train_backward_f32 -- gradients against float64, against the autograd
graph-resident route (key True), determinism, no read-back in a steady state, the fallbacks, and the reference's recorded runs
(chem_tensorflow_dense.py:93-117, chem_tensorflow.py:183-191).  Helpers come from test_gpu_dense_train.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import reference_golden as RG
import test_gpu_dense_train as DT
import train_reference as TR

pytestmark = pytest.mark.gpu

# (N, rows_per_step, E, D): the flagship stack (4 timesteps x 256 graphs x 29 vertices), the shapes of test_gpu_dense_train.SHAPES
# stacked over their timesteps, two rows, and an N that is no multiple of any slab or split size
KERNEL_SHAPES = [(29696, 7424, 4, 100), (7 * 29 * 4, 7 * 29, 4, 100), (5 * 17 * 3, 5 * 17, 8, 64), (4 * 5 * 4, 4 * 5, 2, 32), (2, 1, 4, 100),
                 (4099, 4099, 6, 64)]
ACCURACY = {}            # figures of test_edge_grad_kernel_against_fp64, written to $GGNN_DENSE_EDGE_GRAD_ACCURACY_JSON when that is set
NATIVE = "native"


def _kernel_inputs(N, rps, E, D, cuda):
    rng = np.random.default_rng(N + 7 * E + D)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)
    h = t(rng.uniform(-1, 1, (N, D)))
    dM = t(rng.normal(0, 1, (N, E * D)))
    dx = t(rng.normal(0, 1, (N, D)))
    nin = t(rng.integers(0, 4, (rps, E)))                                  # in-degrees: small non-negative integers
    return h, dM, dx, nin


def _replaced(pkg, h, dM, nin_rows, dx):
    """What the kernel replaces: ggnn_gemm_tn_f32 once per product and the permute copy into the variable's layout."""
    N, D = h.shape
    E = dM.shape[1] // D
    dW = pkg.ops.gemm_tn(h, dM).view(D, E, D).permute(1, 0, 2).contiguous()
    db = pkg.ops.gemm_tn(nin_rows, dx) if nin_rows is not None else None
    return dW, db


@pytest.mark.parametrize("with_nin", [True, False])
@pytest.mark.parametrize("N,rps,E,D", KERNEL_SHAPES)
def test_edge_grad_kernel_against_fp64(pkg, cuda, N, rps, E, D, with_nin):
    """ggnn_dense_edge_grad_f32 against h^T dM_e and nin^T dx in float64 on the kernel's own fp32 inputs.  Yardstick: ggnn_gemm_tn_f32
    on the same inputs against the same float64 (what the autograd route runs).  Bound for the new kernel, as in
    test_gpu_dense_train.test_backward_kernel_against_fp64: twice the yardstick's worst normwise error and twice its worst max-abs
    error, separately -- both are exact-format f32 chains that differ in summation order; a dropped term is an error of order 1.

    Measured on an MI355X (normwise / max-abs, worst of dW and db; profiles/dense_edge_grad_accuracy.json has every figure -- this
    test writes it when GGNN_DENSE_EDGE_GRAD_ACCURACY_JSON names a file):
        shape (N, rows_per_step, E, D)   yardstick (ggnn_gemm_tn_f32)   new kernel
        29696, 7424, 4, 100              3.9e-7 / 7.5e-7                4.0e-7 / 4.0e-7
        812, 203, 4, 100                 1.6e-7 / 2.0e-7                1.5e-7 / 1.7e-7
        255, 85, 8, 64                   1.5e-7 / 2.2e-7                1.5e-7 / 2.1e-7
        80, 20, 2, 32                    1.2e-7 / 1.7e-7                1.3e-7 / 2.3e-7
        2, 1, 4, 100                     3.0e-8 / 5.1e-8                3.0e-8 / 5.1e-8
        4099, 4099, 6, 64                2.1e-7 / 2.4e-7                1.9e-7 / 2.0e-7
    (the same with and without nin: the worst tensor is dW in every shape)."""
    assert pkg.ops.dense_edge_grad_supported(E, D)
    h, dM, dx, nin = _kernel_inputs(N, rps, E, D, cuda)
    nin_rows = nin[torch.arange(N, device=cuda) % rps].contiguous()
    h64, dM64 = h.double().cpu(), dM.double().cpu()
    want = {"dW": torch.stack([h64.t().matmul(dM64[:, e * D:(e + 1) * D]) for e in range(E)])}
    if with_nin:
        want["db"] = nin_rows.double().cpu().t().matmul(dx.double().cpu())

    yW, yb = _replaced(pkg, h, dM, nin_rows if with_nin else None, dx)
    yard = TR.normwise_errors({"dW": yW.cpu(), "db": None if yb is None else yb.cpu()}, want)
    worst_norm = max(e[0] for e in yard.values())
    worst_abs = max(e[1] for e in yard.values())

    dW, db = pkg.ops.dense_edge_grad(h, dM, nin if with_nin else None, dx if with_nin else None)
    assert tuple(dW.shape) == (E, D, D) and (db is None) == (not with_nin)
    new = TR.normwise_errors({"dW": dW.cpu(), "db": None if db is None else db.cpu()}, want)

    key = "N%d_rps%d_E%d_D%d_%s" % (N, rps, E, D, "nin" if with_nin else "nonin")
    ACCURACY[key] = {"yardstick_gemm_tn": yard, "dense_edge_grad": new, "bound": {"normwise": 2 * worst_norm, "max_abs": 2 * worst_abs}}
    print(key, json.dumps(ACCURACY[key]))
    path = os.environ.get("GGNN_DENSE_EDGE_GRAD_ACCURACY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(ACCURACY, f, indent=1, sort_keys=True)
    for k, (en, ea) in new.items():
        assert en <= 2 * worst_norm and ea <= 2 * worst_abs, (k, en, ea, worst_norm, worst_abs)


@pytest.mark.parametrize("N,rps,E,D", [(29696, 7424, 4, 100), (4099, 4099, 6, 64), (80, 20, 2, 32)])
def test_edge_grad_kernel_is_deterministic_and_accumulates(pkg, cuda, N, rps, E, D):
    h, dM, dx, nin = _kernel_inputs(N, rps, E, D, cuda)
    dW, db = pkg.ops.dense_edge_grad(h, dM, nin, dx)
    dW2, db2 = pkg.ops.dense_edge_grad(h, dM, nin, dx)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)                    # fixed-order sums: the same bits
    assert torch.isfinite(dW).all() and torch.isfinite(db).all() and float(dW.abs().max()) > 0 and float(db.abs().max()) > 0
    # whatever the workspace held before the call
    nbytes = pkg._lib.load().ggnn_dense_edge_grad_workspace_bytes(N, E, D)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=cuda)        # every float of it a NaN
    assert torch.isnan(ws[:nbytes // 4 * 4].view(torch.float32)).all()
    dW3, db3 = pkg.ops.dense_edge_grad(h, dM, nin, dx, ws=ws)
    assert torch.equal(dW, dW3) and torch.equal(db, db3)
    # without the bias operands: the same edge-weight gradient
    dW4, none = pkg.ops.dense_edge_grad(h, dM, ws=ws)
    assert none is None and torch.equal(dW, dW4)
    # accumulate: destination + result, one f32 add per element
    g = torch.Generator(device="cpu").manual_seed(3)
    accW = torch.randn((E, D, D), generator=g).to(cuda)
    accb = torch.randn((E, D), generator=g).to(cuda)
    wantW, wantb = accW + dW, accb + db
    outW, outb = pkg.ops.dense_edge_grad(h, dM, nin, dx, dW=accW, db=accb, accumulate=True)
    assert outW is accW and outb is accb
    assert torch.equal(accW, wantW) and torch.equal(accb, wantb)


def test_edge_grad_kernel_without_rows(pkg, cuda):
    """N == 0: zeros, or nothing under accumulate (as ggnn_gemm_tn_f32 treats M == 0)."""
    E, D = 4, 100
    h, dM, dx = (torch.empty((0, c), device=cuda) for c in (D, E * D, D))
    nin = torch.ones((5, E), device=cuda)
    dW = torch.full((E, D, D), 7.0, device=cuda)
    db = torch.full((E, D), 7.0, device=cuda)
    pkg.ops.dense_edge_grad(h, dM, nin, dx, dW=dW, db=db, accumulate=True)
    assert bool((dW == 7.0).all()) and bool((db == 7.0).all())
    pkg.ops.dense_edge_grad(h, dM, nin, dx, dW=dW, db=db)
    assert bool((dW == 0.0).all()) and bool((db == 0.0).all())
    dW2, none = pkg.ops.dense_edge_grad(h, dM)
    assert none is None and bool((dW2 == 0.0).all())


# ---- the step ------------------------------------------------------------------------------------------------------------------
class _Recorder(DT._Recorder):
    """... plus the autograd backward passes entered and the native launches counted."""

    def __init__(self, pkg, monkeypatch):
        super().__init__(pkg, monkeypatch)
        self.backwards = 0
        tb, ab = torch.Tensor.backward, torch.autograd.backward

        def tensor_backward(t, *a, **k):
            self.backwards += 1
            return tb(t, *a, **k)

        def autograd_backward(*a, **k):
            self.backwards += 1
            return ab(*a, **k)

        monkeypatch.setattr(torch.Tensor, "backward", tensor_backward)
        monkeypatch.setattr(torch.autograd, "backward", autograd_backward)
        self.forwards = lambda: sum(n.startswith("dense_train_forward[") for n in self.names)
        self.native_backwards = lambda: sum(n.startswith("dense_train_backward[") for n in self.names)


PER_TIMESTEP = ("dense_propagate_save[", "dense_propagate_bwd[", "gru", "msg_transform", "gather_segment_sum", "dense_aggregate", "gemm_tn", "xty")


@pytest.mark.parametrize("config", [{}, {"use_edge_bias": False, "hidden_size": 64, "task_ids": [0, 1]}])
def test_native_step_gradients_against_fp64(pkg, oracle, oracle_torch, cuda, monkeypatch, config):
    """test_gpu_dense_train.test_step_gradients_against_fp64 with the key 'native': every variable's gradient as the optimiser
    consumes it against float64 at the 2e-4 bound, the loss within 1e-5 relative; the two native calls ran once each, and the step
    issued no launch of the other routes, no A.nonzero() and entered no autograd backward."""
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5, num_tasks=2)
    m = DT._model(pkg, ms, cuda, graph_resident_training=NATIVE, **config)
    DT._randomise(m, oracle)
    assert pkg.train_native.dense_model_eligible(m)
    feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
    assert pkg.train_native.dense_eligible(m, feed)
    want_loss, want = DT._fp64_step(oracle_torch, m, feed)
    rec = _Recorder(pkg, monkeypatch)
    with TR.capture_step_gradients(m) as steps:
        loss = float(m.train_batch(feed))
    T = m.params["num_timesteps"]
    assert rec.names.count("dense_train_forward[steps=%d]" % T) == 1 and rec.names.count("dense_train_backward[steps=%d]" % T) == 1
    assert rec.forwards() == 1 and rec.native_backwards() == 1
    assert not [n for n in rec.names if n.startswith(PER_TIMESTEP)], rec.names
    assert rec.nonzero == 0 and rec.backwards == 0
    print("loss", loss, "float64", want_loss)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    got = steps[0]
    assert set(got) == set(want) and ("graph_model/Variable_1:0" in got) == m.params["use_edge_bias"]
    TR.assert_gradients_match(got, want)
    ew = "graph_model/Variable:0"
    D = m.params["hidden_size"]
    alias = lambda g: {(k + " /gnn_edge_weights_0" if k == ew else k): (t.reshape(-1, D) if k == ew else t) for k, t in g.items()}
    TR.assert_comparison_has_teeth(alias(got), alias(want))
    # model.ops as the autograd route leaves them
    assert tuple(m.ops["final_node_representations"].shape) == tuple(feed["initial_node_representation"].shape)
    assert float(m.ops["loss"]) == loss and len(m.ops["losses"]) == len(m.params["task_ids"])


EDGE_VARIABLES = ("graph_model/Variable:0", "graph_model/Variable_1:0")      # edge weights, edge biases


@pytest.mark.parametrize("config", [{}, {"use_edge_bias": False, "hidden_size": 64, "task_ids": [0, 1]}])
def test_native_step_against_the_autograd_graph_resident_route(pkg, oracle, oracle_torch, cuda, config):
    """Same seeded feed and weights under the keys 'native' and True: the same operand format; the loss and the gradient of every
    variable but the edge weights and edge biases bit for bit (the same launches on the same operands); the edge weights' and edge
    biases' gradients -- ggnn_dense_edge_grad_f32 here, ggnn_gemm_tn_f32 there -- apart by at most twice the True route's own error
    against float64, normwise and max-abs."""
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5, num_tasks=2)
    out = {}
    for key in (True, NATIVE):
        m = DT._model(pkg, ms, cuda, graph_resident_training=key, **config)
        DT._randomise(m, oracle)
        np.random.seed(17)
        feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
        want = DT._fp64_step(oracle_torch, m, feed)[1]
        with TR.capture_step_gradients(m) as steps:
            loss = float(m.train_batch(feed))
        out[key] = (loss, steps[0], m.last_format, want, {k: t.detach().clone() for k, t in m.named_variables().items()})
    (lt, gt, ft, want, wt), (ln, gn, fn, _, wn) = out[True], out[NATIVE]
    assert ft == fn and ft in (pkg.formats.F16X2, pkg.formats.BF16X3)
    assert lt == ln
    assert set(gt) == set(gn)
    for k in gt:
        if k not in EDGE_VARIABLES:
            assert torch.equal(gt[k], gn[k]), k
    edge = [k for k in gt if k in EDGE_VARIABLES]
    own = TR.normwise_errors({k: gt[k].cpu() for k in edge}, {k: want[k] for k in edge})
    for k in edge:
        w = want[k].double()
        d = gn[k].cpu().double().reshape(w.shape) - gt[k].cpu().double().reshape(w.shape)
        apart = (float(d.norm() / w.norm()), float(d.abs().max() / w.abs().max()))
        print(k, "apart", apart, "True route against float64", own[k])
        assert apart[0] <= 2 * own[k][0] and apart[1] <= 2 * own[k][1], (k, apart, own[k])
    for k in wt:                                                           # ... and the weights after Adam
        if k not in EDGE_VARIABLES:
            assert torch.equal(wt[k], wn[k]), k


def test_native_seeded_steps_are_deterministic(pkg, oracle, cuda, monkeypatch):
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5)
    rec = _Recorder(pkg, monkeypatch)
    runs = [DT._seeded_steps(pkg, oracle, cuda, ms, 3, graph_resident_training=NATIVE) for _ in range(2)]
    assert rec.forwards() == 6 and rec.native_backwards() == 6 and rec.saves() == 0
    DT._assert_same_bits(*runs)


def test_steady_state_step_reads_nothing_back(pkg, oracle, cuda, monkeypatch):
    """After two warm-up steps on device-packed feeds (whose packer declares max|h0| and max|A|) a native step measures no maximum
    (formats.absmax, i.e. no ggnn_absmax_f32 launch) and reads no tensor back (.tolist() / .item()): the weights' maxima come from
    formats.TrainingWeightBounds."""
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5)
    m = DT._model(pkg, ms, cuda, graph_resident_training=NATIVE, pack_on_device=True)
    DT._randomise(m, oracle, seed=1)
    np.random.seed(11)
    feeds = list(m.make_minibatch_iterator(m.train_data, True))[:3]
    assert len(feeds) == 3
    for f in feeds[:2]:
        m.train_batch(f)
    torch.cuda.synchronize()
    counts = {"absmax": 0, "tolist": 0, "item": 0}
    absmax, tolist, item = pkg.formats.absmax, torch.Tensor.tolist, torch.Tensor.item

    def count(name, fn):
        def wrapped(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(pkg.formats, "absmax", count("absmax", absmax))
    monkeypatch.setattr(torch.Tensor, "tolist", count("tolist", tolist))
    monkeypatch.setattr(torch.Tensor, "item", count("item", item))
    rec = _Recorder(pkg, monkeypatch)
    loss = m.train_batch(feeds[2])
    monkeypatch.undo()
    assert rec.forwards() == 1 and rec.native_backwards() == 1
    assert counts == {"absmax": 0, "tolist": 0, "item": 0}, counts
    assert np.isfinite(float(loss))
    assert m.last_format_bounds["proven"] and m.last_format == pkg.formats.F16X2


@pytest.mark.parametrize("config", [{"hidden_size": 128}, {"bucket": 40}, {"edge_weight_dropout_keep_prob": 0.8},
                                    {"graph_state_keep_prob": 0.9}])
def test_batches_the_native_step_cannot_take_fall_back(pkg, oracle, cuda, monkeypatch, config):
    """With the key 'native' but no graph-resident kernels for the batch, or dropout on the propagation, a seeded step equals the
    step of a model with the key True bit for bit (which test_gpu_dense_train.py equates with the step of a model without the key)."""
    ms = pkg.synthetic_qm9(120, mean_nodes=12, seed=6)
    cfg = {k: v for k, v in config.items() if k == "hidden_size"}

    def run(**extra):
        m = DT._model(pkg, ms, cuda, **cfg, **extra)
        DT._randomise(m, oracle, seed=2)
        if "bucket" in config:                                             # every graph into one bucket of 40 vertices
            m.train_data = m.process_raw_graphs(ms, True, bucket_sizes=np.array([config["bucket"]]))
        np.random.seed(13)
        feed = dict(next(iter(m.make_minibatch_iterator(m.train_data, True))))
        for k in ("edge_weight_dropout_keep_prob", "graph_state_keep_prob"):
            if k in config:
                feed[k] = config[k]
        with TR.capture_step_gradients(m) as steps:
            loss = float(m.train_batch(feed))
        return [loss], steps, {k: t.detach().clone() for k, t in m.named_variables().items()}

    rec = _Recorder(pkg, monkeypatch)
    native = run(graph_resident_training=NATIVE)
    assert rec.forwards() == 0 and rec.saves() == 0 and rec.names
    DT._assert_same_bits(native, run(graph_resident_training=True))


@pytest.mark.parametrize("case", [c for c in RG.DENSE_CASES if len(RG.Golden(c).train_losses)])
def test_training_follows_reference_run_on_the_native_step(pkg, cuda, tmp_path, monkeypatch, case):
    """test_gpu_dense_train.test_training_follows_reference_run_on_the_new_route with the key 'native': the same tolerances, copied."""
    g = RG.Golden(case)
    path = g.write_checkpoint(str(tmp_path / ("%s.pickle" % g.case)))
    with open(path, "rb") as f:
        ckpt = pickle.load(f)
    ckpt["params"] = dict(ckpt["params"], graph_resident_training=NATIVE)
    with open(path, "wb") as f:
        pickle.dump(ckpt, f)
    args = g.model_args(str(cuda), **{"--restore": path})
    args["--config"] = json.dumps(dict(g.params, graph_resident_training=NATIVE))
    m = pkg.DenseGGNNChemModel(args)
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    batches = list(m.make_minibatch_iterator(m.train_data, False))
    assert len(batches) == int(g.z["num_train_batches"])
    rec = _Recorder(pkg, monkeypatch)
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    assert rec.forwards() == rec.native_backwards() == len(g.train_losses) and rec.saves() == 0
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
    nv = m.named_variables()
    for i, n in enumerate(g.names):
        a = nv[n].detach().cpu().numpy()
        np.testing.assert_allclose(RG.stats(a), g.z["trained_stats"][i], rtol=1e-3, atol=5e-3, err_msg=n)
        if "trained/" + n in g.z.files:
            np.testing.assert_allclose(a.reshape(g.z["trained/" + n].shape), g.z["trained/" + n], rtol=1e-2, atol=3e-3, err_msg=n)


def _train_loop(pkg, cuda, g, log_dir, **extra):
    params = dict(g.params, graph_resident_training=NATIVE, **extra)
    m = pkg.DenseGGNNChemModel({"--device": str(cuda), "--log_dir": str(log_dir), "--config": json.dumps(params),
                                "train_data": g.train_molecules, "valid_data": g.valid_molecules})
    log = m.train()
    with open(m.best_model_file, "rb") as f:
        return log, pickle.load(f)


def test_train_loop_reproduces_reference_log_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """test_gpu_dense_train.test_train_loop_reproduces_reference_log_on_the_new_route with the key 'native': the same tolerances,
    copied; the checkpoint's params are the fixture's plus the key."""
    g = RG.GoldenLoop("loop_dense")
    rec = _Recorder(pkg, monkeypatch)
    log, best = _train_loop(pkg, cuda, g, tmp_path)
    assert rec.forwards() > 0 and rec.forwards() == rec.native_backwards() and rec.saves() == 0
    assert len(log) == len(g.z["train_loss"])
    np.testing.assert_allclose([e["train_results"][0] for e in log], g.z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][1] for e in log], g.z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][2] for e in log], g.z["train_error_ratio"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][0] for e in log], g.z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][1] for e in log], g.z["valid_accuracy"], rtol=1e-3)
    assert best["params"] == dict(g.params, graph_resident_training=NATIVE)
    assert (best["train_step"], best["valid_step"]) == (int(g.z["best_train_step"]), int(g.z["best_valid_step"]))
    assert set(best["weights"]) - {"ggnn_amd/adam_step:0"} == set(g.best_names)
    for i, n in enumerate(g.best_names):
        a = np.asarray(best["weights"][n], dtype=np.float64)
        ref = g.z["best_stats"][i]
        np.testing.assert_allclose(RG.stats(a)[1:], ref[1:], rtol=2e-3, atol=1e-6, err_msg=n)
        assert abs(RG.stats(a)[0] - ref[0]) <= 2e-3 * max(ref[1], 1e-3), n


def test_device_packing_equals_host_packing_on_the_native_step(pkg, cuda, tmp_path, monkeypatch):
    """pack_on_device and the key 'native' both set: the seeded three-epoch train() prints the same log and saves the same checkpoint
    as host packing with the key 'native', bit for bit."""
    g = RG.GoldenLoop("loop_dense")
    rec = _Recorder(pkg, monkeypatch)
    (log_h, best_h), (log_d, best_d) = (_train_loop(pkg, cuda, g, tmp_path / str(dev), pack_on_device=dev) for dev in (False, True))
    assert rec.forwards() > 0 and rec.forwards() == rec.native_backwards() and rec.saves() == 0
    assert len(log_d) == len(log_h) == len(g.z["train_loss"])
    for eh, ed in zip(log_h, log_d):
        for part in ("train_results", "valid_results"):
            assert float(eh[part][0]) == float(ed[part][0]), part
            np.testing.assert_array_equal(np.asarray(eh[part][1]), np.asarray(ed[part][1]))
            np.testing.assert_array_equal(np.asarray(eh[part][2]), np.asarray(ed[part][2]))
    assert set(best_h["weights"]) == set(best_d["weights"])
    for n in best_h["weights"]:
        assert np.asarray(best_h["weights"][n]).tobytes() == np.asarray(best_d["weights"][n]).tobytes(), n
