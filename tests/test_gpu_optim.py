"""ggnn_clip_adam_f32 (csrc/ggnn_optim.hip) -- per-variable tf.clip_by_norm + TF-1.3 ApplyAdam for all variables in two launches --
against the float64 reference of tests/optim_reference.py: p, m and v of every variable after every step, each step judged on its
own from the float32 state read back before it, with s the clip scale and u = 2^-24

    |dm| <= C u (b1 |m| + (1 - b1) s |g|)
    |dv| <= C u (b2 v + (1 - b2) s^2 g^2)
    |dp| <= u |p_want| + C u lr_t (b1 |m| + (1 - b1) s |g|) / (sqrt(v_want) + eps)

first on the kernel alone (tails, the block edge, 40 and 301 blocks; clipped and unclipped neighbours in one launch; inactive
variables; all-zero gradients; no clipping; determinism; the padding of the flat buffers; the per-step bound of
formats.adam_step_bound that the f16x2 range proof leans on), then on the optimiser as four step routes of the models wire it
(pointer and block tables, active flags, views, t and lr_t across steps, save and restore of the slots).

C = 16 (optim_reference.C): the smallest power of two at least twice the worst ratio measured on the MI355X against float64.
Worst ratios there (every test prints its own): m 3.81, v 6.33, p 3.99 over the kernel cases (m and v: the seven-variable case, p:
no clipping), m 3.45, v 6.31, p 2.94 over the four model routes; worst step of the 400-step run 2.874 lr = 0.395 of
adam_step_bound.  The float32 NumPy restatement of the kernel (test_optim_reference_host.py) predicts the same: worst 3.9 / 6.3 /
4.0 without contraction into fused multiply-adds, worst step 2.874 lr.  test_optim_reference_host.py shows that on the inputs used here every wrong optimiser of
optim_reference.MUTATIONS is outside these bounds by at least 100 C."""
import numpy as np
import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

HYPER = R.KERNEL_HYPER


def _device(xs, cuda):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(cuda) for x in xs]


def _state(ws, opt):
    return R.to_numpy(ws), R.to_numpy(opt.m), R.to_numpy(opt.v)


def _drive(pkg, cuda, p0, grads, clip, reference=True):
    """One fused TFAdam over float32 copies of p0; per step: read p, m, v back, load the gradients (None: no gradient), step, read
    back again.  -> (weights, optimiser, [{"before", "after": (p, m, v); "want": the float64 step on `before`; "ratios"}])."""
    ws = _device(p0, cuda)
    opt = pkg.train.TFAdam(ws, **{"lr": HYPER["lr"], "beta1": HYPER["b1"], "beta2": HYPER["b2"], "epsilon": HYPER["eps"]})
    assert opt.fused
    recs = []
    for t, gs in enumerate(grads, 1):
        before = _state(ws, opt)
        opt.load_gradients(_device(gs, cuda))
        opt.clip_and_apply(clip)
        after = _state(ws, opt)
        rec = {"t": t, "before": before, "after": after}
        if reference:
            active = [0 if g is None else 1 for g in gs]
            g0 = [np.zeros_like(p) if g is None else g for g, p in zip(gs, p0)]
            rec["want"] = R.step(*before[:1], g0, *before[1:], t, clip, active=active, **HYPER)
            rec["ratios"] = R.ratios(*after, rec["want"])
        recs.append(rec)
    assert opt.t == len(grads)
    return ws, opt, recs


def _assert_inside_bounds(recs, label, sizes):
    worst = np.zeros(3)
    for rec in recs:
        for i, r in enumerate(rec["ratios"]):
            worst = np.maximum(worst, r)
    print("clip_adam %s: worst C  m %.2f  v %.2f  p %.2f" % ((label,) + tuple(worst)))
    for rec in recs:
        for i, r in enumerate(rec["ratios"]):
            assert max(r) <= R.C, (label, "step %d" % rec["t"], "numel %d" % sizes[i], dict(zip("mvp", r)))
    return worst


def _bit_equal(a, b):
    return all(np.array_equal(x, y) for xs, ys in zip(a, b) for x, y in zip(xs, ys))


# ---- the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magnitude", [1.0, 1e-3], ids=["w1", "w1e-3"])
def test_clip_adam_kernel_against_fp64(pkg, cuda, magnitude):
    """Seven variables of 1, 3, 1023, 1024, 1025, 40000 and 307205 floats (optim_reference.KERNEL_SIZES) over five steps with a
    fresh gradient each (uniform, 10 % exact zeros, base scales 1e-7 .. 30 and a per-step factor 0.3 .. 3) at clip norm 1: in every
    launch clipped and unclipped variables are neighbours in the flat buffer.  From weights of magnitude 1 the rounding of p
    dominates its bound; from 1e-3 the update itself is checked to about 1e-6 relative.  The padding of g, m and v stays zero."""
    p0, grads = R.kernel_inputs(magnitude)
    ws, opt, recs = _drive(pkg, cuda, p0, grads, R.KERNEL_CLIP)
    for rec in recs:
        clipped = [n > R.KERNEL_CLIP for n in rec["want"]["norm"]]
        assert any(a != b for a, b in zip(clipped, clipped[1:])), clipped
    assert {rec["want"]["norm"][R.KERNEL_SIZES.index(1023)] > R.KERNEL_CLIP for rec in recs} == {True, False}
    assert opt._flat["nblocks"] == sum((n + 1023) // 1024 for n in R.KERNEL_SIZES) and (307205 + 1023) // 1024 > 256
    _assert_inside_bounds(recs, "kernel sizes, |w| ~ %g" % magnitude, R.KERNEL_SIZES)
    assert R.padding_is_zero(opt)
    assert all(np.isfinite(x).all() for xs in recs[-1]["after"] for x in xs)


def test_inactive_variable_is_left_alone_and_resumes_at_the_global_step(pkg, cuda):
    """A variable with a None gradient in steps 2 and 3 (var_active == 0 through load_gradients): p, m and v are bit-equal across
    those steps, and its step 4 is taken with t = 4 -- a step taken with the variable's own count of updates (t = 2) is outside
    the bound."""
    sizes = (3, 1025, 2000)
    rng = np.random.default_rng(11)
    p0 = [rng.uniform(-1e-3, 1e-3, n).astype(np.float32) for n in sizes]
    grads = [[R.draw_gradient(rng, n, s * f) for n, s in zip(sizes, (1e-4, 30.0, 3e-2))] for f in R.KERNEL_STEP_FACTORS]
    for t in (2, 3):
        grads[t - 1][1] = None
    ws, opt, recs = _drive(pkg, cuda, p0, grads, R.KERNEL_CLIP)
    _assert_inside_bounds(recs, "inactive variable", sizes)
    for t in (2, 3):
        rec = recs[t - 1]
        assert all(np.array_equal(rec["before"][k][1], rec["after"][k][1]) for k in range(3)), t
        assert any(not np.array_equal(rec["before"][0][i], rec["after"][0][i]) for i in (0, 2))          # (the others moved)
    assert np.abs(recs[3]["after"][0][1] - recs[3]["before"][0][1]).max() > 0
    rec = recs[3]
    own_count = R.step(*rec["before"][:1], grads[3], *rec["before"][1:], 2, R.KERNEL_CLIP, **HYPER)
    assert max(R.ratios(*rec["after"], own_count)[1]) > 100 * R.C
    assert R.padding_is_zero(opt)


def test_all_zero_gradient_of_an_active_variable(pkg, cuda):
    """An active variable whose gradient is all zero has norm 0 and scale 1 (no 0 / 0): at step 1 its p, m and v stay exactly as
    they were; after two real steps its m decays, its p moves on momentum, everything stays finite and inside the bounds."""
    sizes = (5, 1500)
    rng = np.random.default_rng(12)
    p0 = [rng.uniform(-1e-3, 1e-3, n).astype(np.float32) for n in sizes]
    grads = [[R.draw_gradient(rng, n, 30.0 * f) for n in sizes] for f in R.KERNEL_STEP_FACTORS]
    for t in (1, 2):
        grads[t - 1][0] = np.zeros(5, np.float32)
    for t in (3, 4, 5):
        grads[t - 1][1] = np.zeros(1500, np.float32)
    ws, opt, recs = _drive(pkg, cuda, p0, grads, R.KERNEL_CLIP)
    _assert_inside_bounds(recs, "all-zero gradient", sizes)
    assert all(np.isfinite(x).all() for rec in recs for xs in rec["after"] for x in xs)
    first = recs[0]
    assert first["want"]["norm"][0] == 0.0 and first["want"]["scale"][0] == 1.0
    assert np.array_equal(first["after"][0][0], p0[0]) and not first["after"][1][0].any() and not first["after"][2][0].any()
    for t in (3, 4, 5):
        (pb, mb, vb), (pa, ma, va) = recs[t - 1]["before"], recs[t - 1]["after"]
        live = mb[1] != 0
        assert live.mean() > 0.8 and (np.abs(ma[1][live]) < np.abs(mb[1][live])).all() and (va[1] <= vb[1]).all()
        assert (pa[1][live] != pb[1][live]).mean() > 0.9


def test_clip_norm_none_and_zero_both_mean_no_clipping(pkg, cuda):
    p0, grads = R.kernel_inputs(1e-3, seed=5)
    out = []
    for clip in (None, 0.0):
        ws, opt, recs = _drive(pkg, cuda, p0, grads, clip)
        assert all(s == 1.0 for rec in recs for s in rec["want"]["scale"])
        assert max(n for rec in recs for n in rec["want"]["norm"]) > 100.0                  # (which clip norm 1 would have scaled)
        _assert_inside_bounds(recs, "clip_norm %r" % (clip,), R.KERNEL_SIZES)
        out.append(recs[-1]["after"])
    assert _bit_equal(out[0], out[1])


def test_second_optimizer_on_the_same_inputs_is_bit_equal(pkg, cuda):
    p0, grads = R.kernel_inputs(1.0, seed=6)
    runs = [_drive(pkg, cuda, p0, grads, R.KERNEL_CLIP, reference=False)[2] for _ in range(2)]
    for a, b in zip(*runs):
        assert _bit_equal(a["after"], b["after"]), a["t"]


def test_step_bound_holds_on_the_kernel(pkg, cuda):
    """formats.adam_step_bound -- the per-step |delta w| <= lr C with which TrainingWeightBounds calls a layer's weights provably
    inside the f16x2 operand range between re-measurements -- on the kernel that moves the weights: one variable of 60 elements from
    p = 0, clipping off, element i following adversarial history i of test_adam_step_bound_holds_against_adversarial_gradients for
    400 steps.  Every step: max |p_after - p_before| <= adam_step_bound + ulp(p); over the run the worst step exceeds 0.5 lr."""
    lr, b1, b2 = HYPER["lr"], HYPER["b1"], HYPER["b2"]
    bound = pkg.formats.adam_step_bound(lr, b1, b2)
    hist = torch.from_numpy(R.adversarial_histories(b1, b2).astype(np.float32).T.copy()).to(cuda)        # [400, 60]
    w = torch.zeros(hist.shape[1], dtype=torch.float32, device=cuda)
    opt = pkg.train.TFAdam([w], lr=lr, beta1=b1, beta2=b2, epsilon=HYPER["eps"])
    assert opt.fused
    worst = torch.zeros((), dtype=torch.float64, device=cuda)
    over = torch.zeros((), dtype=torch.float64, device=cuda)                       # worst (delta - bound - ulp)
    for t in range(hist.shape[0]):
        prev = w.clone()
        opt.load_gradients([hist[t]])
        opt.clip_and_apply(None)
        delta = (w.double() - prev.double()).abs()
        ulp = (torch.nextafter(w.abs(), torch.full_like(w, float("inf"))) - w.abs()).double()
        worst = torch.maximum(worst, delta.max())
        over = torch.maximum(over, (delta - bound - ulp).max())
    worst, over = float(worst), float(over)
    print("clip_adam step bound: worst step %.3f lr = %.3f of adam_step_bound" % (worst / lr, worst / bound))
    assert bool(torch.isfinite(w).all()) and over <= 0.0, (worst, bound, over)
    assert worst > 0.5 * lr


# ---- the optimiser as the models wire it -------------------------------------------------------------------------------------------
# clamp_gradient_norm per route, read off the norms the test prints, so that already in step 1 (whose gradient does not depend on
# the choice) clipped and unclipped variables alternate in the flat buffer.  Step-1 norms on the MI355X:
#   sparse  edge weights 0.010-0.029, candidate kernels 0.026-0.070 and biases 0.05-0.33 | gates kernels and biases 0.0009-0.0036
#   dense   edge weights 0.76, edge biases 0.52, candidate 0.96 / 0.53, regression 0.35 / 0.43 | gates 0.083 / 0.036, gate MLP 0.03 / 0.01
#   gcn     layer weights 0.76-1.38, regression 0.99 / 4.7 | regression gate 0.054 / 0.107
ROUTE_CLIP = {"sparse-native": 0.02, "sparse-autograd": 0.02, "dense": 0.3, "gcn": 0.3}


def _route_model(pkg, route, monkeypatch, clip=None):
    config = {"clamp_gradient_norm": ROUTE_CLIP[route] if clip is None else clip}
    args = lambda ms, **c: {"--quiet": True, "--device": "cuda:0", "train_data": ms, "valid_data": ms, "--config": dict(config, **c)}
    if route.startswith("sparse"):
        if route == "sparse-autograd":
            monkeypatch.setattr(pkg.backward, "USE_NATIVE_STEP", False)
            monkeypatch.setattr(pkg.backward, "USE_WGRAD_STREAM", True)
        return pkg.SparseGGNNChemModel(args(pkg.synthetic_qm9(300, mean_nodes=10, seed=4), batch_size=1000))
    if route == "dense":
        return pkg.DenseGGNNChemModel(args(pkg.synthetic_qm9(200, mean_nodes=12, seed=5), batch_size=16, random_seed=5))
    return pkg.SparseGCNChemModel(args(pkg.synthetic_qm9(300, seed=2), batch_size=1000, random_seed=3))


def _three_batches(model):
    np.random.seed(model.params["random_seed"])
    feeds = []
    for feed in model.make_minibatch_iterator(model.train_data, is_training=True):
        feed = dict(feed)
        feed["out_layer_dropout_keep_prob"] = model.params["out_layer_dropout_keep_prob"]
        feeds.append(feed)
        if len(feeds) == 3:
            break
    assert len(feeds) == 3
    return feeds


def _check_captured_steps(model, steps, label):
    """Every captured step against optim_reference.step on its own gradient and pre-step state -> the per-step per-variable
    (norm, clipped) table."""
    opt = model.optimizer
    worst, table = np.zeros(3), []
    for rec in steps:
        want = R.reference_of_captured_step(rec, opt.lr, opt.b1, opt.b2, opt.eps)
        got = [R.to_numpy(rec["after"][k]) for k in ("p", "m", "v")]
        rs = R.ratios(*got, want)
        for name, r in zip(rec["names"], rs):
            assert max(r) <= R.C, (label, "step %d" % rec["t"], name, dict(zip("mvp", r)))
            worst = np.maximum(worst, r)
        active = rec["active"].cpu().tolist()
        table.append([(n, a, name) for n, a, name in zip(want["norm"], active, rec["names"])])
        print("%s step %d clip %g norms: %s" % (label, rec["t"], rec["clip"],
                                                 "  ".join("%s %.3g%s" % (name.split("/", 1)[-1], n, "" if a else " (inactive)")
                                                           for n, a, name in table[-1])))
    print("clip_adam %s: worst C  m %.2f  v %.2f  p %.2f" % ((label,) + tuple(worst)))
    return table


@pytest.mark.parametrize("route", ["sparse-native", "sparse-autograd", "dense", "gcn"])
def test_model_optimizer_steps_against_fp64(pkg, cuda, route, monkeypatch):
    """Three training steps on three different batches: the sparse default model on the native step and on the autograd path with
    the weight-gradient sink, the dense model and the sparse GCN.  Every variable's p, m and v after each step against
    optim_reference.step on that step's captured gradient and pre-step state, with the bounds and the C of the kernel tests (the
    gradient itself is held elsewhere: test_gpu_train_gradients.py); t, the version counters and the padding."""
    model = _route_model(pkg, route, monkeypatch)
    opt = model.optimizer
    assert opt.fused and opt.t == 0
    feeds = _three_batches(model)
    if route.startswith("sparse"):
        assert pkg.train_native.eligible(model, feeds[0]) == (route == "sparse-native")
    versions = [v._version for v in opt.vars]
    with R.capture_optimizer_steps(model) as steps:
        for feed in feeds:
            model.train_batch(feed)
    torch.cuda.synchronize()
    assert len(steps) == 3 and [rec["t"] for rec in steps] == [1, 2, 3] and opt.t == 3
    assert all(rec["clip"] == ROUTE_CLIP[route] for rec in steps)
    assert [v._version for v in opt.vars] == [n + 3 for n in versions]
    table = _check_captured_steps(model, steps, route)
    clip = ROUTE_CLIP[route]
    assert any(a and n > clip for n, a, _ in table[0]) and any(a and 0 < n <= clip for n, a, _ in table[0]), table[0]
    assert R.padding_is_zero(opt)
    for rec in steps:                                        # (an inactive variable's zero magnitudes admit no change at all)
        for i, a in enumerate(rec["active"].cpu().tolist()):
            if a and bool(rec["g"][i].any()):
                assert not torch.equal(rec["before"]["p"][i], rec["after"]["p"][i]), (rec["t"], rec["names"][i])


def test_resumed_model_takes_a_bit_equal_next_step(pkg, cuda, monkeypatch, tmp_path):
    """After three steps the sparse model's checkpoint, written by its own save_progress, is restored into a fresh model (m and v
    through load_state_variables into the views of the flat buffers); step 4 on the same batch leaves p, m and v bit-equal in
    both.  (Dropout masks are keyed on the number of steps the model object has taken, which a checkpoint does not hold: step 4
    runs with both keep probabilities at 1.)"""
    model = _route_model(pkg, "sparse-native", monkeypatch)
    feeds = _three_batches(model)
    for feed in feeds:
        model.train_batch(feed)
    path = str(tmp_path / "model.pickle")
    model.save_progress(path, 3, 0)
    fresh = _route_model(pkg, "sparse-native", monkeypatch)
    assert fresh.optimizer.fused and fresh.optimizer.t == 0
    assert fresh.restore_progress(path) == (3, 0)
    a, b = model.optimizer, fresh.optimizer
    assert b.t == 3 and all(x.untyped_storage().data_ptr() == b._flat["m"].untyped_storage().data_ptr() for x in b.m)
    assert float(sum(x.abs().sum() for x in a.m)) > 0 and float(sum(x.sum() for x in a.v)) > 0
    state = lambda o: (o.vars, o.m, o.v)
    for xs, ys in zip(state(a), state(b)):
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    for mdl in (model, fresh):
        feed = dict(feeds[0])
        feed["edge_weight_dropout_keep_prob"] = feed["out_layer_dropout_keep_prob"] = 1.0
        assert pkg.train_native.eligible(mdl, feed)
        mdl.train_batch(feed)
    torch.cuda.synchronize()
    assert a.t == b.t == 4
    for k, (xs, ys) in zip("pmv", zip(state(a), state(b))):
        for name, x, y in zip(model.trainable_variables, xs, ys):
            assert torch.equal(x, y), (k, name)
    assert R.padding_is_zero(b)
