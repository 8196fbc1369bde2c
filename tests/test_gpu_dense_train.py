"""GPU tests of the graph-resident dense training route (params['graph_resident_training']; chem_tensorflow_dense.py:93-117 and what TF
autodiff derives from it): the saving forward launch against the plain one and the float64 twin, the backward launch against float64
autograd with the per-timestep route as the yardstick, the model's step gradients, determinism, the fallbacks, the reference's
recorded runs under the new route, and device packing."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import reference_golden as RG
import train_reference as TR

pytestmark = pytest.mark.gpu

# test_graph_resident_dense_forward's shapes, plus one vertex in one graph and the flagship batch, plus two with six edge types (the
# backward's second group of operand blocks half full; D = 64 and D = 32 differ in chunk count)
SHAPES = [(7, 29, 4, 100, True, 4), (3, 32, 4, 100, False, 2), (5, 17, 8, 64, True, 3), (4, 5, 2, 32, True, 4), (2, 16, 6, 100, True, 1),
          (256, 29, 4, 100, True, 4), (1, 1, 4, 100, True, 2), (3, 9, 6, 64, True, 2), (2, 20, 6, 32, False, 3)]
ACCURACY = {}            # figures of test_backward_kernel_against_fp64, written to $GGNN_DENSE_TRAIN_ACCURACY_JSON when that is set


def _inputs(oracle, b, v, E, D, bias, steps, weighted=False):
    rng = np.random.default_rng(b * v + E)
    A = (rng.random((b, E, v, v)) < 2.0 / v).astype(np.float32)
    if weighted:
        A = A * rng.uniform(0.05, 1.95, A.shape).astype(np.float32)        # weighted edges, entries in (0, 2)
    if b > 1:
        A[b - 1] = 0.0                                                     # a graph without edges
    h0 = rng.uniform(-1, 1, (b, v, D)).astype(np.float32)
    W = oracle.glorot_init(rng, [E, D, D])
    eb = rng.normal(0, 0.1, [E, D]).astype(np.float32) if bias else None
    gru = {"Wg": oracle.glorot_init(rng, [2 * D, 2 * D]), "bg": (1 + rng.normal(0, 0.1, 2 * D)).astype(np.float32),
           "Wc": oracle.glorot_init(rng, [2 * D, D]), "bc": rng.normal(0, 0.1, D).astype(np.float32)}
    d_out = rng.normal(0, 1, (b, v, D)).astype(np.float32)
    return dict(A=A, h0=h0, W=W, eb=eb, d_out=d_out, **gru)


def _twin(x, steps):
    """The float64 twin of chem_tensorflow_dense.py:93-117 with every intermediate kept (torch, differentiable):
    -> (out [b,v,D], [per timestep {h, x, r, u, c, rh, pg, pc, M}])."""
    b, v, D = x["h0"].shape
    E = x["W"].shape[0]
    h = x["h0"].reshape(b * v, D)
    inter = []
    for _ in range(steps):
        M = [h.matmul(x["W"][e]) for e in range(E)]                        # h W_e; the bias joins below (:107-108)
        acts = 0
        for e in range(E):
            m = M[e] if x["eb"] is None else M[e] + x["eb"][e]
            acts = acts + torch.bmm(x["A"][:, e], m.reshape(b, v, D))
        xs = acts.reshape(b * v, D)
        pg = torch.cat([xs, h], dim=1).matmul(x["Wg"]) + x["bg"]
        r, u = torch.sigmoid(pg[:, :D]), torch.sigmoid(pg[:, D:])
        rh = r * h
        pc = torch.cat([xs, rh], dim=1).matmul(x["Wc"]) + x["bc"]
        c = torch.tanh(pc)
        inter.append(dict(h=h, x=xs, r=r, u=u, c=c, rh=rh, pg=pg, pc=pc, M=M))
        h = u * h + (1 - u) * c
    return h.reshape(b, v, D), inter


def _t64(x, grad=()):
    out = {k: None if a is None else torch.from_numpy(np.asarray(a)).double() for k, a in x.items()}
    for k in grad:
        if out[k] is not None:
            out[k].requires_grad_(True)
    return out


def _dev(x, cuda):
    return {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for k, a in x.items()}


def _fp64_gradients(x, steps):
    """float64 autograd of the twin on the kernel's own fp32 inputs -> d_h0, the stacked dpc / dpg / dx / dM, the variables' gradients."""
    t = _t64(x, grad=("h0", "W", "eb", "Wg", "bg", "Wc", "bc"))
    out, inter = _twin(t, steps)
    keep = [s[k] for s in inter for k in ("pc", "pg", "x")] + [m for s in inter for m in s["M"]]
    for k in keep:
        k.retain_grad()
    (out * t["d_out"]).sum().backward()
    D = x["h0"].shape[2]
    want = {"d_h0": t["h0"].grad, "dpc": torch.stack([s["pc"].grad for s in inter]), "dpg": torch.stack([s["pg"].grad for s in inter]),
            "dx": torch.stack([s["x"].grad for s in inter]),
            "dM": torch.stack([torch.cat([m.grad for m in s["M"]], dim=1) for s in inter])}
    var = {k: t[k].grad for k in ("W", "eb", "Wg", "bg", "Wc", "bc") if t[k] is not None}
    return want, var, [{k: s[k].detach() for k in ("h", "x", "r", "u", "c", "rh")} for s in inter], out.detach(), D


def _formulas(x, inter, steps):
    """The backward as the issue writes it, in float64 on the twin's intermediates."""
    t = _t64(x)
    b, v, D = x["h0"].shape
    E = x["W"].shape[0]
    Wg, Wc, W, A = t["Wg"], t["Wc"], t["W"], t["A"]
    g = t["d_out"].reshape(b * v, D)
    out = {k: [None] * steps for k in ("dpc", "dpg", "dx", "dM")}
    for s in range(steps - 1, -1, -1):
        h, r, u, c = (inter[s][k] for k in ("h", "r", "u", "c"))
        dpc = g * (1 - u) * (1 - c * c)
        dpu = g * (h - c) * u * (1 - u)
        drh = dpc.matmul(Wc[D:].t())
        dpr = drh * h * r * (1 - r)
        dx = dpr.matmul(Wg[:D, :D].t()) + dpu.matmul(Wg[:D, D:].t()) + dpc.matmul(Wc[:D].t())
        dh = g * u + drh * r + dpr.matmul(Wg[D:, :D].t()) + dpu.matmul(Wg[D:, D:].t())
        dMs = []
        for e in range(E):
            dM = torch.bmm(A[:, e].transpose(1, 2), dx.reshape(b, v, D)).reshape(b * v, D)     # dM_e[src] = sum_dst A_e[dst,src] dx[dst]
            dh = dh + dM.matmul(W[e].t())
            dMs.append(dM)
        out["dpc"][s], out["dpg"][s], out["dx"][s], out["dM"][s] = dpc, torch.cat([dpr, dpu], dim=1), dx, torch.cat(dMs, dim=1)
        g = dh
    res = {k: torch.stack(vv) for k, vv in out.items()}
    res["d_h0"] = g.reshape(b, v, D)
    return res


REFUSED = (16, 6, 100)   # (v, E, D) of the forward's list outside the training route's set, see _assert_refused


def _supported(pkg, v, E, D):
    """Every shape of SHAPES must run the route on the split matrix path -- a build that refuses one FAILS here -- except REFUSED."""
    if not pkg.formats.split_path():
        pytest.skip("f32 matrix path (GGNN_MATRIX=f32): the graph-resident training route reports itself unsupported there")
    if (v, E, D) == REFUSED:
        return False
    assert pkg.ops.dense_train_supported(v, E, D), (v, E, D)
    return True


def _assert_refused(pkg, x, cuda, steps):
    """The one shape of the forward's list outside the training route's set (the split-form forward's LDS blocks do not fit D = 100
    with six edge types, so that launch runs the f32-MFMA kernel): the route says so, and both launches return GGNN_E_UNSUPPORTED
    with a message instead of running."""
    b, v, D = x["h0"].shape
    E = x["W"].shape[0]
    assert not pkg._lib.load().ggnn_dense_propagate_is_split(v, E, D) and not pkg.ops.dense_train_supported(v, E, D)
    d = _dev(x, cuda)
    _, eimg, gimg = _images(pkg, d)
    with pytest.raises(pkg._lib.GGNNError) as e:
        pkg.ops.dense_propagate_save(d["h0"], d["A"], eimg, gimg, d["eb"], d["bg"], d["bc"], steps)
    assert e.value.code == -2 and "v=%d E=%d D=%d" % (v, E, D) in str(e.value)
    saved = torch.zeros((6, steps, b * v, D), device=cuda)
    with pytest.raises(pkg._lib.GGNNError) as e:
        pkg.ops.dense_propagate_bwd(d["d_out"], d["A"], torch.zeros(16, device=cuda), saved)
    assert e.value.code == -2


def _images(pkg, d):
    P = pkg.ops.PackedWeights()
    D = d["h0"].shape[2]
    return P, P.dense_edge(d["W"]), P.dense_gru(d["Wg"], d["Wc"], D)


@pytest.mark.parametrize("b,v,E,D,bias,steps", SHAPES)
@pytest.mark.parametrize("fmt", [3, 2])
def test_saving_forward_is_the_plain_forward(pkg, oracle, oracle_torch, cuda, b, v, E, D, bias, steps, fmt):
    """The saving launch's `out` equals ops.dense_propagate's bit for bit in both operand formats; every saved tensor matches the
    float64 twin's intermediate at test_graph_resident_dense_forward's tolerances (atol 1e-5, rtol 1e-4); saved h_0 is h0 exactly."""
    x = _inputs(oracle, b, v, E, D, bias, steps)
    if not _supported(pkg, v, E, D):
        return _assert_refused(pkg, x, cuda, steps)
    d = _dev(x, cuda)
    _, eimg, gimg = _images(pkg, d)
    plain = pkg.ops.dense_propagate(d["h0"], d["A"], eimg, gimg, d["eb"], d["bg"], d["bc"], steps, fmt=fmt)
    out, saved = pkg.ops.dense_propagate_save(d["h0"], d["A"], eimg, gimg, d["eb"], d["bg"], d["bc"], steps, fmt=fmt)
    assert torch.equal(out, plain)
    assert saved.shape == (6, steps, b * v, D)
    assert torch.equal(saved[0, 0], d["h0"].reshape(b * v, D))
    t = _t64(x)
    with torch.no_grad():
        want_out, inter = _twin(t, steps)
        ref = oracle_torch.dense_propagate(t["h0"], t["A"], t["W"], None if t["eb"] is None else t["eb"].reshape(E, 1, D),
                                           {k: t[k] for k in ("Wg", "bg", "Wc", "bc")}, steps)
    assert float((want_out - ref).abs().max()) < 1e-12                     # the twin IS the oracle's dense_propagate
    np.testing.assert_allclose(out.cpu().numpy(), want_out.numpy(), atol=1e-5, rtol=1e-4)
    for k, name in enumerate(("h", "x", "r", "u", "c", "rh")):
        for s in range(steps):
            w = inter[s][name].numpy()
            np.testing.assert_allclose(saved[k, s].cpu().numpy(), w, atol=1e-5, rtol=1e-4, err_msg="%s step %d" % (name, s))
    again = pkg.ops.dense_propagate_save(d["h0"], d["A"], eimg, gimg, d["eb"], d["bg"], d["bc"], steps, fmt=fmt)
    assert torch.equal(again[0], out) and torch.equal(again[1], saved)


def _errors(got, want):
    """{name: (normwise, max-abs relative to max |want|)} -- train_reference.normwise_errors."""
    return TR.normwise_errors(got, want)


def _yardstick(pkg, x, steps, cuda):
    """Today's route on the same inputs: backward.PropagationStepFn once per timestep on the sparse form of A (as
    DenseGGNNChemModel._compute_for_training derives it), through torch.autograd -> d_h0 and the variables' gradients."""
    from importlib import import_module
    autograd = import_module(pkg.__name__ + ".autograd")
    sparse_model = import_module(pkg.__name__ + ".sparse_model")
    b, v, D = x["h0"].shape
    E0 = E = x["W"].shape[0]
    if E % 4:
        # today's route takes the edge biases' gradient on ggnn_xty_f32, which has no kernel for E % 4 != 0 columns (the models have
        # 4 or 8 edge types): the same function with the types padded to a multiple of 4 by types that carry no edge
        E = (E + 3) // 4 * 4
        pad = lambda a, axis: None if a is None else np.concatenate(
            [a, np.zeros(a.shape[:axis] + (E - E0,) + a.shape[axis + 1:], a.dtype)], axis=axis)
        x = dict(x, A=pad(x["A"], 1), W=pad(x["W"], 0), eb=pad(x["eb"], 0))
    d = _dev(x, cuda)
    A = d["A"]
    nz = A.nonzero()
    base = nz[:, 0] * v
    pairs = torch.stack([base + nz[:, 3], base + nz[:, 2]], dim=1).to(torch.int32)
    lists = [pairs[nz[:, 1] == t].contiguous() for t in range(E)]
    nin = (A != 0).sum(dim=3).permute(0, 2, 1).reshape(b * v, E).to(torch.float32).contiguous()
    index = pkg.ops.build_message_index(lists, b * v)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("h0", "W", "eb", "Wg", "bg", "Wc", "bc") if d[k] is not None}
    cell = sparse_model.GRUCellWeights(leaves["Wg"], leaves["bg"], leaves["Wc"], leaves["bc"])
    h = leaves["h0"].reshape(b * v, D)
    for _ in range(steps):
        h = autograd.propagation_step(h, index, nin, leaves["W"], leaves.get("eb"), False, [], cell, "tanh", need_grad=True, ew_mask=None)
    (h.reshape(b, v, D) * d["d_out"]).sum().backward()
    torch.cuda.synchronize()
    return {("d_h0" if k == "h0" else k): (t.grad[:E0] if k in ("W", "eb") else t.grad).detach().cpu() for k, t in leaves.items()}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("b,v,E,D,bias,steps", SHAPES)
def test_backward_kernel_against_fp64(pkg, oracle, cuda, b, v, E, D, bias, steps, weighted):
    """ggnn_dense_propagate_bwd_f32 against float64 autograd of the twin on the kernel's own fp32 inputs (saved tensors from the
    saving launch in the exact format, a random d_out; every case has a graph without edges, `weighted` scales the edges into (0, 2)).

    1. The formulas of the kernel's header, evaluated in float64, equal float64 autograd to 1e-12 (relative to each tensor's max).
    2. Yardstick: today's per-timestep route (PropagationStepFn on the sparse form, through torch.autograd) on the same inputs,
       measured against float64 per tensor it exposes (d_h0 and the six variables' gradients): normwise and max-abs relative error.
       The sparse form cannot carry edge weights, so for the weighted cases the yardstick runs on the 0/1 PATTERN of A against its own
       float64 reference: their bound is BORROWED from that neighbouring problem (same shape, weights, states and d_out).  For
       E % 4 != 0 the yardstick pads the edge types to a multiple of 4 with types that carry no edge (_yardstick).
    3. Bound for EVERY tensor of the new route (d_h0, stacked dpc / dpg / dx / dM, and the variables' gradients of
       DensePropagateFn): twice the worst value so measured, normwise and max-abs separately.  Both routes are exact-format f32 chains
       that differ in summation order; a dropped term or a wrong operand is an error of order 1.

    Measured on an MI355X (worst tensor, normwise / max-abs; profiles/dense_train_accuracy.json has every tensor -- this test writes
    it when GGNN_DENSE_TRAIN_ACCURACY_JSON names a file):
        shape (b, v, E, D, steps)  A      yardstick (per-timestep route)   backward launch      variables (DensePropagateFn)
        256, 29, 4, 100, 4         0/1    2.8e-6 / 2.2e-6                  6.1e-7 / 7.4e-7      1.2e-6 / 9.0e-7
        256, 29, 4, 100, 4         (0,2)  2.7e-6 / 2.3e-6                  7.0e-7 / 1.2e-6      1.5e-6 / 1.4e-6
        7, 29, 4, 100, 4           0/1    6.7e-7 / 7.4e-7                  6.2e-7 / 6.8e-7      5.3e-7 / 5.2e-7
        7, 29, 4, 100, 4           (0,2)  6.5e-7 / 6.9e-7                  7.0e-7 / 1.0e-6      6.3e-7 / 7.4e-7
        5, 17, 8, 64, 3            0/1    6.9e-7 / 9.7e-7                  7.3e-7 / 9.1e-7      7.4e-7 / 7.8e-7
        5, 17, 8, 64, 3            (0,2)  8.1e-7 / 9.8e-7                  8.6e-7 / 9.5e-7      8.4e-7 / 9.3e-7
        4, 5, 2, 32, 4             0/1    3.0e-7 / 5.2e-7                  3.3e-7 / 4.1e-7      3.0e-7 / 3.2e-7
        4, 5, 2, 32, 4             (0,2)  3.4e-7 / 4.0e-7                  3.0e-7 / 4.5e-7      3.2e-7 / 3.3e-7
        3, 32, 4, 100, 2           0/1    5.0e-7 / 7.2e-7                  4.6e-7 / 4.9e-7      4.2e-7 / 5.7e-7
        3, 32, 4, 100, 2           (0,2)  5.1e-7 / 6.8e-7                  5.1e-7 / 7.6e-7      4.9e-7 / 5.4e-7
        1, 1, 4, 100, 2            0/1    4.0e-7 / 4.5e-7                  3.2e-7 / 3.2e-7      3.2e-7 / 2.6e-7
        1, 1, 4, 100, 2            (0,2)  4.0e-7 / 6.3e-7                  2.6e-7 / 3.2e-7      1.9e-7 / 3.0e-7
        3, 9, 6, 64, 2             0/1    4.8e-7 / 6.3e-7                  5.4e-7 / 7.1e-7      5.4e-7 / 9.5e-7
        3, 9, 6, 64, 2             (0,2)  5.1e-7 / 5.7e-7                  6.0e-7 / 1.1e-6      6.2e-7 / 5.6e-7
        2, 20, 6, 32, 3            0/1    4.2e-7 / 5.4e-7                  4.4e-7 / 5.5e-7      4.0e-7 / 6.3e-7
        2, 20, 6, 32, 3            (0,2)  4.5e-7 / 5.9e-7                  5.0e-7 / 5.2e-7      5.1e-7 / 5.1e-7
    (2, 16, 6, 100, 1) is refused by the route (_assert_refused) and has no figures."""
    x = _inputs(oracle, b, v, E, D, bias, steps, weighted=weighted)
    if not _supported(pkg, v, E, D):
        return _assert_refused(pkg, x, cuda, steps)
    want, want_var, inter, _, _ = _fp64_gradients(x, steps)
    form = _formulas(x, inter, steps)
    for k, w in want.items():
        assert float((form[k].reshape(w.shape) - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), k

    # the yardstick on the same inputs (weighted: the 0/1 pattern and its own float64 reference)
    xy = dict(x, A=(x["A"] != 0).astype(np.float32)) if weighted else x
    if weighted:
        wy, wy_var, _, _, _ = _fp64_gradients(xy, steps)
    else:
        wy, wy_var = want, want_var
    yard = _errors(_yardstick(pkg, xy, steps, cuda), dict(wy_var, d_h0=wy["d_h0"]))
    worst_norm = max(e[0] for e in yard.values())
    worst_abs = max(e[1] for e in yard.values())

    d = _dev(x, cuda)
    P, eimg, gimg = _images(pkg, d)
    _, saved = pkg.ops.dense_propagate_save(d["h0"], d["A"], eimg, gimg, d["eb"], d["bg"], d["bc"], steps)
    bimg = P.dense_bwd(d["W"], d["Wg"], d["Wc"])
    names = ("d_h0", "dpc", "dpg", "dx", "dM")
    got = dict(zip(names, pkg.ops.dense_propagate_bwd(d["d_out"], d["A"], bimg, saved)))
    again = pkg.ops.dense_propagate_bwd(d["d_out"], d["A"], bimg, saved)
    for k, t in zip(names, again):
        assert torch.equal(t, got[k]), k                                   # no atomics: the same bits
    assert pkg.ops.dense_propagate_bwd(d["d_out"], d["A"], bimg, saved, need_d_h0=False)[0] is None
    new = _errors({k: t.cpu() for k, t in got.items()}, want)

    # the variables' gradients through DensePropagateFn (returned to autograd: no sink is open)
    from importlib import import_module
    Fn = import_module(pkg.__name__ + ".backward").DensePropagateFn
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("h0", "W", "eb", "Wg", "bg", "Wc", "bc") if d[k] is not None}
    nin = d["A"].sum(dim=3).permute(0, 2, 1).reshape(b * v, E).contiguous() if bias else None
    out = Fn.apply(leaves["h0"], d["A"], nin, leaves["W"], leaves.get("eb"), leaves["Wg"], leaves["bg"], leaves["Wc"], leaves["bc"], steps, 3)
    (out * d["d_out"]).sum().backward()
    torch.cuda.synchronize()
    new_var = _errors({k: t.grad.cpu() for k, t in leaves.items() if k != "h0"}, want_var)
    assert torch.equal(leaves["h0"].grad, got["d_h0"])

    key = "b%d_v%d_E%d_D%d_bias%d_steps%d_%s" % (b, v, E, D, bias, steps, "weighted" if weighted else "01")
    ACCURACY[key] = {"yardstick_per_timestep_route": yard, "graph_resident_kernel": new, "graph_resident_variables": new_var,
                     "bound": {"normwise": 2 * worst_norm, "max_abs": 2 * worst_abs}}
    print(key, json.dumps(ACCURACY[key]))
    path = os.environ.get("GGNN_DENSE_TRAIN_ACCURACY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(ACCURACY, f, indent=1, sort_keys=True)
    for k, (en, ea) in list(new.items()) + list(new_var.items()):
        assert en <= 2 * worst_norm and ea <= 2 * worst_abs, (k, en, ea, worst_norm, worst_abs)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _model(pkg, ms, cuda, **config):
    cfg = {"batch_size": 16, "random_seed": 5}
    cfg.update(config)
    return pkg.DenseGGNNChemModel({"--quiet": True, "--device": str(cuda), "train_data": ms, "valid_data": ms, "--config": json.dumps(cfg)})


def _randomise(model, oracle, seed=0):
    """Weights with non-zero biases everywhere (the fresh model's edge biases are zero, its gate biases one)."""
    rng = np.random.default_rng(seed)
    D, T = model.params["hidden_size"], model.num_edge_types
    gru = {"Wg": oracle.glorot_init(rng, [2 * D, 2 * D]), "bg": (1 + rng.normal(0, 0.1, 2 * D)).astype(np.float32),
           "Wc": oracle.glorot_init(rng, [2 * D, D]), "bc": rng.normal(0, 0.1, D).astype(np.float32)}
    model.set_graph_weights(oracle.glorot_init(rng, [T, D, D]), rng.normal(0, 0.1, [T, 1, D]).astype(np.float32), gru)


def _fp64_step(oracle_torch, model, feed):
    """Loss and every variable's gradient of one training step in float64: the twin, the gated readout on the real vertices
    (chem_tensorflow_dense.py:119-129) and the task losses (chem_tensorflow.py:161-169)."""
    nv = {n: t.detach().cpu().double().requires_grad_(True) for n, t in model.named_variables().items()}
    f = lambda t: t.detach().cpu().double()
    h0, A = f(feed["initial_node_representation"]), f(feed["adjacency_matrix"])
    b, v, D = h0.shape
    E = A.shape[1]
    base = "graph_model/gru_scope/gru_cell"
    eb = nv["graph_model/Variable_1:0"].reshape(E, D) if model.params["use_edge_bias"] else None
    x = dict(h0=h0, A=A, W=nv["graph_model/Variable:0"].reshape(E, D, D), eb=eb, Wg=nv[base + "/gates/kernel:0"],
             bg=nv[base + "/gates/bias:0"], Wc=nv[base + "/candidate/kernel:0"], bc=nv[base + "/candidate/bias:0"])
    last, _ = _twin(x, model.params["num_timesteps"])
    real = f(feed["node_mask"]).reshape(-1).nonzero()[:, 0]
    gnl = torch.arange(b).repeat_interleave(v)[real]
    targets, tmask = f(feed["target_values"]), f(feed["target_mask"])
    loss = 0.0
    for i, task in enumerate(model.params["task_ids"]):
        w = [nv["out_layer_task%i/%s:0" % (task, n)] for n in ("regression_gate/MLP_W_layer0", "regression_gate/MLP_b_layer0",
                                                                "regression/MLP_W_layer0", "regression/MLP_b_layer0")]
        pred = oracle_torch.gated_regression(last.reshape(b * v, D)[real], h0.reshape(b * v, D)[real], gnl, b, *w)
        loss = loss + oracle_torch.task_loss(pred, targets[i], tmask[i])[0]
    loss.backward()
    return float(loss), {n: t.grad for n, t in nv.items()}


class _Recorder:
    """Names of the launches ops._launch issues, and the calls of Tensor.nonzero, within the block."""

    def __init__(self, pkg, monkeypatch):
        self.names, self.nonzero = [], 0
        self.saves = lambda: sum(n.startswith("dense_propagate_save") for n in self.names)    # forward launches of the new route
        original, nz = pkg.ops._launch, torch.Tensor.nonzero

        def launch(name, fn):
            self.names.append(name)
            return original(name, fn)

        def nonzero(t, *a, **k):
            self.nonzero += 1
            return nz(t, *a, **k)

        monkeypatch.setattr(pkg.ops, "_launch", launch)
        monkeypatch.setattr(torch.Tensor, "nonzero", nonzero)


@pytest.mark.parametrize("config", [{}, {"use_edge_bias": False, "hidden_size": 64, "task_ids": [0, 1]}])
def test_step_gradients_against_fp64(pkg, oracle, oracle_torch, cuda, monkeypatch, config):
    """One train_batch of a model with the key set: every variable's gradient as the optimiser consumes it (the edge biases included)
    against float64 at the 2e-4 bound of the other step tests, the loss within 1e-5 relative; the graph-resident launches ran, and the
    step enqueued no A.nonzero() and no per-timestep propagation launch."""
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5, num_tasks=2)
    m = _model(pkg, ms, cuda, graph_resident_training=True, **config)
    _randomise(m, oracle)
    feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
    want_loss, want = _fp64_step(oracle_torch, m, feed)
    rec = _Recorder(pkg, monkeypatch)
    with TR.capture_step_gradients(m) as steps:
        loss = float(m.train_batch(feed))
    assert rec.saves() == 1                                                # not a silent fallback
    T = m.params["num_timesteps"]
    assert "dense_propagate_save[steps=%d]" % T in rec.names and "dense_propagate_bwd[steps=%d]" % T in rec.names
    assert rec.nonzero == 0
    assert not [n for n in rec.names if n.startswith(("gru", "msg_transform", "gather_segment_sum", "dense_aggregate"))], rec.names
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
    got = steps[0]
    assert set(got) == set(want) and ("graph_model/Variable_1:0" in got) == m.params["use_edge_bias"]
    TR.assert_gradients_match(got, want)
    # assert_comparison_has_teeth looks for the sparse model's edge-weight name and a [rows, D] gradient: give the dense variable both
    ew = "graph_model/Variable:0"
    D = m.params["hidden_size"]
    alias = lambda g: {(k + " /gnn_edge_weights_0" if k == ew else k): (t.reshape(-1, D) if k == ew else t) for k, t in g.items()}
    TR.assert_comparison_has_teeth(alias(got), alias(want))


def _seeded_steps(pkg, oracle, cuda, ms, n, **config):
    m = _model(pkg, ms, cuda, **config)
    _randomise(m, oracle, seed=1)
    np.random.seed(11)
    feeds = list(m.make_minibatch_iterator(m.train_data, True))[:n]
    with TR.capture_step_gradients(m) as steps:
        losses = [float(m.train_batch(f)) for f in feeds]
    return losses, steps, {k: t.detach().clone() for k, t in m.named_variables().items()}


def _assert_same_bits(a, b):
    assert a[0] == b[0]
    for sa, sb in zip(a[1], b[1]):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_seeded_step_is_deterministic(pkg, oracle, cuda, monkeypatch):
    ms = pkg.synthetic_qm9(200, mean_nodes=12, seed=5)
    rec = _Recorder(pkg, monkeypatch)
    runs = [_seeded_steps(pkg, oracle, cuda, ms, 3, graph_resident_training=True) for _ in range(2)]
    assert rec.saves() == 6
    _assert_same_bits(*runs)


@pytest.mark.parametrize("config", [{"hidden_size": 128}, {"bucket": 40}, {"edge_weight_dropout_keep_prob": 0.8},
                                    {"graph_state_keep_prob": 0.9}])
def test_unsupported_batches_take_todays_route(pkg, oracle, cuda, monkeypatch, config):
    """With the key set but no graph-resident kernels for the batch (hidden size 128, a bucket of 40 vertices) or dropout on the
    propagation (either keep-prob placeholder below 1), a seeded step equals the step of a model without the key bit for bit."""
    ms = pkg.synthetic_qm9(120, mean_nodes=12, seed=6)
    cfg = {k: v for k, v in config.items() if k == "hidden_size"}

    def run(**extra):
        m = _model(pkg, ms, cuda, **cfg, **extra)
        _randomise(m, oracle, seed=2)
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
    with_key = run(graph_resident_training=True)
    assert rec.saves() == 0 and rec.names
    _assert_same_bits(with_key, run())


@pytest.mark.parametrize("case", [c for c in RG.DENSE_CASES if len(RG.Golden(c).train_losses)])
def test_training_follows_reference_run_on_the_new_route(pkg, cuda, tmp_path, monkeypatch, case):
    """tests/test_gpu_reference_golden.py::test_training_follows_reference_run for the dense cases, with the key added to the config:
    the same tolerances, copied."""
    g = RG.Golden(case)
    path = g.write_checkpoint(str(tmp_path / ("%s.pickle" % g.case)))
    with open(path, "rb") as f:
        ckpt = pickle.load(f)
    ckpt["params"] = dict(ckpt["params"], graph_resident_training=True)    # restoring asserts the params key for key (chem_model.py:484):
    with open(path, "wb") as f:                                            # the checkpoint of a run WITH the key carries the key
        pickle.dump(ckpt, f)
    args = g.model_args(str(cuda), **{"--restore": path})
    args["--config"] = json.dumps(dict(g.params, graph_resident_training=True))
    m = pkg.DenseGGNNChemModel(args)
    for n, t in m.named_variables().items():
        np.testing.assert_array_equal(t.detach().cpu().numpy().reshape(g.weights[n].shape), g.weights[n])
    batches = list(m.make_minibatch_iterator(m.train_data, False))
    assert len(batches) == int(g.z["num_train_batches"])
    rec = _Recorder(pkg, monkeypatch)
    losses = [float(m.train_batch(batches[s % len(batches)])) for s in range(len(g.train_losses))]
    assert rec.saves() == len(g.train_losses)
    np.testing.assert_allclose(losses, g.train_losses, rtol=5e-4)
    nv = m.named_variables()
    for i, n in enumerate(g.names):
        a = nv[n].detach().cpu().numpy()
        np.testing.assert_allclose(RG.stats(a), g.z["trained_stats"][i], rtol=1e-3, atol=5e-3, err_msg=n)
        if "trained/" + n in g.z.files:
            np.testing.assert_allclose(a.reshape(g.z["trained/" + n].shape), g.z["trained/" + n], rtol=1e-2, atol=3e-3, err_msg=n)


def _train_loop(pkg, cuda, g, log_dir, **extra):
    params = dict(g.params, graph_resident_training=True, **extra)
    m = pkg.DenseGGNNChemModel({"--device": str(cuda), "--log_dir": str(log_dir), "--config": json.dumps(params),
                                "train_data": g.train_molecules, "valid_data": g.valid_molecules})
    log = m.train()
    with open(m.best_model_file, "rb") as f:
        return log, pickle.load(f)


def test_train_loop_reproduces_reference_log_on_the_new_route(pkg, cuda, tmp_path, monkeypatch):
    """test_train_loop_reproduces_reference_log for loop_dense with the key added: the same tolerances, copied; the checkpoint's
    params are the fixture's plus the key."""
    g = RG.GoldenLoop("loop_dense")
    rec = _Recorder(pkg, monkeypatch)
    log, best = _train_loop(pkg, cuda, g, tmp_path)
    assert rec.saves() > 0
    assert len(log) == len(g.z["train_loss"])
    np.testing.assert_allclose([e["train_results"][0] for e in log], g.z["train_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][1] for e in log], g.z["train_accuracy"], rtol=1e-3)
    np.testing.assert_allclose([e["train_results"][2] for e in log], g.z["train_error_ratio"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][0] for e in log], g.z["valid_loss"], rtol=1e-3)
    np.testing.assert_allclose([e["valid_results"][1] for e in log], g.z["valid_accuracy"], rtol=1e-3)
    assert best["params"] == dict(g.params, graph_resident_training=True)
    assert (best["train_step"], best["valid_step"]) == (int(g.z["best_train_step"]), int(g.z["best_valid_step"]))
    assert set(best["weights"]) - {"ggnn_amd/adam_step:0"} == set(g.best_names)
    for i, n in enumerate(g.best_names):
        a = np.asarray(best["weights"][n], dtype=np.float64)
        ref = g.z["best_stats"][i]
        np.testing.assert_allclose(RG.stats(a)[1:], ref[1:], rtol=2e-3, atol=1e-6, err_msg=n)
        assert abs(RG.stats(a)[0] - ref[0]) <= 2e-3 * max(ref[1], 1e-3), n


def test_device_packing_equals_host_packing_on_the_new_route(pkg, cuda, tmp_path, monkeypatch):
    """pack_on_device and the key both set: the seeded three-epoch train() prints the same log and saves the same checkpoint as host
    packing with the key set, bit for bit."""
    g = RG.GoldenLoop("loop_dense")
    rec = _Recorder(pkg, monkeypatch)
    (log_h, best_h), (log_d, best_d) = (_train_loop(pkg, cuda, g, tmp_path / str(dev), pack_on_device=dev) for dev in (False, True))
    assert rec.saves() > 0
    assert len(log_d) == len(log_h) == len(g.z["train_loss"])
    for eh, ed in zip(log_h, log_d):
        for part in ("train_results", "valid_results"):
            assert float(eh[part][0]) == float(ed[part][0]), part
            np.testing.assert_array_equal(np.asarray(eh[part][1]), np.asarray(ed[part][1]))
            np.testing.assert_array_equal(np.asarray(eh[part][2]), np.asarray(ed[part][2]))
    assert set(best_h["weights"]) == set(best_d["weights"])
    for n in best_h["weights"]:
        assert np.asarray(best_h["weights"][n]).tobytes() == np.asarray(best_d["weights"][n]).tobytes(), n
