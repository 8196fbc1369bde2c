"""Host-side checks (no GPU) of the dense model's native training step: the five new C symbols (edge-weight / edge-bias gradient
kernel, the two launch sequences and their workspace functions; include/ggnn_hip.h), their argument validation before any launch,
and the opt-in value params['graph_resident_training'] == 'native' on a CPU model (chem_tensorflow_dense.py:93-117 and
chem_tensorflow.py:183-191 are what the step computes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ggnn_dense_edge_grad_workspace_bytes", "ggnn_dense_edge_grad_f32", "ggnn_dense_train_workspace_bytes",
       "ggnn_dense_train_forward_f32", "ggnn_dense_train_backward_f32"]
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3     # GGNN_E_* (include/ggnn_hip.h)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _err(lib):
    return (lib.ggnn_last_error() or b"").decode()


def test_symbols_are_exported_with_the_declared_signatures(pkg, lib):
    with open(os.path.join(ROOT, "include", "ggnn_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    c_types = {ctypes.c_int: "int", ctypes.c_size_t: "size_t"}
    for name in NEW:
        assert hasattr(lib, name), name
        restype, argtypes = pkg._lib.SYMBOLS[name]
        assert getattr(lib, name).argtypes == argtypes
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert m.group(1) == c_types[restype]
        args = [a.strip() for a in m.group(2).split(",")]
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):
            if t in c_types:
                assert a.split()[0] == c_types[t] and "*" not in a, (name, a)
            else:                                                       # pointers and streams
                assert "*" in a or a.startswith("ggnn_stream_t"), (name, a)
    assert lib.ggnn_abi_version() == pkg._lib.ABI_VERSION == 3            # additions only


def test_workspace_sizing(lib):
    f = lib.ggnn_dense_train_workspace_bytes
    for b, v, E, D, steps in ((256, 29, 4, 100, 4), (1, 1, 2, 32, 1), (7, 17, 8, 64, 3), (16, 16, 6, 64, 4)):
        n = f(b, v, E, D, steps)
        rows = steps * b * v
        stacked = rows * D * 4 * (1 + 2 + 1 + E)                          # dpc, dpg, dx, dM
        assert n >= lib.ggnn_dense_train_saved_bytes(b, v, D, steps) + stacked + b * v * D * 4
        assert n >= lib.ggnn_dense_edge_grad_workspace_bytes(rows, E, D)
    # non-decreasing in b, v and steps, one at a time (a caller may size once for its largest batch)
    for E, D in ((4, 100), (8, 64), (2, 32)):
        for fixed in ((1, 29, 4), (256, 1, 4), (256, 29, 1)):
            for axis in range(3):
                prev = 0
                for x in list(range(1, 40)) + [64, 100, 129, 255, 256, 257, 300]:
                    if axis == 1 and x > 32:
                        break
                    arg = list(fixed)
                    arg[axis] = x
                    n = f(arg[0], arg[1], E, D, arg[2])
                    assert n >= prev > -1, (E, D, axis, x)
                    prev = n
    g = lib.ggnn_dense_edge_grad_workspace_bytes
    prev = 0
    for N in range(0, 9000, 7):
        assert g(N, 4, 100) >= prev
        prev = g(N, 4, 100)


def _buf(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 512)
    base = (ctypes.addressof(raw) + 255) & ~255
    return raw, base


def test_argument_validation_without_a_launch(lib):
    """Every refusal comes back as an error code with ggnn_last_error set before anything touches the device (the pointers are host
    memory: a launch would fault)."""
    keep, p = _buf(1024)
    N, E, D = 64, 4, 32
    need = lib.ggnn_dense_edge_grad_workspace_bytes(N, E, D)
    eg = lambda **kw: lib.ggnn_dense_edge_grad_f32(
        kw.get("h", p), kw.get("dM", p), kw.get("nin", p), kw.get("dx", p), kw.get("N", N), kw.get("rps", 16), kw.get("E", E), kw.get("D", D),
        kw.get("dW", p), kw.get("db", p), 0, kw.get("ws", p), kw.get("ws_bytes", need), None)
    assert eg(h=None) == E_INVALID and "null" in _err(lib)
    assert eg(dM=None) == E_INVALID and _err(lib)
    assert eg(dW=None) == E_INVALID and _err(lib)
    assert eg(db=None) == E_INVALID and _err(lib)                     # nin without a destination for the bias gradient
    assert eg(dx=None) == E_INVALID and _err(lib)
    assert eg(ws=None) == E_INVALID and _err(lib)
    assert eg(h=p + 4) == E_INVALID and "align" in _err(lib)
    assert eg(rps=0) == E_INVALID and _err(lib)
    assert eg(N=-1) == E_INVALID and _err(lib)
    assert eg(ws_bytes=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    for bad in (dict(D=128), dict(E=3), dict(D=96), dict(E=10)):
        assert eg(**bad) == E_UNSUPPORTED, bad
        assert "32/64/100" in _err(lib) and "{2,4,6,8}" in _err(lib)     # the supported list

    b, v, steps = 2, 5, 2
    wsb = lib.ggnn_dense_train_workspace_bytes(b, v, E, D, steps)
    assert wsb > 0
    off = ctypes.c_int64(-1)
    fwd = lambda **kw: lib.ggnn_dense_train_forward_f32(
        kw.get("h0", p), p, p, p, None, p, p, kw.get("b", b), kw.get("v", v), kw.get("E", E), kw.get("D", D), kw.get("steps", steps), 0,
        kw.get("ws", p), kw.get("ws_bytes", wsb), ctypes.byref(off), None)
    assert fwd(h0=None) == E_INVALID and "null" in _err(lib)
    assert fwd(ws=None) == E_INVALID and _err(lib)
    assert fwd(ws=p + 16) == E_INVALID and "align" in _err(lib)
    assert fwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert fwd(steps=0) == E_INVALID and _err(lib)
    for bad in (dict(D=128), dict(E=3), dict(v=40)):
        assert fwd(**bad) == E_UNSUPPORTED and "v=%d E=%d D=%d" % (bad.get("v", v), bad.get("E", E), bad.get("D", D)) in _err(lib), bad
    assert fwd(b=0, h0=None, ws=None, ws_bytes=0) == 0
    assert off.value == -1                                            # nothing ran

    bwd = lambda **kw: lib.ggnn_dense_train_backward_f32(
        kw.get("d_final", p), p, kw.get("nin", p), p, kw.get("b", b), kw.get("v", v), kw.get("E", E), kw.get("D", D), steps, kw.get("g_W", p),
        kw.get("g_b", p), p, p, kw.get("g_Wc", p), p, kw.get("ws", p), kw.get("ws_bytes", wsb), None, None)
    assert bwd(d_final=None) == E_INVALID and "null" in _err(lib)
    assert bwd(g_W=None) == E_INVALID and _err(lib)
    assert bwd(g_Wc=None) == E_INVALID and _err(lib)
    assert bwd(g_b=None) == E_INVALID and _err(lib)                   # in-degrees and the bias gradient's buffer come together
    assert bwd(nin=None) == E_INVALID and _err(lib)
    assert bwd(ws=None) == E_INVALID and _err(lib)
    assert bwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    for bad in (dict(D=128), dict(E=3), dict(v=40)):
        assert bwd(**bad) == E_UNSUPPORTED and _err(lib), bad
    assert bwd(b=0, d_final=None, ws=None, ws_bytes=0) == 0
    del keep


def test_ops_dense_edge_grad_refuses_cpu_tensors(pkg):
    h, dM = torch.zeros(8, 32), torch.zeros(8, 4 * 32)
    with pytest.raises(ValueError):
        pkg.ops.dense_edge_grad(h, dM)
    with pytest.raises(ValueError):
        pkg.ops.dense_edge_grad(h, dM, nin=torch.zeros(4, 4), dx=torch.zeros(8, 32))
    assert pkg.ops.dense_edge_grad_supported(4, 100) and pkg.ops.dense_edge_grad_supported(8, 64) and pkg.ops.dense_edge_grad_supported(2, 32)
    assert not pkg.ops.dense_edge_grad_supported(3, 100) and not pkg.ops.dense_edge_grad_supported(4, 128)


def _cpu_model(pkg, ms, **config):
    cfg = {"batch_size": 8, "random_seed": 3}
    cfg.update(config)
    return pkg.DenseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": cfg})


def test_native_is_a_value_of_the_existing_key(pkg):
    assert "graph_resident_training" not in pkg.DenseGGNNChemModel.default_params()
    ms = pkg.synthetic_qm9(40, mean_nodes=8, seed=2)
    m = _cpu_model(pkg, ms, graph_resident_training="native")
    assert m.params["graph_resident_training"] == "native"
    assert not pkg.train_native.dense_model_eligible(m)               # a CPU model: no native step
    feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
    assert not pkg.train_native.dense_eligible(m, feed)
    m.feed(feed)
    assert not m._graph_resident_step(int(feed["num_vertices"]), feed["initial_node_representation"], feed["adjacency_matrix"])
    # neither is a model without the key, or with the key True, wherever it lives
    for value in (None, True, False):
        cfg = {} if value is None else {"graph_resident_training": value}
        assert not pkg.train_native.dense_model_eligible(_cpu_model(pkg, ms, **cfg))


def test_cpu_model_with_native_takes_the_route_of_one_without_the_key(pkg):
    """With the key 'native' a CPU model is dispatched exactly like one without the key.  This package has no CPU implementation of
    the hot path (neither the propagation nor the readout MLP's product, ops.gemm), so on a CPU model that route ends in the same
    TypeError of the same op for both, before any weight is touched: the seeded weights stay equal bit for bit.  The comparison of a
    completed step, loss and weights bit for bit, runs where a step can complete: the fallback test of tests/test_gpu_dense_native.py."""
    ms = pkg.synthetic_qm9(40, mean_nodes=8, seed=2)

    def run(**extra):
        np.random.seed(7)
        m = _cpu_model(pkg, ms, **extra)
        before = {k: t.detach().clone() for k, t in m.named_variables().items()}
        np.random.seed(9)
        feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
        assert not pkg.train_native.eligible(m, feed) and not pkg.train_native.dense_eligible(m, feed)
        with pytest.raises(TypeError) as e:
            m.train_batch(feed)
        after = {k: t.detach().clone() for k, t in m.named_variables().items()}
        for k in before:
            assert torch.equal(before[k], after[k]), k
        return str(e.value), after, m.dropout_step

    (ea, wa, sa), (eb, wb, sb) = run(graph_resident_training="native"), run()
    assert ea == eb and "CUDA/HIP" in ea
    assert sa == sb == 1
    assert set(wa) == set(wb)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k
