"""Host-side checks (no GPU) of the native training step with propagation attention: the new C symbols (the source-side backward
kernel, the two launch sequences and their workspace function; include/ggnn_hip.h), their argument validation before any launch,
and the opt-in value params['compact_attention'] == 'native' on a CPU model (chem_tensorflow_sparse.py:147-149, 170-196 and
chem_tensorflow.py:183-191 are what the step computes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ggnn_attn_bwd_source_compact_f32", "ggnn_sparse_attn_train_workspace_bytes", "ggnn_sparse_attn_train_forward_f32",
       "ggnn_sparse_attn_train_backward_f32"]
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3     # GGNN_E_* (include/ggnn_hip.h)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _err(lib):
    return (lib.ggnn_last_error() or b"").decode()


def test_symbols_are_exported_with_the_declared_signatures(pkg, lib):
    with open(os.path.join(ROOT, "include", "ggnn_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    c_types = {ctypes.c_int: "int", ctypes.c_size_t: "size_t", ctypes.c_int64: "int64_t"}
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
    f = lib.ggnn_sparse_attn_train_workspace_bytes
    base = lib.ggnn_sparse_train_workspace_bytes
    V, D, T, R, steps, M = 1000, 100, 4, 2100, 8, 2300
    n = f(V, D, T, R, steps, M)
    # the default model's layout plus the three per-message coefficient arrays
    assert n >= base(V, D, T, R, steps) + 3 * M * 4
    for bad in ((-1, D, T, R, steps, M), (V, 0, T, R, steps, M), (V, D, 0, R, steps, M), (V, D, T, -1, steps, M),
                (V, D, T, R, 0, M), (V, D, T, R, steps, 0), (V, D, T, R, steps, -5), (V, D, T, R, steps, 1 << 31)):
        assert f(*bad) == 0, bad
    # grows with the timesteps, the nodes, the compact rows (and the messages): a caller may size once for its largest batch
    assert f(V, D, T, R, steps + 1, M) > n and f(V + 1, D, T, R, steps, M) > n and f(V, D, T, R + 64, steps, M) > n
    assert f(V, D, T, R, steps, M + 64) > n
    for axis in range(4):
        prev = 0
        for x in list(range(1, 40)) + [64, 100, 129, 255, 256, 257, 300, 5000]:
            arg = [V, R, steps, M]
            arg[axis] = x
            got = f(arg[0], D, T, arg[1], arg[2], arg[3])
            assert got >= prev > -1 and got % 256 == 0, (axis, x)
            prev = got


def _buf(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 512)
    base = (ctypes.addressof(raw) + 255) & ~255
    return raw, base


def test_argument_validation_without_a_launch(lib):
    """Every refusal comes back as an error code with ggnn_last_error set before anything touches the device (the pointers are host
    memory: a launch would fault)."""
    keep, p = _buf(4096)
    V, D = 10, 32
    src = lambda **kw: lib.ggnn_attn_bwd_source_compact_f32(
        kw.get("d", p), kw.get("h", p), kw.get("node_ptr", p), p, p, kw.get("slot_row", p), kw.get("coef_a", p), kw.get("coef_s", p),
        kw.get("dHc", p), kw.get("dh", p), kw.get("V", V), kw.get("D", D), None)
    assert src(d=None) == E_INVALID and "null" in _err(lib)
    assert src(node_ptr=None) == E_INVALID and "null" in _err(lib)
    assert src(slot_row=None) == E_INVALID and src(coef_a=None) == E_INVALID and src(dHc=None) == E_INVALID
    assert src(h=None) == E_INVALID and "dh" in _err(lib)              # h and coef_s come with dh
    assert src(coef_s=None) == E_INVALID and "dh" in _err(lib)
    assert src(d=p + 4) == E_INVALID and "align" in _err(lib)
    assert src(dh=p + 8) == E_INVALID and "align" in _err(lib)
    assert src(D=6) == E_INVALID and "bad sizes" in _err(lib)
    assert src(V=-1) == E_INVALID and _err(lib)
    assert src(D=260) == E_UNSUPPORTED and "up to 256" in _err(lib)
    assert src(V=0, d=None, dHc=None, node_ptr=None) == 0               # no nodes: a no-op

    T, M, L = 4, 20, 2
    lt = (ctypes.c_int32 * L)(2, 1)
    rp = (ctypes.c_int32 * (L + 1))(0, 0, 1)
    ri = (ctypes.c_int32 * 1)(0)
    tro = (ctypes.c_int64 * (T + 1))(0, 4, 8, 10, 12)
    mto = (ctypes.c_int64 * (T + 1))(0, 5, 10, 15, 20)
    arr = (ctypes.c_void_p * L)(p, p)
    wsb = lib.ggnn_sparse_attn_train_workspace_bytes(V, D, T, 12, 3, M)
    assert wsb > 0
    off = ctypes.c_int64(-1)
    fwd = lambda **kw: lib.ggnn_sparse_attn_train_forward_f32(
        kw.get("h0", p), kw.get("V", V), kw.get("D", D), T, kw.get("M", M), p, kw.get("slot_pair", p), kw.get("slot_row", p), p,
        kw.get("tro", tro), p, 1, L, lt, rp, ri, arr, kw.get("factors", arr), arr, arr, arr, 0, kw.get("ws", p),
        kw.get("ws_bytes", wsb), ctypes.byref(off), None)
    assert fwd(h0=None) == E_INVALID and "null" in _err(lib)
    assert fwd(slot_pair=None) == E_INVALID and "null" in _err(lib)
    assert fwd(slot_row=None) == E_INVALID and fwd(factors=None) == E_INVALID
    assert fwd(ws=None) == E_INVALID and _err(lib)
    assert fwd(ws=p + 16) == E_INVALID and "align" in _err(lib)
    assert fwd(M=0) == E_INVALID and "message" in _err(lib)
    assert fwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert fwd(tro=(ctypes.c_int64 * (T + 1))(0, 0, 0, 0, 0)) == E_INVALID and "no messages" in _err(lib)
    assert fwd(D=128) == E_UNSUPPORTED and "128" in _err(lib)
    assert fwd(D=6) == E_INVALID
    assert off.value == -1                                            # nothing ran

    bwd = lambda **kw: lib.ggnn_sparse_attn_train_backward_f32(
        kw.get("h0", p), V, kw.get("D", D), T, kw.get("M", M), p, p, p, kw.get("msg_perm", p), kw.get("mto", mto), p, tro, p, 1, L, lt, rp,
        ri, kw.get("src_node_ptr", p), p, p, kw.get("src_row", p), p, p, None, p, kw.get("edge_packed", arr), arr, arr, arr, 0, arr,
        kw.get("g_attn", arr), arr, arr, arr, arr, kw.get("d_final", p), arr, kw.get("ws", p), kw.get("ws_bytes", wsb), None, None)
    assert bwd(h0=None) == E_INVALID and "null" in _err(lib)
    assert bwd(msg_perm=None) == E_INVALID and "null" in _err(lib)
    assert bwd(mto=None) == E_INVALID and bwd(src_node_ptr=None) == E_INVALID and bwd(src_row=None) == E_INVALID
    assert bwd(edge_packed=None) == E_INVALID and bwd(g_attn=None) == E_INVALID and bwd(d_final=None) == E_INVALID
    assert bwd(ws=None) == E_INVALID and _err(lib)
    assert bwd(ws=p + 16) == E_INVALID and "align" in _err(lib)
    assert bwd(M=-3) == E_INVALID and "message" in _err(lib)
    assert bwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert bwd(D=128) == E_UNSUPPORTED and _err(lib)
    del keep


def test_ops_wrapper_refuses_cpu_tensors(pkg):
    V, D, M = 4, 32, 5
    z = torch.zeros(V, D)
    sni = pkg.ops.SegmentIndex(torch.zeros(V + 1, dtype=torch.int32), torch.zeros(M, dtype=torch.int32), V,
                               torch.zeros(M, dtype=torch.int32))
    with pytest.raises(TypeError) as e:
        pkg.ops.attn_backward_source_compact(z, z, sni, torch.zeros(M, dtype=torch.int32), 3, torch.zeros(M), torch.zeros(M), z.clone())
    assert "no CPU implementation" in str(e.value)


def _cpu_model(pkg, ms, **config):
    cfg = {"use_propagation_attention": True, "pack_on_device": False}
    cfg.update(config)
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": cfg})


def test_native_is_a_value_of_the_existing_key(pkg):
    assert "compact_attention" not in pkg.SparseGGNNChemModel.default_params()
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    m = _cpu_model(pkg, ms, compact_attention="native")
    assert m.params["compact_attention"] == "native"
    assert not m.attention_route() and not pkg.train_native.attn_model_eligible(m)       # a CPU model: no HIP route, no native step
    feed = {"initial_node_representation": torch.zeros(6, 100), "num_graphs": 1, "graph_nodes_sorted": True}
    assert not pkg.train_native.attn_eligible(m, feed) and not pkg.train_native.eligible(m, feed)      # (the model decides: no batch can)
    assert m.threaded_batches_default() is True
    m.device = torch.device("cuda:0")                       # (the route's device condition alone; nothing runs)
    assert m.attention_route()                              # any truthy value turns the compacted route on
    # neither is a model without the key, or with the key True, or without attention, wherever it lives
    for cfg in ({}, {"compact_attention": True}, {"compact_attention": False},
                {"compact_attention": "native", "use_propagation_attention": False}):
        assert not pkg.train_native.attn_model_eligible(_cpu_model(pkg, ms, **cfg)), cfg


def test_cpu_model_with_native_takes_the_route_of_one_without_the_key(pkg):
    """With the key 'native' a CPU model is dispatched exactly like one with the key True or without it.  This package has no CPU
    implementation of the hot path, so on a CPU model that route ends in the same TypeError of the same op for all three, before
    any weight is touched: the seeded weights stay equal bit for bit.  The comparison of a completed step runs where a step can
    complete: the fall-back test of tests/test_gpu_attention_native.py."""
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)

    def run(**extra):
        np.random.seed(7)
        m = _cpu_model(pkg, ms, **extra)
        before = {k: t.detach().clone() for k, t in m.named_variables().items()}
        np.random.seed(9)
        with pytest.raises(TypeError) as e:
            feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
            assert not pkg.train_native.attn_eligible(m, feed)
            m.train_batch(feed)
        after = {k: t.detach().clone() for k, t in m.named_variables().items()}
        for k in before:
            assert torch.equal(before[k], after[k]), k
        return str(e.value), after

    (ea, wa), (eb, wb), (ec, wc) = run(compact_attention="native"), run(compact_attention=True), run()
    assert ea == eb == ec and "no CPU implementation" in ea
    assert set(wa) == set(wb) == set(wc)
    for k in wa:
        assert torch.equal(wa[k], wb[k]) and torch.equal(wa[k], wc[k]), k
