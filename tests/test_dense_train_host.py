"""Host-side checks (no GPU) of the graph-resident dense training route: the C ABI's new symbols, their shape rules and argument
validation, and the model's opt-in key (chem_tensorflow_dense.py:93-117 is what the route computes; see include/ggnn_hip.h)."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ggnn_dense_train_supported", "ggnn_dense_train_saved_bytes", "ggnn_dense_propagate_save_f32", "ggnn_dense_bwd_packed_bytes",
       "ggnn_dense_bwd_pack_f32", "ggnn_dense_propagate_bwd_f32"]
E_INVALID, E_UNSUPPORTED = -1, -2            # GGNN_E_INVALID, GGNN_E_UNSUPPORTED (include/ggnn_hip.h)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


def _err(lib):
    return (lib.ggnn_last_error() or b"").decode()


def test_symbols_are_exported_with_the_declared_signatures(pkg, lib):
    with open(os.path.join(ROOT, "include", "ggnn_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    c_types = {ctypes.c_int: "int", ctypes.c_size_t: "size_t", ctypes.c_void_p: "*"}
    for name in NEW:
        restype, argtypes = pkg._lib.SYMBOLS[name]
        assert getattr(lib, name).argtypes == argtypes
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert m.group(1) == c_types[restype]
        args = [a.strip() for a in m.group(2).split(",")]
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):
            if t is ctypes.c_void_p:
                assert "*" in a or a.startswith("ggnn_stream_t"), (name, a)
            else:
                assert a.split()[0] == c_types[t] and "*" not in a, (name, a)
    assert lib.ggnn_abi_version() == 3            # additions only


def test_supported_shapes(lib):
    for shape in ((29, 4, 100), (32, 4, 64), (17, 8, 64)):
        assert lib.ggnn_dense_train_supported(*shape) == 1, shape
    for shape in ((33, 4, 100), (29, 3, 100), (29, 4, 128), (0, 4, 100)):
        assert lib.ggnn_dense_train_supported(*shape) == 0, shape
    # never wider than the forward: whatever the split-form forward refuses, training refuses
    for v, E, D in itertools.product((1, 16, 32, 33, 40), (1, 2, 3, 4, 6, 8, 10), (32, 64, 96, 100, 128)):
        if not (lib.ggnn_dense_propagate_supported(v, E, D) and lib.ggnn_dense_propagate_is_split(v, E, D)):
            assert lib.ggnn_dense_train_supported(v, E, D) == 0, (v, E, D)
        assert (lib.ggnn_dense_bwd_packed_bytes(D, E) > 0) == (D in (32, 64, 100))


def test_saved_bytes(lib):
    f = lib.ggnn_dense_train_saved_bytes
    for b, v, D, steps in ((256, 29, 100, 4), (1, 1, 32, 1), (7, 17, 64, 3)):
        n = f(b, v, D, steps)
        assert n >= 6 * steps * b * v * D * 4
        assert f(b + 1, v, D, steps) >= n and f(b, v + 1, D, steps) >= n and f(b, v, D + 4, steps) >= n and f(b, v, D, steps + 1) >= n


def _buf(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 32)
    base = (ctypes.addressof(raw) + 15) & ~15
    return raw, base


def test_argument_validation_without_a_launch(lib):
    """Every refusal comes back as an error code with ggnn_last_error set, before anything touches the device (the pointers are host
    memory: a launch would fault)."""
    b, v, E, D, steps = 2, 5, 4, 32, 2
    keep, p = _buf(64)
    sb = lib.ggnn_dense_train_saved_bytes(b, v, D, steps)
    save = lambda saved, nbytes, **kw: lib.ggnn_dense_propagate_save_f32(
        kw.get("h0", p), p, p, p, None, p, p, p, kw.get("b", b), kw.get("v", v), kw.get("E", E), kw.get("D", D), steps, 0, saved, nbytes, None)
    assert save(None, sb) == E_INVALID and _err(lib)
    assert save(p + 4, sb) == E_INVALID and "align" in _err(lib)
    assert save(p, sb - 1) == E_INVALID and "saved_bytes" in _err(lib)
    assert save(p, sb, h0=None) == E_INVALID and _err(lib)
    assert save(p, sb, h0=p + 4) == E_INVALID and _err(lib)
    for bad in (dict(v=33), dict(E=3), dict(D=128)):
        assert save(p, sb, **bad) == E_UNSUPPORTED and _err(lib), bad
    assert save(None, 0, b=0) == 0

    bwd = lambda **kw: lib.ggnn_dense_propagate_bwd_f32(
        kw.get("d_out", p), p, p, kw.get("saved", p), kw.get("b", b), kw.get("v", v), kw.get("E", E), kw.get("D", D), steps,
        kw.get("d_h0", None), p, kw.get("dpg", p), p, p, None)
    assert bwd(d_out=None) == E_INVALID and _err(lib)
    assert bwd(saved=None) == E_INVALID and _err(lib)
    assert bwd(dpg=p + 8) == E_INVALID and "align" in _err(lib)
    assert bwd(d_h0=p + 4) == E_INVALID and _err(lib)
    for bad in (dict(v=33), dict(E=3), dict(D=128)):
        assert bwd(**bad) == E_UNSUPPORTED and _err(lib), bad
    assert bwd(b=0, d_out=None, saved=None) == 0

    assert lib.ggnn_dense_bwd_pack_f32(None, p, p, E, D, p, None) == E_INVALID and _err(lib)
    assert lib.ggnn_dense_bwd_pack_f32(p, p, p, E, D, p + 4, None) == E_INVALID and _err(lib)
    assert lib.ggnn_dense_bwd_pack_f32(p, p, p, E, 128, p, None) == E_UNSUPPORTED and _err(lib)
    del keep


def test_key_is_not_a_default_param(pkg):
    assert "graph_resident_training" not in pkg.DenseGGNNChemModel.default_params()


def test_cpu_model_with_the_key_builds_and_takes_todays_route(pkg):
    ms = pkg.synthetic_qm9(40, mean_nodes=8, seed=2)
    cfg = {"batch_size": 8, "graph_resident_training": True}
    m = pkg.DenseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": cfg})
    assert m.params["graph_resident_training"] is True
    feed = next(iter(m.make_minibatch_iterator(m.train_data, True)))
    m.feed(feed)
    assert not m._graph_resident_step(int(feed["num_vertices"]), feed["initial_node_representation"], feed["adjacency_matrix"])
