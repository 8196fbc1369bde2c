"""Host-side checks (no GPU) of the native training step with the BasicRNNCell: the new C symbols (the fused cell backward, the two
launch sequences and their workspace function; include/ggnn_hip.h), their sizing and argument validation before any launch, the
opt-in value params['compact_rnn'] == 'native' and the dispatch order of train.train_step (chem_tensorflow_sparse.py:109-110 and
chem_tensorflow.py:183-191 are what the step computes)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ggnn_rnn_bwd_fused_supported", "ggnn_rnn_bwd_packed_bytes", "ggnn_rnn_bwd_pack_weights_f32", "ggnn_rnn_bwd_fused_f32",
       "ggnn_rnn_bwd_fused_gather_f32", "ggnn_sparse_rnn_train_workspace_bytes", "ggnn_sparse_rnn_train_forward_f32",
       "ggnn_sparse_rnn_train_backward_f32"]
E_INVALID, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3     # GGNN_E_* (include/ggnn_hip.h)
README = {"use_edge_bias": False, "use_edge_msg_avg_aggregation": True, "residual_connections": {},
          "layer_timesteps": [1, 1, 1, 1, 1, 1, 1, 1], "graph_rnn_cell": "RNN", "graph_rnn_activation": "ReLU"}


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


def test_supported_set_is_the_forwards(pkg, lib):
    for D in (4, 16, 32, 48, 64, 96, 100, 104, 128, 192, 256):
        for nx in range(0, 6):
            assert lib.ggnn_rnn_bwd_fused_supported(D, nx) == lib.ggnn_rnn_fused_supported(D, nx), (D, nx)
            assert pkg.ops.rnn_bwd_fused_supported(D, nx) == pkg.ops.rnn_fused_supported(D, nx)
            nbytes = lib.ggnn_rnn_bwd_packed_bytes(D, nx)
            assert (nbytes > 0) == bool(lib.ggnn_rnn_fused_supported(D, nx)), (D, nx)
            assert nbytes == lib.ggnn_rnn_packed_bytes(D, nx)           # nx + 1 images of the same format
    assert [(D, nx) for D in (32, 64, 100) for nx in (1, 2, 3) if lib.ggnn_rnn_bwd_fused_supported(D, nx)] == \
        [(32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3), (100, 1)]
    assert lib.ggnn_rnn_bwd_packed_bytes(64, 1) < lib.ggnn_rnn_bwd_packed_bytes(64, 2) < lib.ggnn_rnn_bwd_packed_bytes(64, 3)
    assert lib.ggnn_rnn_bwd_packed_bytes(100, 1) <= 160 * 1024          # resident in a CU's LDS


def test_workspace_sizing(lib):
    f = lib.ggnn_sparse_rnn_train_workspace_bytes
    gru = lib.ggnn_sparse_train_workspace_bytes
    V, D, T, R, steps = 1000, 100, 4, 2100, 8
    n = f(V, D, T, R, steps)
    # states (steps + 1), incoming, dP, dh, three dx per step, dHc per step: at least that; no r / u / c / r*h / dpg: the GRU's 6 V D
    # floats per step less
    assert n >= ((steps + 1) + 6 * steps) * V * D * 4 + steps * R * D * 4
    assert n <= gru(V, D, T, R, steps) - 6 * steps * V * D * 4
    for bad in ((-1, D, T, R, steps), (0, D, T, R, steps), (V, 0, T, R, steps), (V, D, 0, R, steps), (V, D, 65, R, steps),
                (V, D, T, -1, steps), (V, D, T, R, 0), (V, D, T, 1 << 31, steps)):
        assert f(*bad) == 0, bad
    for D_bad in (16, 48, 96, 104, 128, 192, 256):                        # hidden sizes outside the fused cell's
        assert f(V, D_bad, T, R, steps) == 0, D_bad
    for D_ok in (32, 64, 100):
        assert f(V, D_ok, T, R, steps) > 0
    # grows with the timesteps, the nodes and the compact rows: a caller may size once for its largest batch
    assert f(V, D, T, R, steps + 1) > n and f(V + 1, D, T, R, steps) > n and f(V, D, T, R + 64, steps) > n
    for axis in range(3):
        prev = 0
        for x in list(range(1, 40)) + [64, 100, 129, 255, 256, 257, 300, 5000]:
            arg = [V, R, steps]
            arg[axis] = x
            got = f(arg[0], D, T, arg[1], arg[2])
            assert got >= prev > -1 and got % 256 == 0, (axis, x)
            prev = got


def _buf(nbytes):
    raw = ctypes.create_string_buffer(nbytes + 512)
    base = (ctypes.addressof(raw) + 255) & ~255
    return raw, base


def test_argument_validation_without_a_launch(lib):
    """Every refusal comes back as an error code with ggnn_last_error set before anything touches the device (the pointers are host
    memory: a launch would fault)."""
    keep, p = _buf(8192)
    q = p + 4096
    V, D, T = 10, 32, 4
    dx = lambda *ptrs: (ctypes.c_void_p * 3)(*(list(ptrs) + [None] * (3 - len(ptrs))))
    cell = lambda **kw: lib.ggnn_rnn_bwd_fused_f32(
        kw.get("g", p), kw.get("out", p + 256), p + 512, kw.get("dP", q), kw.get("dx", dx(q + 256)), kw.get("dh", q + 512),
        kw.get("nin", p + 768), T, kw.get("use_avg", 1), kw.get("nx", 1), kw.get("V", V), kw.get("D", D), kw.get("act", 0), None)
    assert cell(g=None) == E_INVALID and "null" in _err(lib)
    assert cell(dP=None) == E_INVALID and cell(dh=None) == E_INVALID and cell(dx=dx()) == E_INVALID
    assert cell(nin=None) == E_INVALID and "nin" in _err(lib)
    assert cell(g=p + 4) == E_INVALID and "align" in _err(lib)
    assert cell(dh=q + 520) == E_INVALID and "align" in _err(lib)
    assert cell(dP=p) == E_INVALID and "alias" in _err(lib)              # dP == g
    assert cell(dh=p + 256) == E_INVALID and "alias" in _err(lib)        # dh == out
    assert cell(dx=dx(q)) == E_INVALID and "alias" in _err(lib)          # d_incoming == dP
    assert cell(act=7) == E_INVALID and "activation" in _err(lib)
    assert cell(V=-1) == E_INVALID
    assert cell(D=100, nx=2) == E_UNSUPPORTED and "nx=2" in _err(lib)
    assert cell(D=128) == E_UNSUPPORTED and cell(nx=0) == E_UNSUPPORTED and cell(nx=4) == E_UNSUPPORTED
    assert cell(V=(1 << 30) // D) == E_UNSUPPORTED and "2^30" in _err(lib)
    assert cell(V=0, g=None, dP=None) == 0                               # no rows: a no-op
    gather = lambda **kw: lib.ggnn_rnn_bwd_fused_gather_f32(
        p, kw.get("gz", p + 1024), kw.get("heads", p + 1280), kw.get("rows", 5), p + 256, p + 512, q, dx(q + 256), q + 512, p + 768, T, 1,
        1, V, D, 0, None)
    assert gather(gz=None) == E_INVALID and gather(heads=None) == E_INVALID
    assert gather(heads=p + 1284) == E_INVALID and "align" in _err(lib)
    assert gather(rows=-1) == E_INVALID
    assert gather(rows=(1 << 30) // D) == E_UNSUPPORTED and "2^30" in _err(lib)
    assert lib.ggnn_rnn_bwd_pack_weights_f32(p, 1, 48, q, None) == E_UNSUPPORTED
    assert lib.ggnn_rnn_bwd_pack_weights_f32(p, 1, 32, p, None) == E_INVALID
    assert lib.ggnn_rnn_bwd_pack_weights_f32(p, 1, 32, q + 4, None) == E_INVALID

    L, M = 2, 20
    lt = (ctypes.c_int32 * L)(2, 1)
    rp = (ctypes.c_int32 * (L + 1))(0, 0, 1)
    ri = (ctypes.c_int32 * 1)(0)
    tro = (ctypes.c_int64 * (T + 1))(0, 4, 8, 10, 12)
    arr = (ctypes.c_void_p * L)(p, p)
    wsb = lib.ggnn_sparse_rnn_train_workspace_bytes(V, D, T, 12, 3)
    assert wsb > 0
    off = ctypes.c_int64(-1)
    fwd = lambda **kw: lib.ggnn_sparse_rnn_train_forward_f32(
        kw.get("h0", p), V, kw.get("D", D), T, kw.get("M", M), p, p, p, kw.get("tro", tro), kw.get("nin", p), 1, L, lt, kw.get("rp", rp), ri,
        kw.get("edge", arr), kw.get("b", arr), kw.get("packed", arr), 0, kw.get("ws", p), kw.get("ws_bytes", wsb), ctypes.byref(off), None)
    assert fwd(h0=None) == E_INVALID and "null" in _err(lib)
    assert fwd(b=None) == E_INVALID and fwd(packed=None) == E_INVALID and fwd(edge=None) == E_INVALID
    assert fwd(ws=None) == E_INVALID and _err(lib)
    assert fwd(ws=p + 16) == E_INVALID and "align" in _err(lib)
    assert fwd(M=0) == E_INVALID and "message" in _err(lib)
    assert fwd(nin=None) == E_INVALID and "nin" in _err(lib)
    assert fwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert fwd(tro=(ctypes.c_int64 * (T + 1))(0, 0, 0, 0, 0)) == E_INVALID and "no messages" in _err(lib)      # no compact rows
    assert fwd(D=128) == E_UNSUPPORTED and "128" in _err(lib)
    assert fwd(D=100) == E_UNSUPPORTED and "layer 1" in _err(lib)         # nx = 2 at D = 100: a layer outside the fused cell's set
    rp3 = (ctypes.c_int32 * (L + 1))(0, 0, 3)
    assert fwd(rp=rp3) == E_INVALID and "residual" in _err(lib)
    missing = (ctypes.c_void_p * L)(p, None)
    assert fwd(packed=missing) == E_INVALID and "layer 1" in _err(lib)
    assert off.value == -1                                                # nothing ran

    bwd = lambda **kw: lib.ggnn_sparse_rnn_train_backward_f32(
        kw.get("h0", p), V, kw.get("D", D), T, p, kw.get("tro", tro), p, 1, L, lt, rp, ri, kw.get("rows_rp", p), p, None, p, p, None, p,
        kw.get("edge_t", arr), kw.get("packed", arr), 0, arr, kw.get("g_W", arr), kw.get("g_b", arr), kw.get("d_final", p), arr,
        kw.get("ws", p), kw.get("ws_bytes", wsb), None, None)
    assert bwd(h0=None) == E_INVALID and "null" in _err(lib)
    assert bwd(rows_rp=None) == E_INVALID and bwd(d_final=None) == E_INVALID
    assert bwd(packed=None) == E_INVALID and bwd(g_W=None) == E_INVALID and bwd(g_b=None) == E_INVALID and bwd(edge_t=None) == E_INVALID
    assert bwd(ws=None) == E_INVALID and _err(lib)
    assert bwd(ws=p + 16) == E_INVALID and "align" in _err(lib)
    assert bwd(ws_bytes=wsb - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert bwd(tro=(ctypes.c_int64 * (T + 1))(0, 0, 0, 0, 0)) == E_INVALID
    assert bwd(D=128) == E_UNSUPPORTED and bwd(D=100) == E_UNSUPPORTED and "layer 1" in _err(lib)
    assert bwd(g_W=missing) == E_INVALID and "layer 1" in _err(lib)
    del keep


def test_ops_wrappers_refuse_cpu_tensors(pkg):
    z = torch.zeros(4, 32)
    with pytest.raises(TypeError) as e:
        pkg.ops.rnn_bwd_fused(z, z.clone(), torch.zeros(64), None, False, 1, "tanh")
    assert "no CPU implementation" in str(e.value)
    with pytest.raises(TypeError):
        pkg.ops.rnn_bwd_pack(torch.zeros(64, 32), 1)
    with pytest.raises(TypeError):
        pkg.ops.PACKED.rnn_bwd(torch.zeros(64, 32), 1, 32)


def _cpu_model(pkg, ms, args=None, **config):
    cfg = dict(README, hidden_size=32, pack_on_device=False)
    cfg.update(config)
    a = {"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": cfg}
    a.update(args or {})
    return pkg.SparseGGNNChemModel(a)


def test_native_is_a_value_of_the_existing_key(pkg):
    assert "compact_rnn" not in pkg.SparseGGNNChemModel.default_params()
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    m = _cpu_model(pkg, ms, compact_rnn="native")
    assert m.params["compact_rnn"] == "native"
    assert not m.rnn_route() and not pkg.train_native.rnn_model_eligible(m)       # a CPU model: no HIP route, no native step
    feed = {"initial_node_representation": torch.zeros(6, 32), "num_graphs": 1, "graph_nodes_sorted": True}
    assert not pkg.train_native.rnn_eligible(m, feed) and not pkg.train_native.eligible(m, feed)
    assert m.threaded_batches_default() is True
    m.device = torch.device("cuda:0")                       # (the route's device condition alone; nothing runs)
    assert m.rnn_route()                                    # any truthy value turns the compacted route on


def test_model_predicate_per_disqualifying_config(pkg, monkeypatch):
    """rnn_model_eligible on models that LOOK like GPU models to it (device attribute and torch.cuda.is_available patched; nothing
    runs on a device, the optimizer is the model's own): True for the supported configs, False without the key, with True, and for
    each disqualifying config."""
    tn = pkg.train_native
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)

    def verdict(args=None, **config):
        m = _cpu_model(pkg, ms, args, **config)
        m.device = torch.device("cuda:0")
        if not m.optimizer.fused:                          # (a CPU model's optimizer is the per-tensor one; the predicate reads the flag)
            m.optimizer._flat = {}                         # TFAdam.fused: _flat is not None (never stepped here)
            assert m.optimizer.fused
        return tn.rnn_model_eligible(m), m

    ok, m = verdict(compact_rnn="native")
    assert ok and m.threaded_batches_default() is False
    assert not tn.model_eligible(m) and not tn.attn_model_eligible(m) and not tn.panel_model_eligible(m)
    for good in (dict(hidden_size=100), dict(hidden_size=64, layer_timesteps=[2, 1], residual_connections={"1": [0]}),
                 dict(hidden_size=32, layer_timesteps=[1, 1, 1], residual_connections={"2": [0, 1]}, graph_rnn_activation="tanh"),
                 dict(hidden_size=32, task_ids=[0, 1], multitask_readout=True), dict(edge_weight_dropout_keep_prob=0.8),
                 dict(use_edge_msg_avg_aggregation=False)):
        assert verdict(compact_rnn="native", **good)[0], good
    for bad in (dict(), dict(compact_rnn=True), dict(compact_rnn=False), dict(compact_rnn="Native"),
                dict(compact_rnn="native", graph_rnn_cell="GRU", graph_rnn_activation="tanh"),
                dict(compact_rnn="native", use_propagation_attention=True),
                dict(compact_rnn="native", use_edge_bias=True),
                dict(compact_rnn="native", graph_state_dropout_keep_prob=0.8),
                dict(compact_rnn="native", hidden_size=84),                                                  # padded to 100
                dict(compact_rnn="native", hidden_size=128),
                dict(compact_rnn="native", hidden_size=100, layer_timesteps=[2, 1], residual_connections={"1": [0]}),   # nx = 2 at 100
                dict(compact_rnn="native", hidden_size=64, layer_timesteps=[1, 1, 1, 1], residual_connections={"3": [0, 1, 2]}),
                dict(compact_rnn="native", layer_timesteps=[1, 0])):
        got, m = verdict(**bad)
        assert not got, bad
        if bad.get("compact_rnn") != "native":
            assert m.threaded_batches_default() is True
    assert not verdict({"--freeze-graph-model": True}, compact_rnn="native")[0]
    # the batch's part
    ok, m = verdict(compact_rnn="native")
    assert not tn.rnn_eligible(m, {"initial_node_representation": torch.zeros(6, 32), "num_graphs": 1, "graph_nodes_sorted": True})


def test_train_step_dispatch_order(pkg, monkeypatch):
    """train_step asks the predicates of train_native.ROUTES in the order default, attention, panel, RNN, dense, GCN and takes the
    first that holds: the order of the existing five is what it was, the new one sits behind the sparse model's other two.  Each
    entry's predicates are the module's functions of the matching names."""
    tn = pkg.train_native
    names = [r.name for r in tn.ROUTES]
    assert names == ["default", "attention", "panel", "rnn", "dense", "gcn"]
    assert [n for n in names if n != "rnn"] == ["default", "attention", "panel", "dense", "gcn"]
    preds = ["eligible", "attn_eligible", "panel_eligible", "rnn_eligible", "dense_eligible", "gcn_eligible"]
    for route, pred in zip(tn.ROUTES, preds):
        assert route.eligible is getattr(tn, pred), route.name
        assert route.model_eligible is getattr(tn, pred.replace("eligible", "model_eligible")), route.name
    real = tn.ROUTES
    monkeypatch.setattr(tn, "native_step", lambda route, model, batch: "stepped on " + route.name)
    for k in range(len(real)):
        asked = []
        fakes = tuple(r._replace(eligible=lambda model, batch, _n=r.name, _v=(i >= k): (asked.append(_n), _v)[1])
                      for i, r in enumerate(real))
        monkeypatch.setattr(tn, "ROUTES", fakes)
        assert pkg.train.train_step(object(), {}) == "stepped on " + names[k]
        assert asked == names[:k + 1]


def _looks_like_a_gpu_model(m):
    """What test_model_predicate_per_disqualifying_config's verdict() stands in for: the model is said to live on a GPU and its
    optimizer -- which keeps flat buffers on a GPU only -- is said to have them.  Nothing runs on a device."""
    m.device = torch.device("cuda:0")
    if not m.optimizer.fused:
        m.optimizer._flat = {}
    assert m.optimizer.fused
    return m


# (model class, config with its opt-in key, the key(s) whose absence keeps autograd, the one route that takes it)
EXCLUSIVE = {
    "default-h32": ("SparseGGNNChemModel", dict(hidden_size=32), (), "default"),
    "default-h64": ("SparseGGNNChemModel", dict(hidden_size=64), (), "default"),
    "default-h100": ("SparseGGNNChemModel", dict(hidden_size=100), (), "default"),
    "attention": ("SparseGGNNChemModel", dict(hidden_size=64, use_propagation_attention=True, compact_attention="native"),
                  ("compact_attention",), "attention"),
    "panel-h128": ("SparseGGNNChemModel", dict(hidden_size=128, native_panel_training=True), ("native_panel_training",), "panel"),
    "rnn": ("SparseGGNNChemModel", dict(README, hidden_size=32, compact_rnn="native"), ("compact_rnn",), "rnn"),
    "dense": ("DenseGGNNChemModel", dict(batch_size=8, graph_resident_training="native"), ("graph_resident_training",), "dense"),
    "gcn-h64": ("SparseGCNChemModel", dict(hidden_size=64, native_training=True), ("native_training",), "gcn"),
    "gcn-panel-h128": ("SparseGCNChemModel", dict(hidden_size=128, native_training=True, gcn_panel_layers=True), ("native_training",),
                       "gcn"),
}


@pytest.mark.parametrize("case", list(EXCLUSIVE))
def test_model_predicates_are_mutually_exclusive(pkg, monkeypatch, case):
    """What lets a table stand for an ordered chain: a model that looks like a GPU model is taken by exactly one route's model
    predicate, the expected one, and by none once its opt-in key is gone (the default route has no key: it is its own twin)."""
    cls, config, keys, want = EXCLUSIVE[case]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)

    def takers(cfg):
        m = getattr(pkg, cls)({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms,
                               "--config": dict(cfg, pack_on_device=False)})
        return [r.name for r in pkg.train_native.ROUTES if r.model_eligible(_looks_like_a_gpu_model(m))]

    assert takers(config) == [want]
    if keys:
        assert takers({k: v for k, v in config.items() if k not in keys}) == []
