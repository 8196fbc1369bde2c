"""CPU tests of the column-panel BasicRNNCell (csrc/ggnn_rnn_panel.hip, params['rnn_panel_cell']): the header and the ctypes table
agree on the five entry points, ggnn_rnn_panel_supported names the supported set and leaves ggnn_rnn_fused_supported's alone, the
image size is the documented one, every launcher refuses bad arguments with an error code before anything is launched, and on a CPU
model the key changes nothing."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("ggnn_rnn_panel_supported", "ggnn_rnn_panel_packed_bytes", "ggnn_rnn_panel_pack_weights_f32",
               "ggnn_rnn_panel_launch_geometry", "ggnn_rnn_panel_gather_f32")
SUPPORTED = [(D, nx) for D in (128, 192, 256) for nx in (1, 2, 3)]
UNSUPPORTED = [(64, 1), (100, 1), (128, 0), (128, 4), (160, 1), (320, 1)]
FUSED = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 2), (64, 3), (100, 1)]                        # tests/test_rnn_route_host.py
NOT_FUSED = [(48, 1), (128, 1), (64, 0), (64, 4), (32, 0), (32, 4), (100, 0), (100, 4)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_args(name):
    """Number of parameters the header declares for `name`."""
    with open(os.path.join(ROOT, "include", "ggnn_hip.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, "%s is not declared in include/ggnn_hip.h" % name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


def test_header_and_symbol_table_agree(pkg):
    lib = pkg._lib.load()
    for s in NEW_SYMBOLS:
        assert s in pkg._lib.SYMBOLS and hasattr(lib, s), s
        assert _header_args(s) == len(pkg._lib.SYMBOLS[s][1]), s
    assert _header_args("ggnn_rnn_panel_gather_f32") == _header_args("ggnn_rnn_packed_gather_f32")
    assert pkg._lib.SYMBOLS["ggnn_rnn_panel_gather_f32"] == pkg._lib.SYMBOLS["ggnn_rnn_packed_gather_f32"]
    assert lib.ggnn_abi_version() == pkg._lib.ABI_VERSION == 3


def test_supported_sets(pkg):
    lib = pkg._lib.load()
    for D in (32, 48, 64, 100, 128, 160, 192, 256, 320):
        for nx in range(6):
            want = 1 if (D, nx) in SUPPORTED else 0
            assert lib.ggnn_rnn_panel_supported(D, nx) == want, (D, nx)
            assert pkg.ops.rnn_panel_supported(D, nx) == bool(want)
    for D, nx in UNSUPPORTED:
        assert lib.ggnn_rnn_panel_supported(D, nx) == 0, (D, nx)
    # the resident-image cell keeps its set
    for D, nx in FUSED:
        assert lib.ggnn_rnn_fused_supported(D, nx) == 1, (D, nx)
    for D, nx in NOT_FUSED + SUPPORTED:
        assert lib.ggnn_rnn_fused_supported(D, nx) == 0, (D, nx)


def test_packed_bytes_and_geometry(pkg):
    lib = pkg._lib.load()
    for D, nx in SUPPORTED:
        assert lib.ggnn_rnn_panel_packed_bytes(D, nx) == (nx + 1) * (D // 64) * (D // 32) * 12288, (D, nx)
    for D, nx in UNSUPPORTED:
        assert lib.ggnn_rnn_panel_packed_bytes(D, nx) == 0, (D, nx)
        rows, wgs = ctypes.c_int(-1), ctypes.c_int(-1)
        lib.ggnn_rnn_panel_launch_geometry(D, nx, ctypes.byref(rows), ctypes.byref(wgs))
        assert (rows.value, wgs.value) == (0, 0), (D, nx)
        assert pkg.ops.rnn_panel_launch_geometry(D, nx) == (0, 0)


def _aligned(buf):
    p = ctypes.cast(buf, ctypes.c_void_p)
    return ctypes.c_void_p((p.value + 15) // 16 * 16)


def _launch(lib, D, nx, a, b, V=16, act=1, h=None, h_out=None, save=None, packed=None):
    """ggnn_rnn_panel_gather_f32 with distinct, aligned fake pointers (nothing may be launched: every call here must fail or be a
    no-op before the first HIP call)."""
    x = (ctypes.c_void_p * 2)(ctypes.c_void_p(a.value + 64), ctypes.c_void_p(a.value + 128))
    h = a if h is None else h
    h_out = b if h_out is None else h_out
    packed = ctypes.c_void_p(a.value + 192) if packed is None else packed
    return lib.ggnn_rnn_panel_gather_f32(x, nx, h, packed, ctypes.c_void_p(a.value + 256), h_out, ctypes.c_void_p(a.value + 320), 8,
                                         ctypes.c_void_p(a.value + 384), ctypes.c_void_p(a.value + 448), 8,
                                         ctypes.c_void_p(a.value + 512), 4, 1, save, V, D, act, None)


def test_launchers_refuse_bad_arguments_without_gpu(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 1024)()
    a = _aligned(buf)
    b = ctypes.c_void_p(a.value + 2048)
    # unsupported (D, nx)
    for D, nx in UNSUPPORTED + [(32, 1), (64, 3)]:
        assert _launch(lib, D, nx, a, b) == -2, (D, nx)
        assert b"panel RNN cell supports" in lib.ggnn_last_error()
        assert lib.ggnn_rnn_panel_pack_weights_f32(a, nx, D, b, None) == -2, (D, nx)
        assert b"panel RNN cell supports" in lib.ggnn_last_error()
    # null operands
    assert lib.ggnn_rnn_panel_gather_f32(None, 1, None, None, None, None, None, 8, None, None, 8, None, 4, 1, None, 16, 128, 1, None) == -1
    assert b"null" in lib.ggnn_last_error()
    assert lib.ggnn_rnn_panel_pack_weights_f32(None, 1, 128, None, None) == -1
    assert lib.ggnn_rnn_panel_pack_weights_f32(a, 1, 128, a, None) == -1          # packed aliases W
    assert _launch(lib, 192, 2, a, b, packed=ctypes.c_void_p(None)) == -1 and b"null" in lib.ggnn_last_error()
    # misalignment
    assert _launch(lib, 128, 1, a, b, h_out=ctypes.c_void_p(b.value + 4)) == -1 and b"aligned" in lib.ggnn_last_error()
    # aliasing: h_out on h, on a residual segment, on save_incoming; save_incoming on an input
    assert _launch(lib, 128, 1, a, b, h_out=a) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 192, 2, a, b, h_out=ctypes.c_void_p(a.value + 64)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 256, 3, a, b, h_out=ctypes.c_void_p(a.value + 128)) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 256, 1, a, b, save=b) == -1 and b"alias" in lib.ggnn_last_error()
    assert _launch(lib, 128, 1, a, b, save=a) == -1 and b"alias" in lib.ggnn_last_error()
    # unknown activation
    assert _launch(lib, 128, 1, a, b, act=2) == -1 and b"activation" in lib.ggnn_last_error()
    # 32-bit byte offsets: V * D >= 2^30
    for D in (128, 192, 256):
        assert _launch(lib, D, 1, a, b, V=((1 << 30) + D - 1) // D) == -2 and b"2^30" in lib.ggnn_last_error()
    # V == 0 is a no-op
    for D, nx in SUPPORTED:
        assert _launch(lib, D, nx, a, b, V=0) == 0
    assert lib.ggnn_rnn_panel_gather_f32(None, 1, None, None, None, None, None, 0, None, None, 0, None, 4, 0, None, 0, 256, 0, None) == 0


def _cpu_model(pkg, **config):
    ms = pkg.synthetic_qm9(10, mean_nodes=6, seed=3)
    return pkg.SparseGGNNChemModel({"--quiet": True, "--device": "cpu", "train_data": ms, "valid_data": ms, "--config": config})


def test_route_predicate(pkg):
    assert "rnn_panel_cell" not in pkg.SparseGGNNChemModel.default_params()
    on = dict(graph_rnn_cell="RNN", compact_rnn=True, rnn_panel_cell=True, hidden_size=128)
    for config in (dict(on, compact_rnn=False), dict(on, graph_rnn_cell="GRU"), dict(on, use_propagation_attention=True),
                   dict(on, compact_rnn="native"), dict(graph_rnn_cell="RNN", compact_rnn=True, hidden_size=128)):
        model = _cpu_model(pkg, **config)
        assert not model.rnn_panel_route(), config
        model.device = torch.device("cuda:0")               # (the predicate's device condition alone; nothing runs)
        assert not model.rnn_panel_route(), config
    for hidden in (64, 100, 120, 128, 150, 192, 256):
        model = _cpu_model(pkg, **dict(on, hidden_size=hidden))
        assert not model.rnn_panel_route(), "a CPU model has no HIP route"
        model.device = torch.device("cuda:0")
        assert model.rnn_panel_route() and model.rnn_route(), hidden
    assert _cpu_model(pkg, **dict(on, hidden_size=120))._kw == 128 and _cpu_model(pkg, **dict(on, hidden_size=150))._kw == 192


def test_cpu_model_key_changes_nothing(pkg):
    """States, loss and gradients of a CPU model are torch.equal with and without the key -- or, where the hot path has no CPU
    implementation at all, both models say so in the same words."""
    outcomes = []
    for key in (True, False):
        config = dict(graph_rnn_cell="RNN", graph_rnn_activation="ReLU", hidden_size=128, compact_rnn=True, pack_on_device=False)
        if key:
            config["rnn_panel_cell"] = True
        torch.manual_seed(0)
        model = _cpu_model(pkg, **config)
        assert not model.rnn_route() and not model.rnn_panel_route()
        try:
            feed = next(iter(model.make_minibatch_iterator(model.valid_data, is_training=False)))
            with torch.no_grad():
                model.feed(feed)
                states = model.compute_final_node_representations().clone()
            variables = model.trainable_variables
            for v in variables.values():
                v.requires_grad_(True); v.grad = None
            model.training = True
            loss = model.forward_batch(feed)
            loss.backward()
            outcomes.append(("ran", states, loss.detach().clone(), {k: v.grad.clone() for k, v in variables.items()}))
        except TypeError as e:
            outcomes.append(("refused", str(e)))
    on, off = outcomes
    assert on[0] == off[0]
    if on[0] == "refused":
        assert on[1] == off[1] and "no CPU implementation" in on[1]
    else:
        assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2]) and set(on[3]) == set(off[3])
        for k in off[3]:
            assert torch.equal(on[3][k], off[3][k]), k
