"""tests/gru_fwd_ref.py on the CPU, on the very inputs tests/test_gpu_gru_fwd_cells.py feeds the kernels:

  *  the operand formats the library ships stay inside the a-priori bound at FACTOR 1: a plain float32 numpy evaluation of the cell,
     and one with every product operand rounded to two f16 pieces (kSplitF16x2 of csrc/ggnn_split.hpp, emulated in numpy);
  *  the comparison has teeth at the factor the GPU test uses (gru_fwd_ref.CAP[D]): wrong results of eight kinds each fail the
     bound of the output named for them;
  *  ggnn_gru_describe refuses what the launchers refuse, and a sweep of its arguments over the legs of the GPU test selects every
     cell of ggnn_gru_cells and nothing outside it (this part loads the library; it needs no GPU)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gru_fwd_ref as gr
from conftest import PKG, ROOT

# (D, nx, V, gather, T, use_avg, act): gather cells at the three fused sizes, mean and sum, both activations; the panel sizes plain
CASES = [(100, 2, 65, 1, 4, 1, "tanh"), (100, 1, 63, 1, 3, 0, "relu"), (100, 3, 17, 1, 4, 1, "tanh"), (64, 1, 65, 1, 3, 1, "tanh"),
         (32, 3, 17, 1, 4, 0, "tanh"), (100, 1, 1, 1, 4, 1, "tanh"), (100, 2, 65, 0, 0, 0, "relu"), (128, 2, 65, 0, 0, 0, "tanh"),
         (192, 1, 15, 0, 0, 0, "tanh"), (256, 3, 16, 0, 0, 0, "tanh")]
IDS = ["D%d-nx%d-V%d-%s-T%d-%s-%s" % (D, nx, V, "gather" if g else "plain", T, "mean" if avg else "sum", act)
       for D, nx, V, g, T, avg, act in CASES]
GATHER_CASES = [c for c in CASES if c[3] and c[2] > 16]
GATHER_IDS = [i for i, c in zip(IDS, CASES) if c[3] and c[2] > 16]


def _case(p):
    D, nx, V, g, T, avg, act = p
    return gr.make_case(D, nx, V, g, T, avg, act)


def _worst(got, ref, bound, names=gr.OUTPUTS):
    """{output: worst error / bound}; the outputs must all be inside factor 1."""
    return {k: gr.assert_within(got[k], ref[k], bound[k], 1.0, k) for k in names}


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_float32_evaluation_stays_within_factor_1(p):
    c = _case(p)
    ref, bound = gr.bounds(c)
    print("float32 numpy, worst error / bound: %s" % json.dumps(_worst(gr.forward(c, np.float32), ref, bound), sort_keys=True))
    if c.gather and c.V > 1:
        assert not ref["incoming"][0].any() and not gr.forward(c, np.float32)["incoming"][0].any()    # in-degree 0: exactly zero


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_f16x2_operands_stay_within_factor_1(p):
    """Two f16 pieces keep 22 of an operand's 24 significand bits: each of the three products is off by up to ~2^-22 of |a| |w|,
    which is above the 4e-7 of the bound's pre-activation term -- but the roundings are of mixed sign and the bound sums MAGNITUDES
    over K = (nx + 1) D terms, so the format stays inside the same constant; no constant of its own was needed."""
    c = _case(p)
    ref, bound = gr.bounds(c)
    got = gr.forward(c, np.float32, matmul=gr.matmul_f16x2)
    print("f16x2 emulation, worst error / bound: %s" % json.dumps(_worst(got, ref, bound), sort_keys=True))


def _fails(got, ref, bound, name, factor):
    with pytest.raises(AssertionError, match="outside"):
        gr.assert_within(got[name], ref[name], bound[name], factor, name)


@pytest.mark.parametrize("p", CASES, ids=IDS)
def test_wrong_cells_fail_at_the_cap(p):
    """Corruptions of the cell itself, each against the bound of the output it reaches first, at the GPU test's factor."""
    c = _case(p)
    D, nx, cap = c.D, c.nx, gr.CAP[c.D]
    ref, bound = gr.bounds(c)
    # one D x D block of Wg (segment 0, r columns) / of Wc (the r*h rows) scaled by 1.001
    Wg = c.Wg.copy(); Wg[:D, :D] *= np.float32(1.001)
    _fails(gr.forward(c._replace(Wg=Wg)), ref, bound, "r", cap)
    _fails(gr.forward(c._replace(Wg=Wg)), ref, bound, "h_out", cap)
    Wc = c.Wc.copy(); Wc[nx * D:, :] *= np.float32(1.001)
    _fails(gr.forward(c._replace(Wc=Wc)), ref, bound, "c", cap)
    _fails(gr.forward(c._replace(Wc=Wc)), ref, bound, "h_out", cap)
    # r and u swapped
    sw = gr.forward(c._replace(Wg=np.concatenate([c.Wg[:, D:], c.Wg[:, :D]], 1), bg=np.concatenate([c.bg[D:], c.bg[:D]])))
    _fails(sw, ref, bound, "r", cap)
    _fails(sw, ref, bound, "h_out", cap)
    # operands truncated to two bf16 pieces (16 bits): the gates, the first outputs the products reach (2.6 .. 7.6 x their bound
    # on these cases; behind the candidate's tanh and the blend a single row can stay inside 2 x, so r and u are the outputs named)
    _fails(gr.forward(c, np.float32, matmul=gr.matmul_bf16x2_truncated), ref, bound, "r", cap)
    _fails(gr.forward(c, np.float32, matmul=gr.matmul_bf16x2_truncated), ref, bound, "u", cap)
    # the candidate computed from h instead of r * h
    x = np.concatenate([s.astype(np.float64) for s in c.res] + [ref["incoming"]], 1)
    cand = gr._act(c.act, np.concatenate([x, c.h.astype(np.float64)], 1) @ c.Wc.astype(np.float64) + c.bc)
    _fails(dict(c=cand), ref, bound, "c", cap)
    _fails(dict(h_out=ref["u"] * c.h + (1 - ref["u"]) * cand), ref, bound, "h_out", cap)
    # a bias row left out
    _fails(gr.forward(c._replace(bg=np.concatenate([np.zeros(D, np.float32), c.bg[D:]]))), ref, bound, "r", cap)
    _fails(gr.forward(c._replace(bc=np.zeros(D, np.float32))), ref, bound, "h_out", cap)
    # one row computed from the row 16 below it
    if c.V > 16:
        got = {k: v.copy() for k, v in ref.items()}
        for k in got:
            got[k][c.V - 1] = ref[k][c.V - 17]
        _fails(got, ref, bound, "h_out", cap)


@pytest.mark.parametrize("p", GATHER_CASES, ids=GATHER_IDS)
def test_wrong_gathers_fail_at_the_cap(p):
    c = _case(p)
    cap = gr.CAP[c.D]
    ref, bound = gr.bounds(c)
    hub = c.V - 1
    # the hub's fifth message dropped (it is of type 4 % T, the last row of that type's list)
    t = 4 % c.T
    assert c.adj[t][-1, 1] == hub
    adj = tuple(a[:-1] if i == t else a for i, a in enumerate(c.adj))
    den = c.nin.astype(np.float64).sum(-1, keepdims=True) + np.float64(gr.SMALL32)
    inc = gr.segment(c._replace(adj=adj), denominator=den)[0]
    _fails(dict(incoming=inc), ref, bound, "incoming", cap)
    _fails(gr.forward(c, incoming=inc), ref, bound, "h_out", cap)
    # the mean taken with the type count instead of the in-degree sum
    if c.use_avg:
        inc = gr.segment(c, denominator=np.full((c.V, 1), c.T + np.float64(gr.SMALL32)))[0]
        _fails(dict(incoming=inc), ref, bound, "incoming", cap)
        _fails(gr.forward(c, incoming=inc), ref, bound, "h_out", cap)


# ---- the describe query (needs the library, no GPU) -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return importlib.import_module(PKG)._lib.load()


def test_entry_points_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "ggnn_hip.h")).read()
    for name in ("ggnn_gru_describe", "ggnn_gru_cells"):
        assert hasattr(lib, name) and name + "(" in header
    cells = gr.table(lib)
    assert len(cells) == len(set(cells)) == lib.ggnn_gru_cells(None, 0) > 0
    assert len({gr.cell_id(c) for c in cells}) == len(cells)                  # every cell has a name of its own


def test_describe_refuses_what_the_launchers_refuse(lib):
    A = gr.Args
    ok = A(100, 1, 2, 1, 0, "tanh", 1, 4, 0, 1)
    assert gr.describe(lib, ok, matrix_split=1)[0] == 0
    assert lib.ggnn_gru_describe(100, 1, 2, 1, 0, 0, 1, 4, 0, 1, 1, None) == gr.E_INVALID
    assert gr.describe(lib, ok._replace(nx=4), matrix_split=1)[0] == gr.E_INVALID
    assert gr.describe(lib, ok._replace(nx=0), matrix_split=1)[0] == gr.E_INVALID
    assert gr.describe(lib, ok._replace(fmt=1), matrix_split=1)[0] == gr.E_INVALID
    for ms in (0, 1):
        assert gr.describe(lib, ok._replace(D=36), matrix_split=ms)[0] == gr.E_UNSUPPORTED
        assert gr.describe(lib, ok._replace(D=128), matrix_split=ms)[0] == gr.E_UNSUPPORTED        # no gather-fused panel GRU
        assert gr.describe(lib, ok._replace(D=128, gather=0), matrix_split=ms)[0] == 0
    for form in (63, 65, 66, 67, 68, 69):
        for a in (ok, ok._replace(act="relu"), ok._replace(D=64), ok._replace(save=1)):
            assert gr.describe(lib, a, form=form, matrix_split=1)[0] == gr.E_UNSUPPORTED, (form, a)
    # the wide kernel takes the inference launch of the tanh cell only; a launch that saves stays on ring form 0
    rc, cell, geom = gr.describe(lib, ok, form=6, matrix_split=1)
    assert rc == 0 and gr.FAMILIES[cell[0]] == "wide" and cell[11] == 2 and geom == (4, 128, 1, 0)
    rc, cell, geom = gr.describe(lib, ok._replace(save=1), form=6, matrix_split=1)
    assert rc == 0 and gr.FAMILIES[cell[0]] == "ring" and cell[4] == 0 and cell[6] == cell[7] == 1 and geom[:3] == (8, 128, 1)
    # the default selection: form 1, except the single-input launch in bf16x3 (form 0)
    for nx, fmt, form in ((1, 2, 1), (2, 2, 1), (3, 3, 1), (1, 3, 0)):
        a = ok._replace(nx=nx, fmt=fmt, T=3)
        assert gr.describe(lib, a, form=-1, matrix_split=1)[1] == gr.describe(lib, a, form=form, matrix_split=1)[1] or \
            "GGNN_GRU_FORM" in os.environ


_SWEEP = "import importlib, json, sys; sys.path[:0] = [%r, %r]; import gru_fwd_ref as gr; " \
         "lib = importlib.import_module(%r)._lib.load(); print(json.dumps(sorted(gr.sweep(lib))))"


def test_the_sweep_reaches_exactly_the_table(lib):
    """One process per leg (the matrix path and GGNN_GRU_NOSAVE_KERNEL are read once per process): between them the sweeps select
    every cell of the table, and no query returns a cell outside it."""
    table = set(gr.table(lib))
    union, per_leg = set(), {}
    for name, env_add in gr.LEGS.items():
        env = {k: v for k, v in os.environ.items() if k not in gr.LEG_VARS}
        env.update(env_add)
        r = subprocess.run([sys.executable, "-c", _SWEEP % (ROOT, os.path.join(ROOT, "tests"), PKG)], env=env, capture_output=True,
                           text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        per_leg[name] = {tuple(c) for c in json.loads(r.stdout.splitlines()[-1])}
        assert per_leg[name] <= table, (name, sorted(per_leg[name] - table)[:5])
        union |= per_leg[name]
    assert union == table, sorted(table - union)[:10]
    # the split path and GGNN_GRU_NOSAVE_KERNEL=1 each own cells no other leg selects; the plain f32 leg runs the residual inference
    # launches on the training instantiations, its stores skipped at run time -- no cell of its own, but the launch the product makes
    assert per_leg["split"] - per_leg["f32"] - per_leg["f32-nosave"] and per_leg["f32-nosave"] - per_leg["f32"] - per_leg["split"]
