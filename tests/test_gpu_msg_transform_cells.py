"""Every instantiation of the compacted message transform -- msg_transform_compact_kernel (whole-block, csrc/ggnn_msg_compact.hip),
msg_transform_ring_kernel and msg_transform_panel_kernel (ring / stationary, csrc/ggnn_panel.hip), behind
ggnn_msg_transform_compact_f32 -- against Hc[r] = h[pair_node[r]] @ W[t(r)] in float64 (tests/msg_transform_ref.py), per element,
inside the a-priori bound  PRE * (|h[pair_node[r]]| @ |W_t|) + 2^-126.

Which kernel runs depends on D, on `fmt` and on GGNN_MATRIX / GGNN_PANEL_TRANSFORM, which the library reads once per process, so
every case first asserts through ggnn_msg_transform_compact_describe (the launchers' own selection and schedule functions) that it
selects the instantiation the test is named after IN THIS PROCESS.  The legs -- the split path with the ring kernel (the default),
GGNN_MATRIX=f32, and GGNN_PANEL_TRANSFORM=0 on the split path -- are this process plus one child pytest process over this file per
other leg; each writes the instantiations it ran to a report and the parent asserts that between them all 21 ran.

Cases per instantiation, driven through the C entry with caller-owned buffers (pairs node-ascending and unique per type):
  rows        T = 7, rows of a type 1, 15, 16, 17, 127, 128, 129
  empty       empty types first, in the middle (two in a row) and last
  t1, t1-one-row   T = 1 with 129 rows and with one
  t64         T = 64, five types with rows (four of them one row): the linear type scan over equal offsets
  multipass   two unequal types; the row counts are the smallest for which the QUERY reports a wave that walks >= 3 tiles and one that
              walks exactly 2 (msg_transform_ref.multipass_rows; no CU count is known to the test): the loop's a = an, its in-loop
              pair prefetch and, for the panel kernels, a small type floored to one workgroup that makes three passes.  Both types are
              ragged (16 k + 7 and 234 / 300 rows) and one of them has waves a tile apart.
  backward    the backward's Z = dHc W_t^T: identity pair list over all rows, PackedWeights.edge_t images against the raw W^T route,
              rows scaled 1e-6 .. 1e3 (the exact formats only: the backward never runs f16x2)
Per case: every row of every type inside the bound; two runs bit-identical; the pre-packed route (ggnn_edge_weights_pack_f32, then
W = NULL) bit-identical to the raw-weight route; the sentinel rows behind type_row_off[T] bit-unchanged; h, W and pair_node unchanged.

The factor over the bound is measured, not chosen: the dense form (ggnn_msg_transform_f32 of csrc/ggnn_gemm.hip: independent code
on the f32 MFMA), gathered at [pair_node, t], runs on the same inputs and a kernel passes if its worst error / bound ratio is at most
2 x that route's over the same cases (another order of summation over the same number of terms) AND at most msg_transform_ref.CAP[D],
the next power of two above 2 x the route's worst ratio over the whole file.  tests/test_msg_transform_ref_host.py shows that
float32 and both operand formats stay inside factor 1 and that wrong results of eight kinds fail at CAP.  A cap is not raised to
make a kernel pass.

Measured worst error / bound (MI355X; all legs, all cases of an instantiation | the dense route on the same cases):
    D   format  family        kernel   dense route
   32   bf16x3  whole-block   0.318    0.729
   32   f16x2   whole-block   0.346    0.729
   32   f32     whole-block   0.729    0.729
   64   bf16x3  whole-block   0.583    0.917
   64   f16x2   whole-block   0.398    0.917
   64   f32     whole-block   0.917    0.917
  100   bf16x3  whole-block   0.597    0.800
  100   f16x2   whole-block   0.607    0.800
  100   f32     whole-block   0.800    0.800
  128   bf16x3  ring          0.574    0.727
  128   f16x2   ring          0.425    0.727
  128   bf16x3  stationary    0.557    0.635
  128   f32     stationary    0.635    0.635
  192   bf16x3  ring          0.621    0.821
  192   f16x2   ring          0.429    0.821
  192   bf16x3  stationary    0.621    0.737
  192   f32     stationary    0.737    0.737
  256   bf16x3  ring          0.671    0.815
  256   f16x2   ring          0.468    0.815
  256   bf16x3  stationary    0.684    0.772
  256   f32     stationary    0.772    0.772
The dense route's worst ratio per hidden size: 0.729 (32), 0.917 (64), 0.800 (100), 0.727 (128), 0.821 (192), 0.815 (256); twice that is
between 1.45 and 1.83, so every CAP is 2.  The f32 kernels reproduce the dense route bit for bit on every case (the same fmaf chains),
both split formats sit below it in every row; the worst ratios are the multi-pass cases' (the most elements).  The multi-pass sizes the
query gave on the 256-CU part: 130823 + 234 rows for the whole-block kernels (341 workgroups walk 3 / 2 tiles per wave, one walks
2 / 1), 38103 + 300 for the ring kernels (254 workgroups walk 2 / 1, the small type's one walks 3 / 2) and 18903 / 12455 / 9303 + 300
for the stationary kernels at D = 128 / 192 / 256.  All 21 instantiations ran, none missed its bound at factor 1, let alone at the cap.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import msg_transform_ref as mr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

LEG = os.environ.get("GGNN_MSGT_CELLS_LEG")                  # set for the child processes of the legs test: the leg's name
REPORT = os.environ.get("GGNN_MSGT_CELLS_REPORT")            # a file that receives what ran
ONLY = os.environ.get("GGNN_MSGT_CELLS_FAMILY")              # a leg that owns one family runs only that
_ran = {"cells": {}, "route": {}, "multipass": {}}           # instantiation -> worst ratio; -> the route's; -> the schedule asserted
MULTIPASS_LIMIT = {False: 160000, True: 80000}               # rows, by D >= 128: the float64 reference on the CPU is the cost


def _ops():
    import importlib
    return importlib.import_module(PKG).ops


def _selected():
    """[(instantiation, D, fmt)] of THIS process: what the query selects over D x {bf16x3, f16x2}, each instantiation once."""
    ops, seen, out = _ops(), set(), []
    for D in mr.SIZES:
        for fmt in (mr.BF16X3, mr.F16X2):
            d = ops.msg_transform_compact_describe(D, (0, 40), fmt)
            name = mr.instantiation(d["family"], D, d["fmt"])
            if name not in seen and (not ONLY or d["family"] == ONLY):
                seen.add(name)
                out.append((name, D, fmt))
    return out


def pytest_generate_tests(metafunc):
    if "inst" not in metafunc.fixturenames:
        return
    try:
        sel = _selected()
    except Exception as e:                                   # (no library: the tests fail with the reason, the collection goes on)
        metafunc.parametrize("inst", [(e, 0, 0)], ids=["library-not-loaded"])
        return
    metafunc.parametrize("inst", sel, ids=[s[0] for s in sel])


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        with open(REPORT, "w") as f:
            json.dump(_ran, f, indent=1, sort_keys=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=3)
def _prepared(key):
    """(case, device tensors, float64 reference, bound, the dense route's worst ratio) of a case: computed once, shared by the
    instantiations of its hidden size, left unchanged.  key: (name, D, rows or None)."""
    name, D, rows = key
    if name == "backward":
        c, Wf = mr.backward_case(D)
    else:
        c, Wf = (mr.small_case(name, D) if rows is None else mr.make_case(name, D, rows)), None
    ref, bnd = mr.reference(c), mr.bound(c)
    d = dict(h=dev(c.h), W=dev(c.W), pn=dev(c.pair_node), Wf=None if Wf is None else dev(Wf))
    # the dense form on the same inputs, gathered at [pair_node, t]
    H = _ops().msg_transform(d["h"], d["W"]).view(c.V, c.T, D)
    got = torch.cat([H[d["pn"][int(c.row_off[t]):int(c.row_off[t + 1])].long(), t] for t in range(c.T)]).cpu().numpy()
    del H
    return c, d, ref, bnd, mr.worst_ratio(got, ref, bnd)


@functools.lru_cache(maxsize=16)
def _prepared_small(key):
    return _prepared.__wrapped__(key)


def _launch(lib, c, d, W, ws, fmt, Hc):
    import ctypes
    off = (ctypes.c_int64 * (c.T + 1))(*[int(x) for x in c.row_off])
    rc = lib.ggnn_msg_transform_compact_f32(d["h"].data_ptr(), None if W is None else W.data_ptr(), d["pn"].data_ptr(), off, Hc.data_ptr(),
                                            ws.data_ptr(), ws.numel(), c.V, c.D, c.T, fmt, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("ggnn_msg_transform_compact_f32: %d %s" % (rc, lib.ggnn_last_error()))


def _run(pkg, lib, c, d, fmt):
    """The raw-weight route twice and the pre-packed route once, each into a sentinel-filled buffer of its own with GUARD rows
    behind the last type -> (host buffer of the first run, what differed).  A missed bound lets the session go on; an ERROR of
    the library or the runtime ends it here (pytest.exit), so that nothing more is started on a GPU that may have faulted -- a
    leg's parent sees the exit status and starts no further leg."""
    R = int(c.row_off[-1])
    try:
        keep = {k: d[k].clone() for k in ("h", "W", "pn")}
        nbytes = lib.ggnn_msg_transform_compact_workspace_bytes(c.D, c.T)
        bufs = []
        for route in ("raw", "raw", "packed"):
            Hc = torch.full((R + mr.GUARD, c.D), float(mr.SENTINEL), dtype=torch.float32, device="cuda:0")
            if route == "raw":
                ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
                _launch(lib, c, d, d["W"], ws, fmt, Hc)
            elif d["Wf"] is not None:                            # the backward's images: PackedWeights.edge_t of the forward weights
                packed = pkg.ops.PackedWeights().edge_t(d["Wf"], fmt or mr.BF16X3)
                _launch(lib, c, d, None, packed.view(torch.uint8), fmt, Hc)
            else:
                ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
                pkg._lib.check(lib.ggnn_edge_weights_pack_f32(d["W"].data_ptr(), c.T, c.D, fmt, ws.data_ptr(),
                                                              torch.cuda.current_stream().cuda_stream))
                _launch(lib, c, d, None, ws, fmt, Hc)
            bufs.append(Hc)
        torch.cuda.synchronize()
        differ = [w for w, ok in (("two runs", torch.equal(bufs[0].view(torch.int32), bufs[1].view(torch.int32))),
                                  ("the pre-packed route", torch.equal(bufs[0].view(torch.int32), bufs[2].view(torch.int32))),
                                  ("h", torch.equal(keep["h"], d["h"])), ("W", torch.equal(keep["W"], d["W"])),
                                  ("pair_node", torch.equal(keep["pn"], d["pn"]))) if not ok]
        host = bufs[0].cpu().numpy()
    except RuntimeError as e:
        pytest.exit("library or runtime error, nothing more is run: %s" % e, returncode=3)
    return host, differ


def _multipass_key(pkg, name, D, fmt):
    """The multi-pass case of an instantiation, its sizes from the query; asserts the regime through the query."""
    desc = lambda off: pkg.ops.msg_transform_compact_describe(D, off, fmt)
    big, small = mr.multipass_rows(desc, 234 if D < 128 else 300, MULTIPASS_LIMIT[D >= 128])
    d = desc((0, big, big + small))
    three, two, apart = mr.walks(d["types"])
    assert three and two and apart, d
    assert big % 16 and small % 16                                     # both last tiles are ragged
    _ran["multipass"][name] = dict(rows=[big, small], types=d["types"], workgroups=d["workgroups"])
    return ("multipass", D, (big, small))


def test_instantiation_matches_float64(pkg, cuda, lib, inst):
    name, D, fmt = inst
    if isinstance(name, Exception):
        raise name
    used = [k for k, v in mr.FMT_NAMES.items() if name.endswith("-" + v)][0]
    keys = [(n, D, None) for n in mr.SMALL_CASES] + [_multipass_key(pkg, name, D, fmt)]
    if used != mr.F16X2:
        keys.append(("backward", D, None))
    worst, route, failures = 0.0, 0.0, []
    for key in keys:
        c, d, ref, bnd, rt = (_prepared if key[2] else _prepared_small)(key)
        sel = pkg.ops.msg_transform_compact_describe(D, [int(x) for x in c.row_off], fmt)
        assert mr.instantiation(sel["family"], D, sel["fmt"]) == name, (key, sel)
        host, differ = _run(pkg, lib, c, d, fmt)
        try:
            ratio = mr.check(host, ref, bnd, mr.CAP[D], "%s %s" % (name, key[0]))
        except AssertionError as e:
            failures.append(str(e))
            ratio = mr.worst_ratio(host[:ref.shape[0]], ref, bnd)
        if differ:
            failures.append("%s %s: not bit-identical: %s" % (name, key[0], ", ".join(differ)))
        print("%s %-12s rows %-7d worst error / bound %.3f; dense route %.3f" % (name, key[0], ref.shape[0], ratio, rt))
        worst, route = max(worst, ratio), max(route, rt)
    _ran["cells"][name] = worst
    _ran["route"][name] = route
    print("%s: worst error / bound %.3f; dense route on the same cases %.3f; cap %g" % (name, worst, route, mr.CAP[D]))   # (the figures first)
    assert not failures, failures
    assert worst <= 2 * route, "%s: worst ratio %.3f is more than twice the dense route's %.3f" % (name, worst, route)


def _table(cells, route):
    """The header's table: per hidden size, format and kernel family, the worst ratio of the kernel and of the dense route."""
    out = ["    D   format  family        kernel   dense route"]
    for name in sorted(cells, key=lambda n: (int(n.split("-D")[1].split("-")[0]), n)):
        fam, rest = name.split("-D")
        D, f = rest.split("-")
        out.append("  %3s   %-6s  %-11s   %.3f    %.3f" % (D, f, fam, cells[name], route.get(name, float("nan"))))
    return "\n".join(out)


def _is_leg(env_add):
    return all(os.environ.get(k, "") == env_add.get(k, "") for k in mr.LEG_VARS)


def test_other_legs_and_every_instantiation_ran(pkg, cuda, lib, tmp_path):
    """The legs this process is not: one child pytest process over this file each, one at a time, each under its own time limit.
    A child that ends by signal, abort, time limit or a library / runtime error fails the test at once and no further leg is
    started; a child in which only bounds were missed is reported at the end, after the other legs.  Every leg reports the
    instantiations it ran; their union with what this process ran is the 21 of msg_transform_ref.INSTANTIATIONS, and every one of
    them asserted its multi-pass schedule through the query."""
    if LEG:
        pytest.skip("a leg's own process does not start legs")
    mine = {s[0] for s in _selected()}
    cells, route, multipass = dict(_ran["cells"]), dict(_ran["route"]), dict(_ran["multipass"])
    me = os.path.abspath(__file__)
    missed = []
    for n, (env_add, only) in mr.LEGS.items():
        if _is_leg(env_add) and mine <= set(cells):
            continue                                                              # (this process is that leg and has run its kernels)
        env = {k: v for k, v in os.environ.items() if k not in mr.LEG_VARS and k != "GGNN_MSGT_CELLS_FAMILY"}
        env.update(env_add)
        report = str(tmp_path / ("%s.json" % n))
        env.update(GGNN_MSGT_CELLS_LEG=n, GGNN_MSGT_CELLS_REPORT=report)
        if only:
            env["GGNN_MSGT_CELLS_FAMILY"] = only
        r = subprocess.run([sys.executable, "-m", "pytest", me, "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rfP",
                            "--deselect", "%s::test_other_legs_and_every_instantiation_ran" % os.path.relpath(me, ROOT)],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        # 0: all passed; 1: cases outside their bound, the GPU is fine and the other legs still run; anything else (a signal, an
        # abort, the exit of _run, no tests) ends the test here
        assert r.returncode in (0, 1), (n, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], (n, r.stdout[-800:])
        ran = json.load(open(report))
        print("leg %s: %d instantiations" % (n, len(ran["cells"])))
        print("\n".join(l for l in r.stdout.splitlines() if "error / bound" in l or l.startswith(("FAILED", "E  "))))
        for k in ("cells", "route"):
            for name, v in ran[k].items():
                (cells if k == "cells" else route)[name] = max((cells if k == "cells" else route).get(name, 0.0), v)
        multipass.update(ran["multipass"])
        if r.returncode:
            missed.append((n, [l for l in r.stdout.splitlines() if l.startswith("FAILED")]))
    print(_table(cells, route))
    worst = {}
    for name, v in route.items():
        D = int(name.split("-D")[1].split("-")[0])
        worst[D] = max(worst.get(D, 0.0), v)
    print("dense route, worst ratio per D: %s; caps %s" % (json.dumps(worst, sort_keys=True), json.dumps(mr.CAP, sort_keys=True)))
    assert set(cells) == set(mr.INSTANTIATIONS), sorted(set(cells) ^ set(mr.INSTANTIATIONS))
    assert set(multipass) == set(mr.INSTANTIATIONS), sorted(set(multipass) ^ set(mr.INSTANTIATIONS))
    for name, m in multipass.items():
        assert all(mr.walks([tuple(t) for t in m["types"]])), (name, m)
    assert not missed, missed
