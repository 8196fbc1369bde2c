"""Every instantiation of the fused GRU forward -- the ring, hot, wide, panel and f32 families of csrc/ggnn_gru_cells.hpp, behind
ggnn_gru_packed_f32 / ggnn_gru_packed_gather[_train]_f32 -- against the TF-1.3 GRUCell in float64 (tests/gru_fwd_ref.py), per
element, inside a-priori bounds.

Which instantiation runs depends on the launch, on the ring form (ggnn_gru_form_set) and on switches the library reads once per
process, so the cases are FOUND, not listed: ggnn_gru_describe (the launchers' own selection function) is swept on the host and
every cell gets the argument tuples that select it; every case first asserts, through the same query, that it selects the cell the
test is named after IN THIS PROCESS.  The legs -- the split matrix path, GGNN_MATRIX=f32, and that with GGNN_GRU_NOSAVE_KERNEL=1
-- are this process plus one child pytest process over this file per other leg; each writes the cells it ran to a report and the
parent asserts that between them every cell of ggnn_gru_cells ran.

Per cell: V = 1, 15, 16, 17, 63, 65 and one full round of the cell's workgroups plus 40 rows (from the geometry the query
returns), over the variants of activation, aggregation, T, ticket source and save buffers that select the cell.  Every launch runs
twice (bit-identical); h' -- and r, u, c, incoming where the launch saves them -- must be inside the bound; node 0, which
receives no message, has an exactly zero gathered row.

The factor over the bound is measured, not chosen: the generic two-launch GRU (ggnn_gru_gates_f32 + ggnn_gru_candidate_f32:
independent code on the f32 MFMA, for gather cells fed ggnn_gather_segment_sum_f32's output) runs on the same inputs and a cell
passes if its worst error / bound ratio is at most 2 x that route's over the same cases (another order of summation over the same
number of terms) AND at most gru_fwd_ref.CAP[D], the next power of two above 2 x the route's worst ratio over the whole file.
tests/test_gru_fwd_ref_host.py shows that float32 and the f16x2 operand format stay inside factor 1 and that wrong results of
eight kinds fail at CAP.  A cap is not raised to make a cell pass.

Measured worst error / bound (MI355X; all legs, all cases of every cell of a hidden size and format):
    D   format  fused: h_out     r         u         c         incoming | two-launch: h_out     r         u         c         incoming
   32   bf16x3         0.150     0.226     0.322     0.174     0.580    |             0.178     0.341     0.321     0.229     0.580
   32   f16x2          0.120     0.205     0.199     0.137     0.580    |             0.178     0.341     0.321     0.229     0.580
   32   f32            0.178     0.384     0.345     0.250     0.580    |             0.178     0.384     0.345     0.250     0.580
   64   bf16x3         0.168     0.303     0.382     0.219     0.580    |             0.165     0.394     0.411     0.208     0.580
   64   f16x2          0.117     0.241     0.225     0.172     0.580    |             0.165     0.394     0.411     0.208     0.580
   64   f32            0.165     0.394     0.411     0.241     0.580    |             0.165     0.394     0.411     0.241     0.580
  100   bf16x3         0.152     0.329     0.347     0.184     0.592    |             0.197     0.405     0.423     0.262     0.592
  100   f16x2          0.113     0.273     0.247     0.133     0.592    |             0.197     0.405     0.423     0.262     0.592
  100   f32            0.197     0.441     0.423     0.241     0.592    |             0.197     0.435     0.423     0.262     0.592
  128   bf16x3         0.152     0.426     0.390     0.190     -        |             0.160     0.445     0.532     0.236     -
  128   f16x2          0.101     0.296     0.297     0.151     -        |             0.160     0.445     0.532     0.236     -
  128   f32            0.166     0.440     0.532     0.236     -        |             0.160     0.445     0.532     0.236     -
  192   bf16x3         0.138     0.405     0.417     0.230     -        |             0.160     0.501     0.507     0.212     -
  192   f16x2          0.120     0.306     0.318     0.208     -        |             0.160     0.501     0.507     0.212     -
  192   f32            0.160     0.525     0.507     0.212     -        |             0.160     0.501     0.507     0.212     -
  256   bf16x3         0.152     0.479     0.461     0.192     -        |             0.150     0.519     0.496     0.226     -
  256   f16x2          0.105     0.298     0.310     0.143     -        |             0.150     0.519     0.496     0.226     -
  256   f32            0.148     0.519     0.496     0.226     -        |             0.150     0.519     0.496     0.226     -
The two-launch route's worst ratio per hidden size: 0.580 (32), 0.580 (64), 0.592 (100), 0.532 (128), 0.507 (192), 0.519 (256);
twice that is between 1.01 and 1.18, so every CAP is 2.  No row of the table is above 1.09 x the route on any output (D = 192, bf16x3,
c: 0.230 against 0.212); the two-piece f16 format sits below the f32 MFMA throughout.  All 233 cells ran, none missed its bound
at factor 1, let alone at the cap.
"""
import json
import os
import subprocess
import sys

import functools
import numpy as np
import pytest
import torch

import gru_fwd_ref as gr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

LEG = os.environ.get("GGNN_GRU_CELLS_LEG")                  # set for the child processes of the legs test: the leg's name
REPORT = os.environ.get("GGNN_GRU_CELLS_REPORT")            # a file that receives what ran
_ran = {"cells": {}, "route": {}}                           # cell id -> {output: ratio}; "D-fmt" -> {output: the two-launch route's}
_cache = []


def _found():
    if not _cache:
        import importlib
        _cache.append(gr.sweep(importlib.import_module(PKG)._lib.load()))
    return _cache[0]


def pytest_generate_tests(metafunc):
    want = [n for n in ("cell_case", "family_case") if n in metafunc.fixturenames]
    if not want:
        return
    try:
        found = _found()
    except Exception as e:                                   # (no library: the tests fail with the reason, the collection goes on)
        for n in want:
            metafunc.parametrize(n, [e], ids=["library-not-loaded"])
        return
    items = sorted(found.items())
    if "cell_case" in want:
        metafunc.parametrize("cell_case", items, ids=[gr.cell_id(c) for c, _ in items])
    if "family_case" in want:
        first = {}
        for c, a in items:
            first.setdefault(gr.FAMILIES[c[0]], (c, a))
        metafunc.parametrize("family_case", list(first.values()), ids=list(first))


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        with open(REPORT, "w") as f:
            json.dump(_ran, f, indent=1, sort_keys=True)


def _variants(args):
    """The primary tuple, then tuples until every value of save / act / use_avg / T / tickets that selects the cell is covered."""
    fields = ("save", "act", "use_avg", "T", "tickets")
    chosen, covered = [], set()
    for a in args:
        new = {(f, getattr(a, f)) for f in fields} - covered
        if not chosen or new:
            chosen.append(a)
            covered |= new
    return chosen


class _Packed:
    """The stage images per (D, nx, format), packed once (ops.PackedWeights caches them per weight tensor)."""
    def __init__(self):
        self.pw = None

    def gru(self, Wg, Wc, nx, D, fmt):
        if self.pw is None:
            self.pw = sys.modules[PKG].ops.PackedWeights()
        return self.pw.gru(Wg, Wc, nx, D, fmt)


_PACKED = _Packed()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=8)
def _weights(D, nx):
    return tuple(dev(w) for w in gr.weights(D, nx))


@functools.lru_cache(maxsize=48)
def _device(D, V, T, gather):
    """Device tensors shared by every case at these sizes; never written."""
    c = gr.make_case(D, 3, V, gather, T)
    d = dict(h=dev(c.h), res=[dev(r) for r in c.res])
    if gather:
        d.update(H=dev(c.H), adj=[dev(a) for a in c.adj], nin=dev(c.nin))
        d["index"] = sys.modules[PKG].ops.build_message_index(d["adj"], V)
    else:
        d.update(x_last=dev(c.x_last))
    return d


def _reference(key):
    """(float64 reference, bounds, the two-launch route's worst ratios) of a case: computed once, shared, left unchanged (the
    large cases, tens of megabytes each, in a small cache of their own: consecutive cells share them)."""
    return (_reference_large if key[2] > 1024 else _reference_small)(key)


def _reference_of(key):
    D, nx, V, gather, T, use_avg, act = key
    c = gr.make_case(D, nx, V, gather, T, use_avg, act)
    ref, bound = gr.bounds(c)
    pkg = sys.modules[PKG]
    d = _device(D, V, T if gather else 0, bool(gather))
    Wg, bg, Wc, bc = _weights(D, nx)
    xs = d["res"][:nx - 1]
    got = {}
    if gather:
        got["incoming"] = pkg.ops.gather_segment_sum(d["H"], d["index"], d["nin"] if use_avg else None, None, bool(use_avg))
        xs = xs + [got["incoming"]]
    else:
        xs = xs + [d["x_last"]]
    save = {}
    got["h_out"] = pkg.ops.gru(xs, d["h"], Wg, bg, Wc, bc, act, save=save, two_launch=True)
    got.update(save)
    route = {k: gr.worst_ratio(v.cpu().numpy(), ref[k], bound[k]) for k, v in got.items()}
    return ref, bound, route


_reference_large = functools.lru_cache(maxsize=3)(_reference_of)
_reference_small = functools.lru_cache(maxsize=512)(_reference_of)


def _launch(pkg, a, V, cnt):
    """One fused launch of the argument tuple at V rows: ({output: host array}, the case's key)."""
    d = _device(a.D, V, a.T if a.gather else 0, bool(a.gather))
    Wg, bg, Wc, bc = _weights(a.D, a.nx)
    packed = _PACKED.gru(Wg, Wc, a.nx, a.D, a.fmt)
    save = {} if a.save else None
    counter = None
    if a.tickets:
        cnt.zero_()
        counter = cnt
    if a.gather:
        out = pkg.ops.gru_packed_gather(d["res"][:a.nx - 1], d["h"], packed, bg, bc, d["H"].view(V * a.T, a.D), d["index"], None,
                                        d["nin"] if a.use_avg else None, activation=a.act, tile_counter=counter, save=save, fmt=a.fmt)
    else:
        out = pkg.ops.gru_packed(d["res"][:a.nx - 1] + [d["x_last"]], d["h"], packed, bg, bc, activation=a.act, tile_counter=counter,
                                 fmt=a.fmt, save=save)
    got = dict(h_out=out)
    got.update(save or {})
    if a.tickets:                                                       # (the panel kernel deals its tickets statically and ignores the counter)
        assert (int(cnt[0]) > 0) == (a.D < 128), "the ticket counter: %d" % int(cnt[0])
    return got


def _run(pkg, lib, cell, a, V, cnt):
    """The case twice (bit-identical) -> {output: host array}.  A missed bound lets the session go on; an ERROR of the library or
    the runtime ends it here (pytest.exit), so that nothing more is started on a GPU that may have faulted -- a leg's parent sees
    the exit status and starts no further leg."""
    prev = lib.ggnn_gru_form_set(a.form)
    try:
        rc, got_cell, _ = gr.describe(lib, a, form=-1)
        assert rc == 0 and got_cell == cell, (a, gr.cell_id(cell), got_cell, lib.ggnn_last_error())
        try:
            one = _launch(pkg, a, V, cnt)
            two = _launch(pkg, a, V, cnt)
            same = all(torch.equal(one[k], two[k]) for k in one)
            host = {k: v.cpu().numpy() for k, v in one.items()}
        except RuntimeError as e:
            pytest.exit("library or runtime error, nothing more is run: %s" % e, returncode=3)
    finally:
        lib.ggnn_gru_form_set(prev)
    assert same, "two runs differ: %s V=%d" % (a, V)
    return host


def _key(a, V):
    return (a.D, a.nx, V, int(a.gather), a.T if a.gather else 0, a.use_avg if a.gather else 0, a.act)


def _merge(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


def test_cell_matches_float64(pkg, cuda, lib, cell_case):
    cell, args = cell_case
    if isinstance(cell, Exception):
        raise cell
    name, D = gr.cell_id(cell), cell[1]
    variants = _variants(args)
    rc, _, geom = gr.describe(lib, args[0])
    assert rc == 0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [(V, variants[i % len(variants)]) for i, V in enumerate(gr.SMALL_V)] + [(gr.large_v(geom, cus), variants[0])]
    sizes += [(65, a) for a in variants[len(gr.SMALL_V):]]                           # (more variants than small sizes: none is left out)
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    mine, route, failures = {}, {}, []
    _ran["cells"][name] = mine
    for V, a in sizes:
        host = _run(pkg, lib, cell, a, V, cnt)
        ref, bound, rt = _reference(_key(a, V))
        if cell[6] and a.save:
            assert set(host) == ({"h_out", "r", "u", "c", "incoming"} if a.gather else {"h_out", "r", "u", "c"})
        if a.gather and a.save and V > 1:
            assert not host["incoming"][0].any(), "node 0 receives nothing: its gathered row is exactly zero"
        for k, v in host.items():
            try:
                ratio = gr.assert_within(v, ref[k], bound[k], gr.CAP[D], "%s %s V=%d %s" % (name, k, V, tuple(a)))
            except AssertionError as e:
                failures.append(str(e))
                ratio = gr.worst_ratio(v, ref[k], bound[k])
            _merge(mine, {k: ratio})
            _merge(route, {k: rt[k]})
    _merge(_ran["route"].setdefault("%d-%s" % (D, gr.FMT_NAMES[cell[5]]), {}), route)
    print("%s: worst error / bound %s; two-launch route on the same cases %s; cap %g" % (
        name, json.dumps(mine, sort_keys=True), json.dumps(route, sort_keys=True), gr.CAP[D]))      # (the figures first)
    assert not failures, failures
    for k, v in mine.items():
        assert v <= 2 * route[k], "%s %s: worst ratio %.3f is more than twice the two-launch route's %.3f" % (name, k, v, route[k])


def test_comparison_has_teeth(pkg, cuda, lib, family_case):
    """The cap rejects a 1.001 weight block and a candidate computed from h instead of r*h: the EXPECTED values are corrupted,
    never a kernel, and a cell's true output is compared with them at the factor test_cell_matches_float64 uses."""
    cell, args = family_case
    if isinstance(cell, Exception):
        raise cell
    a, V = args[0], 65
    cnt = torch.zeros(1, dtype=torch.int32, device=cuda)
    got = _run(pkg, lib, cell, a, V, cnt)["h_out"]
    D, nx = a.D, a.nx
    c = gr.make_case(*_key(a, V))
    ref, bound = gr.bounds(c)
    gr.assert_within(got, ref["h_out"], bound["h_out"], gr.CAP[D], "uncorrupted")
    Wg = c.Wg.copy(); Wg[:D, :D] *= np.float32(1.001)
    Wc = c.Wc.copy(); Wc[nx * D:, :] *= np.float32(1.001)
    x = np.concatenate([s.astype(np.float64) for s in c.res] + [ref["incoming"]], 1)
    cand = gr._act(c.act, np.concatenate([x, c.h.astype(np.float64)], 1) @ c.Wc.astype(np.float64) + c.bc)
    wrong = {"Wg block x 1.001": gr.forward(c._replace(Wg=Wg))["h_out"], "Wc block x 1.001": gr.forward(c._replace(Wc=Wc))["h_out"],
             "candidate from h": ref["u"] * c.h + (1 - ref["u"]) * cand}
    for what, w in wrong.items():
        with pytest.raises(AssertionError, match="outside"):
            gr.assert_within(got, w, bound["h_out"], gr.CAP[D], what)


def _table(cells, route):
    """The header's table: per hidden size and format, the worst ratio of the fused cells and of the two-launch route."""
    rows = {}
    for name, r in cells.items():
        p = name.split("-")
        key = (int(p[1][1:]), p[3])
        _merge(rows.setdefault(key, {}), r)
    out = ["    D   format  fused: " + "  ".join("%-8s" % k for k in gr.OUTPUTS) + " | two-launch: " + "  ".join("%-8s" % k for k in gr.OUTPUTS)]
    for (D, fmt), r in sorted(rows.items()):
        rt = route.get("%d-%s" % (D, fmt), {})
        f = lambda d: "  ".join("%-8s" % ("%.3f" % d[k] if k in d else "-") for k in gr.OUTPUTS)
        out.append("  %3d   %-6s         %s |             %s" % (D, fmt, f(r), f(rt)))
    return "\n".join(out)


def _is_leg(env_add):
    return all(os.environ.get(k, "") == env_add.get(k, "") for k in ("GGNN_MATRIX", "GGNN_GRU_NOSAVE_KERNEL"))


def test_other_legs_and_every_cell_ran(pkg, cuda, lib, tmp_path):
    """The legs this process is not: one child pytest process over this file each, one at a time, each under its own time limit.
    A child that ends by signal, abort, time limit or a library / runtime error fails the test at once and no further leg is
    started; a child in which only bounds were missed is reported at the end, after the other legs.  Every leg reports the cells it
    ran; their union with what this process ran is ggnn_gru_cells, each cell under its own name, none skipped."""
    if LEG:
        pytest.skip("a leg's own process does not start legs")
    table = {gr.cell_id(c) for c in gr.table(lib)}
    assert len(table) == lib.ggnn_gru_cells(None, 0)
    mine = {gr.cell_id(c) for c in _found()}
    cells, route = dict(_ran["cells"]), {k: dict(v) for k, v in _ran["route"].items()}
    me = os.path.abspath(__file__)
    missed = []
    for n, env_add in gr.LEGS.items():
        if _is_leg(env_add) and mine <= set(cells):
            continue                                                              # (this process is that leg and has run its cells)
        env = {k: v for k, v in os.environ.items() if k not in gr.LEG_VARS}
        env.update(env_add)
        report = str(tmp_path / ("%s.json" % n))
        env.update(GGNN_GRU_CELLS_LEG=n, GGNN_GRU_CELLS_REPORT=report)
        r = subprocess.run([sys.executable, "-m", "pytest", me, "-q", "-m", "gpu", "-p", "no:cacheprovider", "-rfP",
                            "--deselect", "%s::test_other_legs_and_every_cell_ran" % os.path.relpath(me, ROOT)],
                           env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        # 0: all passed; 1: cases outside their bound, the GPU is fine and the other legs still run; anything else (a signal, an
        # abort, the exit of _run, no tests) ends the test here
        assert r.returncode in (0, 1), (n, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], (n, r.stdout[-800:])
        ran = json.load(open(report))
        print("leg %s: %d cells" % (n, len(ran["cells"])))
        print("\n".join(l for l in r.stdout.splitlines() if "error / bound" in l or l.startswith(("FAILED", "E  "))))
        for name, v in ran["cells"].items():
            _merge(cells.setdefault(name, {}), v)
        for k, v in ran["route"].items():
            _merge(route.setdefault(k, {}), v)
        if r.returncode:
            missed.append((n, [l for l in r.stdout.splitlines() if l.startswith("FAILED")]))
    print(_table(cells, route))
    worst = {}
    for k, v in route.items():
        D = int(k.split("-")[0])
        worst[D] = max(worst.get(D, 0.0), max(v.values()))
    print("two-launch route, worst ratio per D: %s; caps %s" % (json.dumps(worst, sort_keys=True), json.dumps(gr.CAP, sort_keys=True)))
    assert set(cells) == table, sorted(set(cells) ^ table)[:10]
    assert all("h_out" in v for v in cells.values())
    assert not missed, missed
