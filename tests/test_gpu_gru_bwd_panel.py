"""The column-panel GRU backward (csrc/ggnn_gru_bwd_panel.hip: hidden sizes 128 / 192 / 256 behind ggnn_gru_bwd_fused_f32 and its
gather form) against the header's formulas in float64 -- the construction of
test_gpu_train_gradients.py::test_fused_gru_backward_against_fp64 -- and against the three-launch route it replaces
(backward._gru_backward_unfused: stage1 / dx_cand / dx_gates, the same sums accumulated in f32) on the same inputs."""
import numpy as np
import pytest
import torch

from test_gpu_train_gradients import U32, _gru_bwd_formulas

pytestmark = pytest.mark.gpu

# Absolute cap of |got - want| / (2^-24 m) per hidden size: the next power of two above 2x the worst ratio of the UNFUSED route,
# and 32 (the small sizes' constant) where that comes out at or below 32.  Measured on the MI355X, worst over every case of this
# file (V = 1 .. 100003, nx = 1 .. 3, tanh / ReLU, mean / sum, plain / gather), split-form matrix path:
#     D      unfused route          fused panel kernel
#     128    6.46 (V=100003, nx=1)  8.02 (V=100003, nx=3)
#     192    7.09 (V=100003, nx=2)  8.35 (V=100003, nx=3)
#     256    6.68 (V=100003, nx=3)  9.12 (V=100003, nx=1)
# 2 x 7.09 = 14.2 -> 16, which is below 32: 32 at every size.  At V = 1 both routes sit at 2.3-3.7, at V = 4099 at 4.5-7.3; the
# fused kernel's worst ratio was 1.0-1.64x the unfused route's in every case.
GRU_BWD_PANEL_C = {128: 32.0, 192: 32.0, 256: 32.0}
NAMES = ["dpc", "dpg", "rh", "dh"]


def _case(pkg, cuda, V, D, nx, T=4):
    gen = torch.Generator(device=cuda).manual_seed(V * 1000 + D * 10 + nx)
    rnd = lambda *s, scale=1.0: ((torch.rand(*s, generator=gen, device=cuda, dtype=torch.float64) * 2 - 1) * scale).float()
    c = {"V": V, "D": D, "nx": nx, "T": T}
    c["h"] = rnd(V, D)
    c["xs"] = [rnd(V, D) for _ in range(nx)]
    c["Wg"] = rnd((nx + 1) * D, 2 * D, scale=(6.0 / ((nx + 2) * D)) ** 0.5)
    c["Wc"] = rnd((nx + 1) * D, D, scale=(6.0 / ((nx + 2) * D)) ** 0.5)
    c["bg"], c["bc"] = 1 + rnd(2 * D, scale=0.2), rnd(D, scale=0.2)
    c["g"] = rnd(V, D)
    nin = torch.randint(0, 3, (V, T), generator=gen, device=cuda).float()
    nin[torch.rand(V, generator=gen, device=cuda) < 0.2] = 0                      # rows without incoming messages
    c["nin"] = nin
    # the gather form's extra rows: node v owns 0..4 rows of Z, not adjacent
    counts = torch.randint(0, 5, (V,), generator=gen, device=cuda)
    R = int(counts.sum())
    Z = rnd(max(R, 1), D)
    perm = torch.randperm(max(R, 1), generator=gen, device=cuda)[:R].to(torch.int32)
    start = torch.cumsum(counts, 0) - counts
    heads = torch.full((V, 4), -1, dtype=torch.int32, device=cuda)
    zsum = torch.zeros(V, D, dtype=torch.float64, device=cuda); zabs = torch.zeros_like(zsum)
    for k in range(4):
        has = counts > k
        heads[has, k] = perm[start[has] + k]
        zk = Z.double()[heads[:, k].clamp_min(0).long()] * has[:, None]
        zsum += zk; zabs += zk.abs()
    c["Z"], c["heads"], c["zsum"], c["zabs"] = Z, heads, zsum, zabs
    return c


def _forward_fp64(c, act):
    """r, u, c of an fp64 forward, rounded to fp32: the kernel's inputs."""
    f64 = lambda t: t.double()
    D = c["D"]
    fn = torch.tanh if act == "tanh" else torch.relu
    X = torch.cat([f64(x) for x in c["xs"]], 1)
    gates = torch.sigmoid(torch.cat([X, f64(c["h"])], 1) @ f64(c["Wg"]) + f64(c["bg"]))
    r64, u64 = gates[:, :D], gates[:, D:]
    c64 = fn(torch.cat([X, r64 * f64(c["h"])], 1) @ f64(c["Wc"]) + f64(c["bc"]))
    return r64.float().contiguous(), u64.float().contiguous(), c64.float().contiguous()


def _want_and_mags(c, r, u, cc, act, use_avg, gather, Wg=None, Wc=None, formulas=_gru_bwd_formulas):
    f64 = lambda t: t.double()
    D, nx = c["D"], c["nx"]
    Wg = f64(c["Wg"] if Wg is None else Wg); Wc = f64(c["Wc"] if Wc is None else Wc)
    den = c["nin"].double().sum(1, keepdim=True) + float(np.float32(1e-7)) if use_avg else None
    geff = f64(c["g"]) + (c["zsum"] if gather else 0)
    want = formulas(geff, f64(c["h"]), f64(r), f64(u), f64(cc), Wg, Wc, nx, act, den)
    ga = f64(c["g"]).abs() + (c["zabs"] if gather else 0)                       # magnitudes: the same formulas on absolute values
    ra, ua, ca, ha = f64(r), f64(u), f64(cc), f64(c["h"]).abs()
    mdact = (1 + ca * ca) if act == "tanh" else (ca > 0).double()
    mpc = ga * (1 - ua) * mdact
    mpu = ga * (ha + ca.abs()) * ua * (1 - ua)
    mrh = mpc @ Wc[nx * D:].abs().t()
    mpg = torch.cat([mrh * ha * ra * (1 - ra), mpu], 1)
    mags = [mpc, mpg, ra * ha, ga * ua + mrh * ra + mpg @ Wg[nx * D:].abs().t(),
            [mpc @ Wc[s * D:(s + 1) * D].abs().t() + mpg @ Wg[s * D:(s + 1) * D].abs().t() for s in range(nx)]]
    if use_avg:
        mags[4][-1] = mags[4][-1] / den
    return want, mags


def _flat(o):
    return list(o[:4]) + list(o[4])


def _ratios(got, want, mags):
    """Worst |got - want| / (2^-24 m) per output (None entries of `got`: not produced by that route)."""
    out = []
    for a, b, m in zip(_flat(got), _flat(want), _flat(mags)):
        if a is None:
            out.append(0.0)
            continue
        err = (a.double() - b).abs()
        out.append(float((err / (U32 * m + 1e-300)).max()) if err.numel() else 0.0)
    return out


def _unfused(pkg, c, geff32, r, u, cc, act, use_avg):
    """The parent route's launches on the same inputs -> (dpc, dpg, None, dh, dx list)."""
    lib = pkg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    dpc, dpg, dh, dinc, d_res, *_ = pkg.backward._gru_backward_unfused(
        lib, geff32, c["h"], r, u, cc, c["Wg"], c["Wc"], c["nin"], c["xs"], c["nx"], c["T"], pkg.ops.ACT_IDS[act], use_avg, st)
    return dpc, dpg, None, dh, list(d_res) + [dinc]


@pytest.mark.parametrize("nx", [1, 2, 3])
@pytest.mark.parametrize("D", [128, 192, 256])
@pytest.mark.parametrize("V", [1, 17, 4099, 100003])
def test_panel_gru_backward_against_fp64(pkg, cuda, V, D, nx):
    """Every output (dpc, dpg, r*h, dh, each dx) of ggnn_gru_bwd_fused_f32 and its gather form at the panel sizes, tanh and ReLU,
    mean (with in-degree-0 rows) and sum aggregation: per element |got - want| <= C 2^-24 m.  K reaches 4 D = 1024 summands here,
    so C is measured against the unfused route on the same inputs, live:
      (a) the fused kernel's worst ratio of this test is at most 2x the unfused route's (a different summation order over the same
          number of terms; a formula error is orders of magnitude larger);
      (b) it is at most GRU_BWD_PANEL_C[D] (measured values at the constant)."""
    ops = pkg.ops
    c = _case(pkg, cuda, V, D, nx)
    packed = ops.PackedWeights().gru_bwd(c["Wg"], c["Wc"], nx, D)
    worst_fused, worst_unfused, where = 0.0, 0.0, None
    for act in ("tanh", "relu"):
        r, u, cc = _forward_fp64(c, act)
        for use_avg in (True, False):
            for gather in (False, True):
                got = ops.gru_bwd_fused(c["g"], c["h"], r, u, cc, packed, c["nin"], use_avg, nx, act,
                                        gather=(c["Z"], c["heads"]) if gather else None)
                again = ops.gru_bwd_fused(c["g"], c["h"], r, u, cc, packed, c["nin"], use_avg, nx, act,
                                          gather=(c["Z"], c["heads"]) if gather else None)
                for a, b in zip(_flat(got), _flat(again)):                      # bit-reproducible
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
                want, mags = _want_and_mags(c, r, u, cc, act, use_avg, gather)
                rf = _ratios(got, want, mags)
                geff32 = (c["g"].double() + c["zsum"]).float() if gather else c["g"]
                ru = _ratios(_unfused(pkg, c, geff32, r, u, cc, act, use_avg), want, mags)
                if max(rf) > worst_fused:
                    i = int(np.argmax(rf))
                    worst_fused, where = max(rf), (act, use_avg, gather, NAMES[i] if i < 4 else "dx%d" % (i - 4))
                worst_unfused = max(worst_unfused, max(ru))
    print("gru_bwd_panel V=%d D=%d nx=%d: worst ratio fused %.2f %s, unfused %.2f" % (V, D, nx, worst_fused, where, worst_unfused))
    assert worst_fused <= 2.0 * worst_unfused, (where, worst_fused, worst_unfused)
    assert worst_fused <= GRU_BWD_PANEL_C[D], (where, worst_fused)


@pytest.mark.parametrize("D", [128, 192, 256])
def test_panel_gru_backward_comparison_has_teeth(pkg, cuda, D):
    """The bound rejects one weight block scaled by 1.001 and an expected dh without its drh*r term."""
    ops = pkg.ops
    V, nx, act = 4099, 2, "tanh"
    c = _case(pkg, cuda, V, D, nx)
    r, u, cc = _forward_fp64(c, act)
    got = ops.gru_bwd_fused(c["g"], c["h"], r, u, cc, ops.PackedWeights().gru_bwd(c["Wg"], c["Wc"], nx, D), c["nin"], True, nx, act)
    want, mags = _want_and_mags(c, r, u, cc, act, True, False)
    assert max(_ratios(got, want, mags)) <= GRU_BWD_PANEL_C[D]
    for blk in range(nx + 1):                                                   # a block of Wg, then of Wc
        for which in ("Wg", "Wc"):
            W = c[which].clone()
            W[blk * D:(blk + 1) * D] *= 1.001
            bad, _ = _want_and_mags(c, r, u, cc, act, True, False, **{which: W})
            assert max(_ratios(got, bad, mags)) > GRU_BWD_PANEL_C[D], (which, blk)

    def no_drh_r(g, h, r_, u_, c_, Wg, Wc, nx_, act_, den):
        out = _gru_bwd_formulas(g, h, r_, u_, c_, Wg, Wc, nx_, act_, den)
        drh = out[0] @ Wc[nx_ * D:].t()
        return out[0], out[1], out[2], out[3] - drh * r_, out[4]
    bad, _ = _want_and_mags(c, r, u, cc, act, True, False, formulas=no_drh_r)
    assert _ratios(got, bad, mags)[3] > GRU_BWD_PANEL_C[D]


def test_panel_gru_backward_empty_graph(pkg, cuda):
    """V = 0: nothing is launched, the outputs come back empty."""
    ops = pkg.ops
    D, nx = 128, 1
    c = _case(pkg, cuda, 1, D, nx)
    e = torch.empty((0, D), dtype=torch.float32, device=cuda)
    out = ops.gru_bwd_fused(e, e, e, e, e, ops.PackedWeights().gru_bwd(c["Wg"], c["Wc"], nx, D), torch.empty((0, 4), device=cuda), True, nx, "tanh")
    torch.cuda.synchronize()
    assert all(t.shape[0] == 0 for t in _flat(out))
