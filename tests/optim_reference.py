"""float64 reference of the optimiser side of the training step -- per-variable tf.clip_by_norm followed by TF-1.3 ApplyAdam
(chem_tensorflow.py:183-191), the step ggnn_clip_adam_f32 (csrc/ggnn_optim.hip) takes for all variables in two launches -- with
the magnitudes its error bounds are stated in, a set of deliberately wrong optimisers, a float32 NumPy restatement of the kernel's
own arithmetic, the inputs of the kernel test, and a hook that records every optimiser step of a model.  A plain module (imported
by the tests), not a conftest.

* step(p, g, m, v, t, clip, lr, b1, b2, eps, active): one step in float64 on the kernel's own arguments: clip, b1, b2 and eps
  rounded to float32 (the ABI passes C floats), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) computed in double from the unrounded
  hyper-parameters as TFAdam.clip_and_apply does and then rounded to float32, 1 - b formed from the rounded b.  With s the clip
  scale of the variable and u = 2^-24 the bounds are
      |dm| <= C u (b1 |m| + (1 - b1) s |g|)
      |dv| <= C u (b2 v + (1 - b2) s^2 g^2)
      |dp| <= u |p_want| + C u lr_t (b1 |m| + (1 - b1) s |g|) / (sqrt(v_want) + eps)
  (first term of the last: the final rounding of p; second: the update), and step returns those magnitudes.
* MUTATIONS: wrong optimisers step(..., mutation=name) computes instead; the host tests show that the kernel test's inputs tell
  each of them from the right one by far more than the bound.
* kernel_f32(...): the kernel's arithmetic in float32 NumPy, reduction order included.
* kernel_inputs(magnitude): the variables and the five gradients of tests/test_gpu_optim.py.
* adversarial_histories(b1, b2): the gradient histories of test_adam_step_bound_holds_against_adversarial_gradients.
* capture_optimizer_steps(model): records t, clip, active flags, gradients and p, m, v before and after every clip_and_apply.
"""
import contextlib
import math

import numpy as np
import torch

U = 2.0 ** -24
BLOCK = 1024                        # floats per block of the flat buffers (ggnn_optim_block_floats)
C = 16.0                            # the bounds' constant: the power of two above 2 x the worst ratio on the MI355X (6.33, test_gpu_optim.py)

MUTATIONS = ("first_block_norm", "global_norm", "l1_norm", "no_clip", "swapped_betas", "eps_in_sqrt", "no_bias_correction",
             "clip_on_m")


def _f32(x):
    return float(np.float32(x))


def kernel_arguments(t, clip, lr, b1, b2, eps, round_args=True):
    """(clip, lr_t, b1, 1 - b1, b2, 1 - b2, eps) as the kernel receives and forms them (as doubles); round_args=False keeps
    every one in double: the arguments of the package's float64 CPU path."""
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    clip = float(clip or 0.0)
    if not round_args:
        return clip, lr_t, b1, 1.0 - b1, b2, 1.0 - b2, eps
    b1, b2 = np.float32(b1), np.float32(b2)
    return _f32(clip), _f32(lr_t), float(b1), float(np.float32(1.0) - b1), float(b2), float(np.float32(1.0) - b2), _f32(eps)


def step(p, g, m, v, t, clip, lr, b1, b2, eps, active=None, mutation=None, round_args=True):
    """One clip + Adam step over lists of arrays, in float64.  -> {"p", "m", "v": the new values; "norm", "scale": per variable;
    "mag_m", "mag_v", "mag_p_round", "mag_p_update": the magnitudes of the bounds}.  A variable with active[i] == 0 keeps p, m and
    v and has zero magnitudes.  clip None or 0: no clipping.  mutation: one of MUTATIONS."""
    assert mutation is None or mutation in MUTATIONS, mutation
    n = len(p)
    active = [1] * n if active is None else [int(a) for a in active]
    d = lambda xs: [np.asarray(x, dtype=np.float64) for x in xs]
    p, g, m, v = d(p), d(g), d(m), d(v)
    clip, lr_t, b1, one_b1, b2, one_b2, eps = kernel_arguments(t, clip, lr, b1, b2, eps, round_args)
    if mutation == "swapped_betas":
        b1, one_b1, b2, one_b2 = b2, one_b2, b1, one_b1
    if mutation == "no_bias_correction":
        lr_t = _f32(lr) if round_args else lr
    if mutation == "global_norm":
        total = math.sqrt(sum(float((x * x).sum()) for x, a in zip(g, active) if a))
    out = {k: [] for k in ("p", "m", "v", "norm", "scale", "mag_m", "mag_v", "mag_p_round", "mag_p_update")}
    for i in range(n):
        if not active[i]:
            for k, x in (("p", p[i]), ("m", m[i]), ("v", v[i])):
                out[k].append(x.copy())
            for k in ("mag_m", "mag_v", "mag_p_round", "mag_p_update"):
                out[k].append(np.zeros_like(p[i]))
            out["norm"].append(0.0); out["scale"].append(1.0)
            continue
        gi = g[i]
        if mutation == "first_block_norm":
            norm = math.sqrt(float((gi.reshape(-1)[:BLOCK] ** 2).sum()))
        elif mutation == "global_norm":
            norm = total
        elif mutation == "l1_norm":
            norm = float(np.abs(gi).sum())
        else:
            norm = math.sqrt(float((gi * gi).sum()))
        s = clip / max(norm, clip) if clip > 0.0 and mutation != "no_clip" else 1.0
        if mutation == "clip_on_m":
            m_new = s * (b1 * m[i] + one_b1 * gi)
            v_new = b2 * v[i] + one_b2 * gi * gi
        else:
            m_new = b1 * m[i] + one_b1 * (s * gi)
            v_new = b2 * v[i] + one_b2 * (s * gi) ** 2
        den = np.sqrt(v_new + eps) if mutation == "eps_in_sqrt" else np.sqrt(v_new) + eps
        p_new = p[i] - lr_t * m_new / den
        mag_m = b1 * np.abs(m[i]) + one_b1 * s * np.abs(gi)
        out["p"].append(p_new); out["m"].append(m_new); out["v"].append(v_new)
        out["norm"].append(norm); out["scale"].append(s)
        out["mag_m"].append(mag_m); out["mag_v"].append(v_new.copy())
        out["mag_p_round"].append(np.abs(p_new)); out["mag_p_update"].append(lr_t * mag_m / (np.sqrt(v_new) + eps))
    return out


def _worst(err, mag, slack=None):
    """max over the elements of (err - slack)+ / (u mag): 0 where the error is within the slack, inf where the magnitude is 0 and the
    error is not, nan where the result is."""
    if err.size == 0:
        return 0.0
    excess = err if slack is None else np.maximum(err - slack, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(excess == 0.0, 0.0, excess / (U * mag))
    return float(np.max(r))


def ratios(got_p, got_m, got_v, want):
    """Per variable the smallest C at which (m, v, p) meet their bounds, want = step(...) on the same inputs."""
    out = []
    for i in range(len(want["p"])):
        f = lambda x: np.asarray(x, dtype=np.float64).reshape(want["p"][i].shape)
        rm = _worst(np.abs(f(got_m[i]) - want["m"][i]), want["mag_m"][i])
        rv = _worst(np.abs(f(got_v[i]) - want["v"][i]), want["mag_v"][i])
        rp = _worst(np.abs(f(got_p[i]) - want["p"][i]), want["mag_p_update"][i], slack=U * want["mag_p_round"][i])
        out.append((rm, rv, rp))
    return out


# ---- the kernel's arithmetic in float32 -------------------------------------------------------------------------------------------
def _tree256(x):
    """The shared-memory reduction of both kernels over the last axis of 256: red[i] += red[i + off], off = 128 .. 1."""
    off = 128
    while off:
        x = x[..., :off] + x[..., off:2 * off]
        off //= 2
    return x[..., 0]


def norm_f32(g):
    """||g|| as the two launches form it: per block of 1024 floats each of 256 threads takes (x^2 + y^2) + (z^2 + w^2) of its float4
    and the block tree-reduces; per variable thread i adds the partials b0 + i, b0 + i + 256, .. in order and the block tree-reduces."""
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    nb = max((g.size + BLOCK - 1) // BLOCK, 1)
    flat = np.zeros(nb * BLOCK, np.float32); flat[:g.size] = g
    sq = flat.reshape(nb, 256, 4) ** 2
    partial = _tree256((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
    rounds = (nb + 255) // 256
    padded = np.zeros(rounds * 256, np.float32); padded[:nb] = partial
    s = np.zeros(256, np.float32)
    for row in padded.reshape(rounds, 256):
        s = s + row
    return np.sqrt(_tree256(s))


def kernel_f32(p, g, m, v, t, clip, lr, b1, b2, eps, active=None, flush_denormals=False):
    """clip_adam_kernel restated in float32 NumPy, one rounding per operation (no contraction into fused multiply-adds).
    flush_denormals: every operand and result below the smallest normal float32 becomes zero.  -> (p, m, v) as float32 lists."""
    f = np.float32
    tiny = np.finfo(np.float32).tiny
    z = (lambda x: np.where(np.abs(x) < tiny, f(0), x).astype(np.float32)) if flush_denormals else (lambda x: x)
    clip, lr_t, b1, _, b2, _, eps = (f(x) for x in kernel_arguments(t, clip, lr, b1, b2, eps))
    one_b1, one_b2 = f(1) - b1, f(1) - b2
    out = ([], [], [])
    with np.errstate(under="ignore"):
        for i in range(len(p)):
            pi, gi, mi, vi = (z(np.asarray(x, dtype=np.float32)) for x in (p[i], g[i], m[i], v[i]))
            if active is not None and not active[i]:
                for o, x in zip(out, (pi, mi, vi)):
                    o.append(x.copy())
                continue
            scale = clip / np.maximum(norm_f32(gi), clip) if clip > 0 else f(1)
            gv = z(gi * scale)
            mv = z(z(mi * b1) + z(gv * one_b1))
            vv = z(z(vi * b2) + z(z(gv * gv) * one_b2))
            dd = z(mv / z(np.sqrt(vv) + eps))
            out[0].append(z(pi - z(lr_t * dd))); out[1].append(mv); out[2].append(vv)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
# The variables of the kernel test: the smallest sizes that reach each path (tails, the block edge, 40 blocks, and 301 blocks: the
# strided loop over the block partials plus a ragged float4 tail).  Base scales of the gradients: with KERNEL_CLIP = 1 the variables
# of scale 30 are always clipped, those of 1e-4 and 1e-7 never, 307205 floats of scale 3e-2 always (norm 9 x the step factor) and
# 1023 floats of scale 3e-2 (norm 0.53 x the step factor) in the steps of factor 3.0 and 2.5 only -- so clipped and unclipped
# variables are neighbours in the flat buffer in every launch.
KERNEL_SIZES = (1, 3, 1023, 1024, 1025, 40000, 307205)
KERNEL_SCALES = (30.0, 1e-4, 3e-2, 30.0, 1e-7, 30.0, 3e-2)
KERNEL_STEP_FACTORS = (1.0, 0.3, 3.0, 0.6, 2.5)
KERNEL_CLIP = 1.0
KERNEL_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def draw_gradient(rng, numel, scale):
    """Uniform in (-scale, scale) with 10 % exact zeros, float32."""
    g = rng.uniform(-1.0, 1.0, numel) * scale
    g[rng.uniform(size=numel) < 0.1] = 0.0
    return g.astype(np.float32)


def kernel_inputs(magnitude, seed=0):
    """(initial weights uniform in (-magnitude, magnitude), [per step: one gradient per variable]) of the kernel test, float32."""
    rng = np.random.default_rng(seed)
    p0 = [(rng.uniform(-1.0, 1.0, n) * magnitude).astype(np.float32) for n in KERNEL_SIZES]
    grads = [[draw_gradient(rng, n, s * factor) for n, s in zip(KERNEL_SIZES, KERNEL_SCALES)] for factor in KERNEL_STEP_FACTORS]
    return p0, grads


def adversarial_histories(b1=0.9, b2=0.999, trials=60, n=400):
    """[trials, n] float64: the gradient histories of test_adam_step_bound_holds_against_adversarial_gradients (test_formats_host.py),
    drawn in the same order from the same generator: noise at a random scale; long silence, then constant large gradients;
    geometric ramps (the Cauchy-Schwarz extremal shape); rare spikes."""
    rng = np.random.default_rng(0)
    out = np.empty((trials, n))
    for trial in range(trials):
        kind = trial % 4
        if kind == 0:
            g = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 3)
        elif kind == 1:
            g = np.concatenate([np.full(n // 2, 1e-12), np.full(n - n // 2, 1e3)])
        elif kind == 2:
            g = (b1 / b2) ** -np.arange(n, dtype=np.float64) * 1e-30
        else:
            g = rng.choice([0.0, 1.0], size=n, p=[0.97, 0.03]) * rng.normal(size=n)
        out[trial] = g
    return out


# ---- a model's optimiser steps ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def capture_optimizer_steps(model):
    """Within the block every TFAdam.clip_and_apply appends {"t": the step it takes, "clip", "names", "active": the flags on the
    device, "g": clones of the flat gradient views, "before" / "after": {"p", "m", "v"} clones of every variable and its slots} to
    the yielded list.  The original clip_and_apply runs unchanged in between."""
    opt = model.optimizer
    assert opt.fused, "the capture reads the flat buffers of the fused optimiser"
    names = {v.data_ptr(): n for n, v in model.named_variables().items()}
    steps = []
    original = opt.clip_and_apply
    clone = lambda ts: [x.detach().clone() for x in ts]
    state = lambda: {"p": clone(opt.vars), "m": clone(opt.m), "v": clone(opt.v)}

    def clip_and_apply(clip_norm):
        rec = {"t": opt.t + 1, "clip": clip_norm, "names": [names[v.data_ptr()] for v in opt.vars],
               "active": opt._flat["active"].clone(), "g": clone(opt._flat["g_views"]), "before": state()}
        result = original(clip_norm)
        rec["after"] = state()
        steps.append(rec)
        return result

    opt.clip_and_apply = clip_and_apply
    try:
        yield steps
    finally:
        del opt.clip_and_apply          # (the class's method again)


def to_numpy(tensors):
    return [x.detach().cpu().numpy().copy() for x in tensors]


def reference_of_captured_step(rec, lr, b1, b2, eps):
    """step(...) on a captured step's own gradient and pre-step state."""
    active = rec["active"].cpu().tolist()
    return step(to_numpy(rec["before"]["p"]), to_numpy(rec["g"]), to_numpy(rec["before"]["m"]), to_numpy(rec["before"]["v"]),
                rec["t"], rec["clip"], lr, b1, b2, eps, active)


def padding_is_zero(opt):
    """The floats of the flat g, m and v buffers that belong to no variable are all exactly zero."""
    f = opt._flat
    pad = torch.ones(f["nblocks"] * f["B"], dtype=torch.bool, device=f["g"].device)
    first = f["var_first"].cpu().tolist()
    for i, v in enumerate(opt.vars):
        pad[first[i] * f["B"]:first[i] * f["B"] + v.numel()] = False
    return all(bool((f[k][pad] == 0).all()) for k in ("g", "m", "v"))
