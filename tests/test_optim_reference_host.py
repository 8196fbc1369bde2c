"""tests/optim_reference.py itself, without a GPU: the float64 step equals the package's CPU optimiser and the TF-op shim's; on the
kernel test's own inputs every wrong optimiser of MUTATIONS is told from the right one by far more than the bound, while a float32
restatement of the kernel's arithmetic stays inside it; and the same restatement keeps every step of the adversarial gradient
histories under formats.adam_step_bound."""
import os
import sys

import numpy as np
import pytest
import torch

import optim_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "oracle", "tf13_shim")
HYPER = R.KERNEL_HYPER


def _five_steps(seed, shapes, scales):
    rng = np.random.default_rng(seed)
    w0 = [rng.uniform(-1, 1, s) for s in shapes]
    grads = [[rng.uniform(-1, 1, s) * k * f for s, k in zip(shapes, scales)] for f in (1.0, 0.3, 3.0, 0.6, 2.5)]
    return w0, grads


def test_reference_equals_the_cpu_optimizer(pkg):
    """Five steps with a different gradient each (variables below, across and far above the clip norm, one without a gradient in
    steps 2 and 3): step(..., round_args=False) == clip_by_norm_ + TFAdam.apply_gradients on float64 tensors to 1e-12."""
    shapes, scales = [(6, 5), (40,), (3, 7, 2), (1,)], [0.01, 1.0, 30.0, 0.3]
    w0, grads = _five_steps(1, shapes, scales)
    ws = [torch.from_numpy(x.copy()) for x in w0]
    opt = pkg.train.TFAdam(ws)
    assert not opt.fused
    p, m, v = [x.copy() for x in w0], [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    for t, gs in enumerate(grads, 1):
        active = [1, 0 if t in (2, 3) else 1, 1, 1]
        tg = [torch.from_numpy(g.copy()) if a else None for g, a in zip(gs, active)]
        pkg.train.clip_by_norm_(tg, 1.0)
        opt.apply_gradients(tg)
        want = R.step(p, gs, m, v, t, 1.0, active=active, round_args=False, **HYPER)
        p, m, v = want["p"], want["m"], want["v"]
        for i in range(len(shapes)):
            for got, ref in ((ws[i], p[i]), (opt.m[i], m[i]), (opt.v[i], v[i])):
                np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-12 * max(1.0, float(np.abs(ref).max())))
    assert opt.t == 5


def test_reference_equals_the_tf_op_shim():
    """The same five steps through the shim's tf.clip_by_norm + tf.train.AdamOptimizer, driven as chem_tensorflow.py:183-191 drives
    them (the gradient of sum(w * a) is the fed a).  The shim computes in float32 with 1 - b taken from the double b, the kernel's
    arguments have 1 - fl(b): the two differ by u / (1 - b) relative (6e-7 for m, 6e-5 for v), so the slots agree to twice that of
    their largest entry plus float32 rounding, and the weights (updates of 1e-3 on weights of magnitude 1) to 3e-7, the figure of
    test_clip_by_norm_and_adam_closed_form."""
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import tensorflow as tf
    assert tf.__version__.endswith("shim")
    shapes, scales = [(6, 5), (40,), (12, 3)], [0.01, 1.0, 30.0]
    w0, grads = _five_steps(2, shapes, scales)
    w0 = [x.astype(np.float32) for x in w0]
    grads = [[g.astype(np.float32) for g in gs] for gs in grads]
    with tf.Graph().as_default():
        vs = [tf.Variable(x, name="w%d" % i) for i, x in enumerate(w0)]
        feeds = [tf.placeholder(tf.float32, list(s)) for s in shapes]
        loss = tf.reduce_sum(vs[0] * feeds[0]) + tf.reduce_sum(vs[1] * feeds[1]) + tf.reduce_sum(vs[2] * feeds[2])
        optimizer = tf.train.AdamOptimizer(HYPER["lr"])
        gv = optimizer.compute_gradients(loss, var_list=vs)
        clipped = [(tf.clip_by_norm(g_, 1.0), var) for g_, var in gv]
        train = optimizer.apply_gradients(clipped)
        sess = tf.Session()
        sess.run(tf.global_variables_initializer())
        p, m, v = list(w0), [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
        for t, gs in enumerate(grads, 1):
            sess.run(train, feed_dict=dict(zip(feeds, gs)))
            want = R.step(p, gs, m, v, t, 1.0, **HYPER)
            p, m, v = want["p"], want["m"], want["v"]
            for i, var in enumerate(vs):
                np.testing.assert_allclose(sess.run(var), p[i], rtol=0, atol=3e-7)
                for slot, ref, b in zip(optimizer.slots[var], (m[i], v[i]), (HYPER["b1"], HYPER["b2"])):
                    np.testing.assert_allclose(sess.run(slot), ref, rtol=0, atol=(2 * R.U / (1 - b) + 8 * R.U) * float(np.abs(ref).max()))


# ---- the kernel test's inputs --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1.0, 1e-3], ids=["w1", "w1e-3"])
def trajectory(request):
    """The five steps of the kernel test from weights of the given magnitude: per step the float32 state before it, the gradient,
    the float64 reference of the step and the state after it as the float32 restatement of the kernel computes it."""
    p0, grads = R.kernel_inputs(request.param)
    p, m, v = p0, [np.zeros_like(x) for x in p0], [np.zeros_like(x) for x in p0]
    steps = []
    for t, gs in enumerate(grads, 1):
        want = R.step(p, gs, m, v, t, R.KERNEL_CLIP, **HYPER)
        got = R.kernel_f32(p, gs, m, v, t, R.KERNEL_CLIP, **HYPER)
        steps.append({"t": t, "p": p, "m": m, "v": v, "g": gs, "want": want, "got": got})
        p, m, v = got
    return steps


def test_inputs_mix_clipped_and_unclipped_neighbours(trajectory):
    for s in trajectory:
        clipped = [n > R.KERNEL_CLIP for n in s["want"]["norm"]]
        assert any(a != b for a, b in zip(clipped, clipped[1:])), clipped
        assert clipped[R.KERNEL_SIZES.index(40000)] and clipped[R.KERNEL_SIZES.index(307205)] and not clipped[R.KERNEL_SIZES.index(1025)]
    mid = R.KERNEL_SIZES.index(1023)
    assert {s["want"]["norm"][mid] > R.KERNEL_CLIP for s in trajectory} == {True, False}
    assert all(abs(n / R.KERNEL_CLIP - 1) > 0.05 for s in trajectory for n in s["want"]["norm"] if n > 0)     # no variable sits on the edge


def _catchers(trajectory, mutation):
    """[(step, numel, clipped, worst ratio)] of the variables and steps where the mutant's output is outside the bound by >= 100 C."""
    out = []
    for s in trajectory:
        bad = R.step(s["p"], s["g"], s["m"], s["v"], s["t"], R.KERNEL_CLIP, mutation=mutation, **HYPER)
        for i, r in enumerate(R.ratios(bad["p"], bad["m"], bad["v"], s["want"])):
            if max(r) >= 100 * R.C:
                out.append((s["t"], R.KERNEL_SIZES[i], s["want"]["norm"][i] > R.KERNEL_CLIP, max(r)))
    return out


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutant_is_far_outside_the_bound(trajectory, mutation):
    """On the kernel test's inputs each wrong optimiser, started from the right state of every step, leaves the bound by at least
    100 C for some variable and step (the weakest, eps inside the root, by 1.7e7); which ones catch it is what the shapes and scales
    were chosen for."""
    caught = _catchers(trajectory, mutation)
    print(mutation, "caught by (step, numel, clipped, ratio):", [(t, n, c, "%.3g" % r) for t, n, c, r in caught])
    assert caught, mutation
    if mutation == "first_block_norm":              # only a variable above one block whose norm exceeds the clip
        assert all(n > R.BLOCK and c for _, n, c, _ in caught) and {n for _, n, _, _ in caught} >= {40000, 307205}
    if mutation in ("no_clip", "clip_on_m"):        # only where the norm exceeds the clip
        assert all(c for _, _, c, _ in caught)
    if mutation == "l1_norm":                       # only where the L1 norm exceeds the clip: never the variables of scale 1e-4 and 1e-7
        assert any(c for _, _, c, _ in caught) and not {n for _, n, _, _ in caught} & {3, 1025}
    if mutation == "global_norm":                   # the unclipped neighbours of clipped variables
        assert any(not c for _, _, c, _ in caught)
    if mutation in ("swapped_betas", "no_bias_correction"):    # every step: a wrong bias correction after step 2 is seen too
        assert {t for t, _, _, _ in caught} == {1, 2, 3, 4, 5}


def test_float32_restatement_of_the_kernel_stays_inside_the_bound(trajectory):
    """The reference alone: the kernel's arithmetic in float32 (block sums of 1024 as a 256-way tree, the strided sum of the block
    partials plus the tree, the update, one rounding per operation) meets the bounds with C = 16 on these inputs, so the inputs
    do not make the bound unreachable.  Worst ratios here: m 3.9, v 6.3, p 4.0."""
    worst = np.zeros(3)
    for s in trajectory:
        worst = np.maximum(worst, np.max(R.ratios(*s["got"], s["want"]), axis=0))
    print("float32 restatement: worst C  m %.2f  v %.2f  p %.2f" % tuple(worst))
    assert (worst <= R.C).all(), worst
    assert (worst > 0.5).all(), worst                 # (and the bound is not slack by orders of magnitude)


def test_restated_norm_is_the_norm():
    rng = np.random.default_rng(3)
    for n in (1, 3, 1023, 1024, 1025, 40000, 307205):
        g = R.draw_gradient(rng, n, 0.5)
        want = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        assert abs(float(R.norm_f32(g)) - want) <= 8 * R.U * want


# ---- the per-step bound behind the f16x2 range proof ----------------------------------------------------------------------------
@pytest.mark.parametrize("flush", [False, True], ids=["denormals", "flushed"])
def test_step_bound_holds_in_float32(pkg, flush):
    """The adversarial histories of test_adam_step_bound_holds_against_adversarial_gradients through the float32 restatement of the
    kernel (one element per history, clipping off, from p = 0): every |p_after - p_before| <= adam_step_bound + ulp(p), and the
    worst step exceeds 0.5 lr.  Worst step here: 2.87 lr, 0.40 of the bound, with and without flushed denormals."""
    lr, b1, b2, eps = (HYPER[k] for k in ("lr", "b1", "b2", "eps"))
    bound = pkg.formats.adam_step_bound(lr, b1, b2)
    hist = R.adversarial_histories(b1, b2).astype(np.float32)
    n = hist.shape[0]
    p, m, v = (np.zeros(n, np.float32) for _ in range(3))
    worst = 0.0
    for t in range(1, hist.shape[1] + 1):
        (q,), (m,), (v,) = R.kernel_f32([p], [hist[:, t - 1]], [m], [v], t, None, lr, b1, b2, eps, flush_denormals=flush)
        delta = np.abs(q.astype(np.float64) - p.astype(np.float64))
        assert np.isfinite(q).all() and (delta <= bound + np.spacing(np.abs(q)).astype(np.float64)).all(), (t, float(delta.max()))
        worst = max(worst, float(delta.max()))
        p = q
    print("float32 restatement: worst step %.3f lr = %.3f of adam_step_bound" % (worst / lr, worst / bound))
    assert 0.5 * lr < worst <= bound
