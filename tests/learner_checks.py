"""Checks shared by the device-learner tests (test_gpu_parity.py,
test_learner_shapes_gpu.py, test_ttt_learner_gpu.py) and the parameter starts
they train from."""
import numpy as np


def check_grads_same_masks(L, g, p0, batch, blocks, report=None):
    """fp32 device gradient vs the float64 restatement run with the DEVICE's ReLU
    masks (spai_learner_activation > 0).  BN's beta is 0 at init, so some
    pre-activations sit within fp32 rounding of 0 and take either side of the kink
    depending on the summation order; forcing the device's side in the
    restatement removes those flips, so every entry is held to the bulk bound
    3e-4 * max|g| (fp32 through 2*blocks+3 layers).  The masks may differ from
    the restatement's own (pre > 0) only where its pre-activation is within
    1e-4 of its layer's scale of zero: a flip anywhere else fails.
    report: optional dict that receives "err" (max|dg| / max|g|) and "flips"."""
    import learner_ref as LR
    nl = 2 * blocks + 3
    masks = [L.activation(l) > 0 for l in range(nl)]
    diag = {}
    n = len(p0)
    _, _, _, _, ref = LR.train_step(p0, np.zeros(n), np.zeros(n), 0, *batch, blocks, 64, masks=masks, diag=diag)
    flips = 0
    for l in range(nl):
        pre = diag["pre"][l]
        diff = masks[l] != (pre > 0)
        flips += int(diff.sum())
        assert np.all(np.abs(pre[diff]) <= 1e-4 * np.abs(pre).max()), (l, np.abs(pre[diff]).max())
    d, m = np.abs(g - ref), np.abs(ref).max()
    print("grad vs f64 (device masks) %.3g of max|g|, flips %d, bar 3e-4" % (d.max() / m, flips))
    if report is not None:
        report.update(err=d.max() / m, flips=flips)
    assert d.max() <= 3e-4 * m, (d.max() / m, flips)
    return flips


def start_params(init, layout, start, seed):
    """`init` as it is ("init": gamma U(0, 1), beta 0, conv biases 0, running mean 0 and
    variance 1) or made trained-like by bf16_ref.trained_like ("trained": every one
    of those non-trivial, gamma U(0.5, 1.5) with every 11th negative)"""
    import bf16_ref as R
    assert start in ("init", "trained")
    return init if start == "init" else R.trained_like(init, layout, seed)


def check_momentum_blend_is_tested(p0, P1_ref, convs):
    """With trained-like parameters the running-mean check of check_learner_params at
    step 1 (rtol 1e-4, atol 1e-5) can tell the blend 0.9 old + 0.1 batch mean from
    both of its halves: the reference's new running mean differs from 0.1 * batch
    mean (the old term lost) and from the old value (no update) by more than that
    tolerance in every conv layer.  Returns the two smallest per-layer maxima, in
    units of the tolerance."""
    p0 = np.asarray(p0, np.float64)
    worst = [np.inf, np.inf]
    for c in convs:
        sl = slice(c["mu"], c["mu"] + c["co"])
        old, new = p0[sl], P1_ref[sl]
        tol = 1e-5 + 1e-4 * np.abs(new)
        for k, other in enumerate((new - 0.9 * old, old)):   # 0.1 * batch mean; the old value
            over = (np.abs(new - other) / tol).max()
            assert over > 1.0, (k, over)
            worst[k] = min(worst[k], over)
    return worst
