"""The Connect4 device learner (csrc/learner.hip) at the batch sizes where its
default-path kernels change what they do, and from trained-like parameters.

What each batch size reaches:
  B = 1    42 values per channel in k_bn_fwd / k_bn_bwd; one partial weight-gradient
           chunk (kWgSamples = 4); three of k_linear_bwd_w's four batch quarters empty
  B = 3    still a single, partial chunk
  B = 129  33 chunks: k_wgrad_reduce's `for (b0 ...; b0 += kWgReduceBatch)` makes a
           second trip, with one valid chunk in it
  B = 147  6174 values per channel, 30 past the kBn * kBnPer = 6144 that k_bn_fwd and
           k_bn_bwd keep in registers: the `for (i = threadIdx.x + kBnPer * kBn; ...)`
           re-read loops (sum, variance, output; backward sums, dz) run for the
           first time
  B = 172  1080 values in the re-read loops: threads 0..55 make two trips; 43 chunks
  B = 300  6456 values re-read (6-7 trips per thread), 75 chunks (3 reduce trips)
init_params has beta, the conv biases and the running mean at 0 and the running
variance at 1; bf16_ref.trained_like makes all of them non-trivial and adds
gammas above 1 and below 0, so the running-statistic blend and every factor of
the BatchNorm backward are exercised with values that cannot hide them.
tests/test_learner_ref_cpu.py proves on the CPU that the float64 restatement is
right at these shapes and parameters, and that each mistake these cases are
meant to catch moves the result by >= 10 x the bars used here.

Bars: those of test_gpu_parity.test_learner_vs_oracle, unchanged: first-step
gradient within 3e-4 max|g| of the restatement run with the device's ReLU masks
(flips only where the pre-activation is within 1e-4 of its layer's scale of 0),
loss rtol 1e-4 / atol 1e-5 at step 1 and rtol 1e-3 / atol 1e-4 later,
parameters and running statistics through check_learner_params(tol=1e-4).
"""
import numpy as np
import pytest

import bf16_ref as R
from learner_checks import check_grads_same_masks, check_momentum_blend_is_tested, start_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def _params(spai, blocks, start):
    return start_params(spai.init_params(blocks, 64, seed=blocks + 7), R.c4_layout(blocks), start, 60 + blocks)


def _batches(spai, e, sizes, seed):
    """one batch per entry of `sizes`: encodings of distinct positions reached by random
    legal play on the device, random normalised pi, z in {-1, 0, 1}"""
    from test_gpu_parity import _reachable_positions
    total = sum(sizes)
    states = _reachable_positions(spai, 2 * total + 8, 10, seed=seed)
    assert len(states) >= total
    e.games_resize(len(states))
    e.games_write(states)
    x_all = e.encode(len(states)).reshape(len(states), 126)
    rng = np.random.default_rng(seed)
    out, first = [], 0
    for B in sizes:
        pi = rng.random((B, 7)).astype(np.float32) ** 2
        out.append((x_all[first:first + B], (pi / pi.sum(1, keepdims=True)).astype(np.float32),
                    rng.choice(np.array([-1, 0, 1], np.float32), B)))
        first += B
    return out


CASES = [(1, 1, 1, "init"), (1, 3, 2, "init"), (1, 129, 1, "init"), (1, 147, 1, "init"), (1, 172, 1, "init"),
         (2, 300, 1, "init"),
         (0, 5, 1, "trained"), (2, 48, 2, "trained"), (1, 172, 1, "trained"), (2, 128, 1, "trained")]


@pytest.mark.parametrize("blocks,B,steps,start", CASES)
def test_learner_batch_edges_and_trained_params(spai, blocks, B, steps, start):
    """every case as test_learner_vs_oracle: first-step gradients under the device's
    masks, every step's loss, parameters and running statistics"""
    import learner_ref as LR
    from test_oracle_golden import check_learner_params
    e = spai.Engine(num_searches=1, max_trees=1)
    batches = _batches(spai, e, [B] * steps, seed=1000 * blocks + B)
    p0 = _params(spai, blocks, start)
    L = spai.Learner(e, blocks, p0)
    dev_losses = [L.train_batch(*batches[0])]
    assert L.last_batch == B
    report = {}
    check_grads_same_masks(L, L.grads(), p0, batches[0], blocks, report)   # reads the first step's activations
    dev_losses += [L.train_batch(*b) for b in batches[1:]]
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks, 64)
    print("case (%d, %d, %d, %s): gradient %.3g of max|g| (bar 3e-4), %d mask flips, loss %s vs %s" % (
        blocks, B, steps, start, report["err"], report["flips"], np.array(dev_losses)[:, 0], ref_losses[:, 0]))
    np.testing.assert_allclose(dev_losses[0], ref_losses[0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=1e-3, atol=1e-4)
    check_learner_params(L.params(), P_ref, ref_grads, blocks, 64, steps, tol=1e-4)
    if start == "trained":
        convs, _, _ = LR._layout(blocks, 64)
        P1_ref = P_ref if steps == 1 else LR.train(p0, batches[:1], blocks, 64)[0]
        print("running mean vs 0.1 * batch mean / vs old: %.3g / %.3g x the tolerance" % tuple(
            check_momentum_blend_is_tested(p0, P1_ref, convs)))
    L.close()
    e.close()


def test_learner_deterministic_past_the_registers(spai):
    """two learners, the same trained-like parameters, the same two batches of 172
    (re-read loops in both BatchNorm kernels, two reduce trips): the kernels promise
    fixed-order sums, so losses, gradients and parameters are bit-identical"""
    blocks, B = 1, 172
    e = spai.Engine(num_searches=1, max_trees=1)
    batches = _batches(spai, e, [B, B], seed=172)
    p0 = _params(spai, blocks, "trained")
    out = []
    for _ in range(2):
        L = spai.Learner(e, blocks, p0)
        rec = []
        for b in batches:
            rec += [L.train_batch(*b), L.grads(), L.params()]
        out.append(rec)
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][1]).max() > 0 and not np.array_equal(out[0][2], p0)
    e.close()


def test_learner_across_batch_sizes(spai):
    """one learner, batches of 3 -> 172 -> 3 -> 129 from trained-like parameters: the
    buffers grown for 172 serve the smaller third step, whose rows, chunk partials
    and statistics must not pick up anything stale.  The third step's gradient is
    checked on its own (from the device's parameters before it, under its masks),
    every loss and the final parameters against the restatement with Adam carried."""
    import learner_ref as LR
    from test_oracle_golden import check_learner_params
    blocks, sizes = 1, [3, 172, 3, 129]
    e = spai.Engine(num_searches=1, max_trees=1)
    batches = _batches(spai, e, sizes, seed=31)
    p0 = _params(spai, blocks, "trained")
    L = spai.Learner(e, blocks, p0)
    dev_losses = []
    for k, b in enumerate(batches):
        before = L.params()
        dev_losses.append(L.train_batch(*b))
        assert L.last_batch == sizes[k]
        if k == 2:
            check_grads_same_masks(L, L.grads(), before, b, blocks)
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks, 64)
    print("loss", np.array(dev_losses)[:, 0], ref_losses[:, 0])
    np.testing.assert_allclose(dev_losses[2], ref_losses[2], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=1e-3, atol=1e-4)
    check_learner_params(L.params(), P_ref, ref_grads, blocks, 64, len(sizes), tol=1e-4)
    L.close()
    e.close()
