"""CPU checks of the bf16 chess learner's yardstick (tests/chess_learner_bf16_ref.py):

  * with round = identity the restatement is chess_learner_ref.forward_backward
    (to 1e-10: both float64), which is pinned to PyTorch float64 autograd;
  * the layer-local checker of tests/test_chess_learner_bf16_gpu.py, fed a stand-in
    device (the quantised step with fp32 sums in three orders, fp32 tensors), stays
    under a third of every bar; and every planted fault of a device exceeds three
    times the bar it should trip.  So the bars sit well over the fp32-order noise and
    well under the subtlest fault, on the GPU tests' own inputs;
  * the host side of the new entry points (symbols, NULL arguments, error codes).

Measured here, error / bar of the check each fault trips hardest, at (init 1, 3),
(init 2, 5), (trained 1, 9); three fp32 orders without a fault reach 0.003 .. 0.006:

    truncation instead of rounding         75 .. 165   (logits, running statistics, a)
    residual read from the bf16 copy       15 .. 26    (a of the block's second conv)
    weight gradient fed truncated dz       22 .. 32    (conv weight gradients)
    dropped corner tap                     4000 .. 5100
    stale weight shadow at step 2          1400
    BatchNorm backward fed rounded z       15 .. 31    (the conv biases' zero gradient)

The last one is the subtlest at the fp32 tests' bars: rounding z moves xhat by 2^-9
of |z| / sigma, which reaches dz only through the xhat * dgamma / n term and dgamma
through a sum whose errors largely cancel, so it moves dz by 0.6 .. 1.0 and dgamma
by 1.7 .. 3.0 times their bars of 3e-4.  What it does break is an identity: the
gradient of a conv bias that feeds a BatchNorm is sum dz = 0, which holds only
while sum xhat = 0, and a rounded z leaves it 6000 x further from 0 than fp32
arithmetic does.  check_local therefore also holds those gradients to the fp32
rounding bound of chess_learner_bf16_ref.zero_bias_bound (derived from the number
format, in its docstring); that is the bar this fault trips."""
import ctypes as C

import numpy as np
import pytest

import bf16_ref as R
import chess_learner_bf16_ref as Q
import chess_learner_ref as LR
from learner_checks import start_params

NEW_SYMBOLS = ["spai_chess_learner_set_compute", "spai_chess_learner_get_compute", "spai_chess_learner_set_capture",
               "spai_chess_learner_gradient", "spai_chess_learner_logits"]


@pytest.fixture(scope="module")
def sc(oracle):
    import spai_chess
    spai_chess.lib()
    return spai_chess


def _params(sc, blocks, start):
    return start_params(sc.init_params(blocks, blocks + 7), R.chess_layout(blocks), start, 60 + blocks)


_BATCHES = {}


def _batches(blocks, B, steps=1, seed_base=1000):
    """the batches of tests/test_chess_learner_bf16_gpu.py (seed_base 1000: init, 2000: trained)"""
    key = (B, steps, seed_base * blocks + B)
    if key not in _BATCHES:
        _BATCHES[key] = LR.make_batches(*key)[2]
    return _BATCHES[key]


def test_rounding():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 2.0 ** 127, 0.0],
                 np.float32)
    # ties go to the even mantissa; bf16 keeps fp32's exponent
    assert np.array_equal(Q.bf16_round(x), np.array([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.0,
                                                     2.0 ** 127, 0.0]))
    assert np.array_equal(Q.bf16_trunc(x)[:4], [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7])
    r = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    q = Q.bf16_round(r)
    assert np.abs(q - r).max() <= 2.0 ** -9 * np.abs(r).max() and np.array_equal(Q.bf16_round(q), q)
    assert np.all(Q._bits(q) & 0xFFFF == 0)


@pytest.mark.parametrize("start", ["init", "trained"])
@pytest.mark.parametrize("blocks", [0, 1])
def test_identity_is_the_fp32_restatement(sc, blocks, start):
    """inherits the PyTorch-float64 pin of tests/test_chess_learner_cpu.py"""
    p0 = _params(sc, blocks, start)
    (batch,) = _batches(1, 3)
    P, G, loss = LR.forward_backward(p0, *batch, blocks)
    rec = Q.step(p0, *batch, blocks, round=Q.identity)
    for got, ref in ((rec["P"], P), (rec["G"], G), (rec["loss"], loss)):
        assert np.abs(got - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
    assert not Q.failures(Q.check_local(p0, *batch, blocks, Q.device_record(rec), round=Q.identity), 1e-6)


SHAPES = [("init", 1, 3), ("init", 2, 5), ("trained", 1, 9)]


@pytest.mark.parametrize("start,blocks,B", SHAPES)
def test_fp32_orders_stay_under_a_third_of_the_bars(sc, start, blocks, B):
    p0 = _params(sc, blocks, start)
    (batch,) = _batches(blocks, B, seed_base=1000 if start == "init" else 2000)
    worst = 0.0
    for mm in Q.F32_ORDERS:
        rec = Q.step(p0, *batch, blocks, round=Q.bf16_round, mm=mm, store=Q.to_f32)
        checks = Q.check_local(p0, *batch, blocks, Q.device_record(rec))
        assert not Q.failures(checks, 1.0 / 3), Q.failures(checks, 1.0 / 3)
        worst = max(worst, max(e / b for e, b in checks.values()))
    print("worst error / bar over three fp32 orders: %.3g" % worst)


def _tripped(checks, names):
    """the largest error / bar among the checks whose name starts with one of `names`"""
    return max(e / b for k, (e, b) in checks.items() if k.startswith(names))


FAULTS = {   # fault -> (step() arguments, the checks it should trip)
    "truncation": (dict(round=Q.bf16_trunc), ("g_w", "dz", "logits")),
    "residual_bf16": (dict(fault="residual_bf16"), ("a2", "a4")),
    "bn_bwd_rounded_z": (dict(fault="bn_bwd_rounded_z"), ("dz", "g_g", "zero_bias")),
    "wgrad_truncated_dz": (dict(wgrad_round=Q.bf16_trunc), ("g_w", "g_p1w", "g_p2w")),
    "corner_tap": (dict(fault="corner_tap"), ("a0", "a1")),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("start,blocks,B", SHAPES)
def test_planted_faults_trip_their_bars(sc, start, blocks, B, fault):
    p0 = _params(sc, blocks, start)
    (batch,) = _batches(blocks, B, seed_base=1000 if start == "init" else 2000)
    kw, names = FAULTS[fault]
    kw = dict(dict(round=Q.bf16_round), **kw)
    rec = Q.step(p0, *batch, blocks, mm=Q.F32_ORDERS[0], store=Q.to_f32, **kw)
    checks = Q.check_local(p0, *batch, blocks, Q.device_record(rec))
    t = _tripped(checks, names)
    print("%s: %.3g x its bar" % (fault, t))
    assert t > 3.0, (fault, t)


def test_stale_weight_shadow_trips_at_step_2(sc):
    """a step whose GEMMs read the weights of the step before"""
    blocks, B = 1, 3
    p0 = _params(sc, blocks, "init")
    batches = _batches(blocks, B, steps=2, seed_base=3000)
    kw = dict(round=Q.bf16_round, mm=Q.F32_ORDERS[0], store=Q.to_f32)
    _, good = Q.train(p0, batches, blocks, **kw)
    _, bad = Q.train(p0, batches, blocks, stale_at=1, **kw)
    assert not Q.failures(Q.check_local(good[1]["P0"], *batches[1], blocks, Q.device_record(good[1])), 1.0 / 3)
    checks = Q.check_local(bad[1]["P0"], *batches[1], blocks, Q.device_record(bad[1]))
    t = _tripped(checks, ("a", "logits", "g_w"))
    print("stale shadow: %.3g x its bar" % t)
    assert t > 3.0, t


def test_symbols(sc):
    import spai
    L = sc.lib()
    for s in NEW_SYMBOLS:
        assert s in spai.SYMBOLS and hasattr(L, s), s
    for m in ("set_compute", "compute", "set_capture", "gradient", "logits"):
        assert callable(getattr(sc.ChessLearner, m)), m
    assert spai.SYMBOLS.count("spai_chess_learner_gradient") == 1
    assert sc.ChessLearner.COMPUTE == {"f32": 1, "bf16": 0}   # spai_dtype


def test_null_arguments(sc):
    L = sc.lib()
    d, buf = C.c_int32(), np.zeros(4, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.spai_chess_learner_set_compute(None, 0), L.spai_chess_learner_get_compute(None, C.byref(d)),
               L.spai_chess_learner_set_capture(None, 1), L.spai_chess_learner_gradient(None, 0, p, 4),
               L.spai_chess_learner_logits(None, p, 4)):
        assert rc == -1
        assert b"NULL" in L.spai_last_error()


def test_learn_rejects_an_unknown_compute_type(sc):
    with pytest.raises(ValueError):
        sc.learn(num_learn_iters=1, compute="fp8")
