"""Exact-arithmetic probes of the fused bf16 forwards (net_c4.hip k_forward,
chess_net.hip k_chess_forward): nets in which nothing rounds -- folded weights in
{-1, 0, +1} (times a power of two), small dyadic biases, 0/1 inputs, running
variance 1 - 1e-5 so that the folded scale is gamma -- so the device must give the
reference's logits bit for bit whatever its summation order, at any depth.

tests/bf16_ref.py builds the nets and asserts their exactness (every pre-rounding
activation a bf16 number, every sum below 2^24 units of its terms' LSB) before
anything is compared; tests/test_bf16_ref_cpu.py proves on the CPU that every probe
reacts to the error it is there to catch (each tap at each cell, each channel's
bias, a cell swap).  Three families per game: shift probes (an identity trunk
around one conv that shifts by one tap, 9 taps x 7 layer positions, 6- and 20-block
depths included), dense ternary probes (one layer kind dense over every (co, ci,
tap)), fold probes (non-trivial dyadic conv bias, BN beta, mean and gamma on every
conv).  Connect4 probes also run through predict at batch sizes that select every
group size S = 1..8 (with partial last groups), chess probes at batch sizes that run
P = 1, P = 2 and the odd split.
"""
import numpy as np
import pytest

import bf16_ref as R

pytestmark = pytest.mark.gpu

# test_net_group_size_invariance's counts: S = 1..8 on 256 CUs, and two rounds of S = 5
C4_COUNTS = (1, 40, 300, 700, 1000, 1300, 1500, 1700, 1800, 2048, 2100)
# test_chess_net_work_split_invariance's: one position per workgroup; m = 3 (P = 2 passes plus
# a P = 1 pass); m = 4 (P = 2)
CHESS_COUNTS = (5, 600, 1000)


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


@pytest.fixture(scope="module")
def c4_in():
    x, states = R.c4_probe_inputs()
    return x, states, R.c4_legal(states)


@pytest.mark.parametrize("probe", R.C4_PROBES, ids=R.probe_id)
def test_c4_exact_probe(spai, c4_in, probe):
    x, states, legal = c4_in
    first = len(x) - len(states)   # the encodings of `states` are the last rows of x
    e = spai.Engine(num_searches=1, max_trees=1)
    for tap, params, blocks, layer in R.probe_nets("c4", *probe):
        rl, rv = R.c4_forward(params, blocks, x, exact=True)
        net = spai.Net(e, blocks, params)
        lg, v = net.forward(x)
        np.testing.assert_array_equal(lg, rl.astype(np.float32), err_msg="%s tap %s" % (probe, tap))
        np.testing.assert_allclose(v, rv, **R.ULP_TOL)
        pri = R.softmax_mask(rl[first:], legal)
        for n in C4_COUNTS:
            idx = np.arange(n) % len(states)
            p, pv = net.predict([states[i] for i in idx])
            assert np.abs(p - pri[idx]).max() <= 1e-6, (probe, tap, n, np.abs(p - pri[idx]).max())
            assert np.all(p[~legal[idx]] == 0.0), (probe, tap, n)
            np.testing.assert_allclose(pv, rv[first:][idx], **R.ULP_TOL)
        net.close()
    e.close()


@pytest.mark.parametrize("probe", R.CHESS_PROBES, ids=R.probe_id)
def test_chess_exact_probe(sc, probe):
    x = R.chess_probe_inputs()
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    for tap, params, blocks, layer in R.probe_nets("chess", *probe):
        rl, rv = R.chess_forward(params, blocks, x, exact=True)
        rl = rl.astype(np.float32)
        net = sc.ChessNet(eng, blocks, params)
        for n in CHESS_COUNTS:
            idx = np.arange(n) % len(x)
            lg, v = net.forward(x[idx])
            assert np.array_equal(lg, rl[idx]), (probe, tap, n, np.abs(lg - rl[idx]).max())
            np.testing.assert_allclose(v, rv[idx], **R.ULP_TOL)
        net.close()
    eng.close()
