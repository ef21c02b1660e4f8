"""The four forwards on trained-like parameters: non-zero conv biases, BN beta and
running mean, running variance != 1, some negative gammas (bf16_ref.trained_like).
Every other net test runs on init parameters, where the folded bias
(b - mu) * scale + beta is identically zero.

fp32 nets: the Connect4 fp32 mode against the CPU oracle bit for bit (values to the
last ulp of tanhf), the TicTacToe net against its oracle and a PyTorch fixture at
the bars of test_ttt_gpu.py.  (tests/test_bf16_ref_cpu.py checks the oracles on
the same parameters against PyTorch and a float64 restatement.)

bf16 nets: against bf16_ref's emulation of the kernels' quantisation points with
fp64 accumulation.  The bound is computed from the reference: 4 x the largest
distance of three fp32-accumulated emulations with permuted K orders from the
fp64-accumulated one (the device is one more fp32 order; rounding flips are rare and
discrete, hence the factor).  test_bf16_ref_cpu.py asserts that this bound is at
most a third of what a dropped corner tap or a zeroed bias moves and below the old
3e-2 bar.  Each test prints its measured device distance / spread; the docstrings
record the figures of an MI355X run.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import bf16_ref as R
from test_bf16_ref_cpu import trained_c4_params, trained_chess_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "trained_like_nets.npz"))


# ---------------------------------------------------------------- fp32 nets
@pytest.mark.parametrize("blocks", [0, 2])
def test_c4_f32_trained_params_bit_exact_vs_oracle(spai, oracle, fixture, blocks):
    p = trained_c4_params(oracle, blocks)
    x = np.concatenate([fixture["c4_x"], R.c4_probe_inputs()[0][:8]]).reshape(-1, 126)
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, blocks, p, dtype=spai.DTYPE_F32)
    lg, v = net.forward(x)
    rl, rv = oracle.Net(oracle.GAME_CONNECT4, blocks, 64, p).forward(x)
    np.testing.assert_array_equal(lg, rl)
    np.testing.assert_allclose(v, rv, **R.ULP_TOL)
    net.close()
    e.close()


def test_ttt_trained_params_vs_oracle_and_torch(oracle, fixture):
    import gen_trained_like_golden as GT
    import spai_ttt as st
    blocks = GT.NETS["ttt"][0]
    p, x = GT.net_params("ttt"), fixture["ttt_x"]
    eng = st.TTTEngine()
    net = st.TTTNet(eng, blocks, p)
    lg, v = net.forward(x)
    ol, ov = oracle.Net(oracle.GAME_TICTACTOE, blocks, 64, p).forward(x.reshape(len(x), -1))
    for rl, rv, what in ((fixture["ttt_logits"], fixture["ttt_value"], "torch"), (ol, ov, "oracle")):
        dl, dv = np.abs(lg - rl).max(), np.abs(v - rv).max()
        print("ttt vs %s: |dlogit| %.3g, |dvalue| %.3g" % (what, dl, dv))
        assert dl <= 1e-4 * max(1.0, np.abs(rl).max()), what   # the bars of test_ttt_net_vs_torch_golden
        assert dv <= 1e-5, what
    net.close()
    eng.close()


# ---------------------------------------------------------------- bf16 nets
def _check(name, lg, v, ref):
    dl, dv = float(np.abs(lg - ref["logits"]).max()), float(np.abs(v - ref["value"]).max())
    print("%s: logits |d| %.3g, spread %.3g, ratio %.2f (bound 4); values |d| %.3g, spread %.3g" % (
        name, dl, ref["spread_l"], dl / ref["spread_l"], dv, ref["spread_v"]))
    assert dl <= ref["bound_l"], (name, dl, ref["bound_l"])
    assert dv <= ref["bound_v"], (name, dv, ref["bound_v"])


@pytest.mark.parametrize("blocks", [0, 1, 2])
def test_c4_bf16_trained_params_vs_emulation(spai, oracle, fixture, blocks):
    """device distance / spread of the logits, measured on an MI355X (the bound is 4):
    0 blocks 0.06 (2.3e-7 / 4.1e-6), 1 block 1.00 (4.2e-3 / 4.2e-3), 2 blocks 1.34
    (1.05e-2 / 7.9e-3)"""
    p, x = trained_c4_params(oracle, blocks), fixture["c4_x"]
    ref = R.spread_bound(R.c4_forward, p, blocks, x)
    R.check_bound_conditions(R.c4_forward, p, blocks, x, ref)
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, blocks, p)
    lg, v = net.forward(x)
    _check("c4 %d blocks" % blocks, lg, v, ref)
    net.close()
    e.close()


@pytest.mark.parametrize("blocks", [0, 1])
def test_chess_bf16_trained_params_vs_emulation(fixture, blocks):
    """device distance / spread of the logits, measured on an MI355X (the bound is 4):
    0 blocks 0.0004 (5.3e-7 / 1.2e-3), 1 block 1.17 (8.9e-3 / 7.7e-3)"""
    import spai_chess as sc
    p, x = trained_chess_params(blocks), fixture["chess_x"]
    ref = R.spread_bound(R.chess_forward, p, blocks, x, chunk=4)
    R.check_bound_conditions(R.chess_forward, p, blocks, x, ref)
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    net = sc.ChessNet(eng, blocks, p)
    lg, v = net.forward(x)
    _check("chess %d blocks" % blocks, lg, v, ref)
    net.close()
    eng.close()


# ---------------------------------------------------------------- the product path: learner -> self-play net
def test_c4_learner_params_into_bf16_net(spai, fixture):
    """three device train steps of the 1x64 net at B = 32, then the bf16 self-play net on
    the learner's parameters (moved running statistics, trained biases) by the same rule.
    Measured device distance / spread of the logits on an MI355X: 0.04 (8.0e-6 / 1.9e-4)"""
    z = np.load(os.path.join(GOLDEN, "learner_c4_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    assert (blocks, hidden, B, K) == (1, 64, 32, 3)
    e = spai.Engine(num_searches=1, max_trees=1)
    L = spai.Learner(e, blocks, spai.init_params(blocks, hidden, seed=seed), hidden=hidden)
    for k in range(K):
        L.train_batch(z["states"][k], z["policies"][k], z["values"][k])
    p = L.params()
    d = R.unflatten(p, R.c4_layout(blocks))
    assert np.abs(d["stem.mu"]).max() > 1e-3 and np.abs(d["res1.var"] - 1).max() > 1e-3   # the statistics moved
    x = fixture["c4_x"]
    ref = R.spread_bound(R.c4_forward, p, blocks, x)
    assert ref["bound_l"] < 3e-2 * max(1.0, np.abs(ref["logits"]).max())
    net = spai.Net(e, blocks, p)
    lg, v = net.forward(x)
    _check("c4 learner 1x64", lg, v, ref)
    net.close()
    L.close()
    e.close()


def test_ttt_learner_params_into_net(oracle, fixture):
    import spai_ttt as st
    z = np.load(os.path.join(GOLDEN, "learner_ttt_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    L = st.TTTLearner(eng, blocks, st.init_params(blocks, seed))
    for k in range(K):
        L.train_batch(z["states"][k], z["policies"][k], z["values"][k])
    p = L.params()
    x = fixture["ttt_x"]
    net = st.TTTNet(eng, blocks, p)
    lg, v = net.forward(x)
    rl, rv = oracle.Net(oracle.GAME_TICTACTOE, blocks, 64, p).forward(x.reshape(len(x), -1))
    assert np.abs(lg - rl).max() <= 1e-4 * max(1.0, np.abs(rl).max())
    assert np.abs(v - rv).max() <= 1e-5
    net.close()
    L.close()
    eng.close()
