"""CPU checks of the TicTacToe learner: the float64 restatement of the train step
(tests/ttt_learner_ref.py) against the PyTorch CPU fp32 golden
(tests/golden/gen_ttt_learner_golden.py), and the host side of the new entry
points (symbols, NULL arguments, no device -> an error, never a CPU fallback)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

NEW_SYMBOLS = ["spai_ttt_learner_create", "spai_ttt_learner_destroy", "spai_ttt_learner_train_batch",
               "spai_ttt_learner_train", "spai_ttt_learner_params", "spai_ttt_learner_grads",
               "spai_ttt_learner_activation", "spai_ttt_learner_last_batch", "spai_ttt_net_set_params"]


@pytest.fixture(scope="module")
def st():
    import spai_ttt
    spai_ttt.lib()
    return spai_ttt


def test_ttt_learner_ref_vs_torch_golden(st):
    """numpy float64 restatement vs PyTorch CPU fp32, with test_learner_oracle_vs_torch_golden's bounds"""
    import ttt_learner_ref as LR
    z = np.load(os.path.join(GOLDEN, "learner_ttt_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    assert (hidden, B, K) == (64, 32, 3)
    p0 = st.init_params(blocks, seed)
    batches = [(z["states"][k], z["policies"][k], z["values"][k]) for k in range(K)]
    P3, losses, grads = LR.train(p0, batches, blocks)
    np.testing.assert_allclose(losses, z["loss"], rtol=1e-5, atol=1e-6)
    g_ref = z["grads1"]
    assert np.abs(grads[0] - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    P1, _, _ = LR.train(p0, batches[:1], blocks)
    LR.check_learner_params(P1, z["params1"], [g_ref], blocks, 1)
    params3 = np.load(os.path.join(GOLDEN, "learner_ttt_1x64_step3.npz"))["params3"]
    LR.check_learner_params(P3, params3, [g_ref], blocks, 3, tol=1e-4)


def test_ttt_learner_golden_inputs_are_positions():
    """the golden's states are TicTacToe encodings: three one-hot planes per cell"""
    z = np.load(os.path.join(GOLDEN, "learner_ttt_1x64.npz"))
    s = z["states"].reshape(-1, 3, 9)
    assert np.all((s == 0) | (s == 1)) and np.all(s.sum(1) == 1)
    np.testing.assert_allclose(z["policies"].sum(2), 1.0, atol=1e-6)
    assert set(np.unique(z["values"])) <= {-1.0, 0.0, 1.0}


def test_ttt_learner_symbols(st):
    import spai
    L = st.lib()
    for s in NEW_SYMBOLS:
        assert s in spai.SYMBOLS and hasattr(L, s), s
    for m in ("train_batch", "train", "params", "grads", "activation", "last_batch", "close"):
        assert callable(getattr(st.TTTLearner, m)), m
    assert callable(st.TTTNet.set_params) and callable(st.learn)


def test_ttt_learner_null_arguments(st):
    L = st.lib()
    p = np.zeros(st.num_params(1), np.float32)
    h = C.c_void_p()
    assert L.spai_ttt_learner_create(None, 1, p.ctypes.data_as(C.c_void_p), p.size, None, C.byref(h)) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_ttt_net_set_params(None, p.ctypes.data_as(C.c_void_p), p.size) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_ttt_learner_destroy(None) == 0
    n = C.c_uint32()
    assert L.spai_ttt_learner_last_batch(None, C.byref(n)) == -1


def test_ttt_learner_needs_a_device(st):
    """without a GPU there is no learner: creating the engine it runs on, and so the
    learner, fails with SPAI_ERR_DEVICE; nothing falls back to the CPU"""
    import spai
    if spai.device_count() > 0:   # as test_no_gpu_fails_loudly
        pytest.skip("a GPU is visible")
    with pytest.raises(st.SpaiError) as ei:
        eng = st.TTTEngine(num_searches=1, max_trees=1)
        st.TTTLearner(eng, 0, st.init_params(0, 0))
    assert ei.value.code == -4
