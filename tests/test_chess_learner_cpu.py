"""CPU checks of the chess learner's yardstick: the float64 restatement of the train
step (tests/chess_learner_ref.py) against PyTorch float64 autograd, live, from
init_params and from bf16_ref.trained_like parameters, with the bars of
tests/test_learner_ref_cpu.py (1e-10: both sides are float64); its eval-mode
forward against oracle/chessref.py::net_forward; that the checks of
tests/test_chess_learner_gpu.py react to planted faults; and the host side of the
new entry points (symbols, NULL arguments, no device -> an error, never a CPU
fallback)."""
import ctypes as C

import numpy as np
import pytest

import bf16_ref as R
import chess_learner_ref as LR
from learner_checks import start_params

NEW_SYMBOLS = ["spai_chess_learner_create", "spai_chess_learner_destroy", "spai_chess_learner_train_batch",
               "spai_chess_learner_train", "spai_chess_learner_params", "spai_chess_learner_grads",
               "spai_chess_learner_activation", "spai_chess_learner_last_batch", "spai_chess_net_set_params"]
GPU_GRAD_BAR = 3e-4    # learner_checks.check_grads_same_masks


@pytest.fixture(scope="module")
def sc(oracle):
    import spai_chess
    spai_chess.lib()
    return spai_chess


def _params(sc, blocks, start):
    return start_params(sc.init_params(blocks, blocks + 7), R.chess_layout(blocks), start, 60 + blocks)


@pytest.fixture(scope="module")
def batch3(oracle):
    """three positions of random legal play, shared by the cases below"""
    _, _, (batch,) = LR.make_batches(3, 1, 3)
    return batch


def test_layout_is_chessref_order(sc):
    import chessref
    for blocks in (0, 1, 2):
        convs, hd, n = LR._layout(blocks)
        assert n == sc.num_params(blocks) == R.layout_size(R.chess_layout(blocks))
        off, names = 0, iter(["p1w", "p1b", "p2w", "p2b", "vw", "vb", "l1w", "l1b", "l2w", "l2b"])
        ci = iter(convs)
        c = None
        for kind, shp in chessref.net_param_shapes(blocks):
            size = 4 * shp if kind == "bn" else int(np.prod(shp))
            if kind == "conv" and len(shp) == 4 and shp[2] == 3:
                c = next(ci)
                assert c["w"] == off
            elif kind == "bn":
                assert (c["g"], c["be"], c["mu"], c["var"]) == tuple(off + k * shp for k in range(4))
            elif c is not None and kind == "bias" and c["b"] == off:
                pass
            else:
                c = None
                assert hd[next(names)] == off, (kind, shp)
            off += size
        assert off == n


def test_batches_are_positions(batch3):
    """encodings of played positions: binary piece planes, non-binary counter planes
    somewhere; pi normalised over the legal moves; z in {-1, 0, 1}"""
    x, pi, z = batch3
    planes = x.reshape(-1, 19, 64)
    assert np.all((planes[:, :12] == 0) | (planes[:, :12] == 1))
    assert np.any((planes[:, 16:] != 0) & (planes[:, 16:] != 1))
    np.testing.assert_allclose(pi.sum(1), 1.0, atol=1e-6)
    assert np.all((pi > 0).sum(1) >= 1) and np.all((pi > 0).sum(1) <= 218)
    assert set(np.unique(z)) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("start", ["init", "trained"])
@pytest.mark.parametrize("blocks", [0, 1])
def test_restatement_vs_torch_float64(sc, batch3, blocks, start):
    """chess_learner_ref.forward_backward against PyTorch float64 autograd at B = 3:
    gradients within 1e-10 of max|g|, losses and updated running statistics within
    1e-10 (agreement is ~1e-15, so the bar fails on any real disagreement); then one
    Adam step against torch.optim.Adam"""
    p = _params(sc, blocks, start)
    P, G, loss = LR.forward_backward(p, *batch3, blocks)
    (lt, Gt, Pt), = LR.torch_train(p, [batch3], blocks)
    convs, _, n = LR._layout(blocks)
    running = np.zeros(n, bool)
    for c in convs:
        running[c["mu"]:c["mu"] + 2 * c["co"]] = True
    eg = np.abs(G - Gt).max() / np.abs(G).max()
    el = np.abs(loss - lt).max()
    er = np.abs(P[running] - Pt[running]).max()
    print("chess %d x 3 %s: gradient %.2g of max|g|, loss %.2g, running statistics %.2g (bars 1e-10)"
          % (blocks, start, eg, el, er))
    assert eg <= 1e-10 and el <= 1e-10 and er <= 1e-10
    assert np.array_equal(P[~running], np.asarray(p, np.float64)[~running])   # the forward moves no trainable parameter
    assert np.abs(G).max() > 0 and np.all(G[running] == 0)
    # Adam divides by |g| + 1e-8: only where |g| is well above that (learner_masks) do two
    # float64 gradients 1e-15 apart give the same step; elsewhere the step bound 2 lr holds
    P1 = LR.train(p, [batch3], blocks)[0]
    well, _ = LR.learner_masks(blocks, [G])
    assert np.abs(P1 - Pt)[well].max() <= 1e-10 and np.abs(P1 - Pt).max() <= 2e-3


@pytest.mark.parametrize("blocks", [0, 1])
def test_eval_forward_is_chessref(sc, batch3, blocks):
    """the restatement's eval-mode forward (running statistics) equals chessref.net_forward"""
    import chessref
    p = _params(sc, blocks, "trained")
    lg, v = LR.eval_forward(p, blocks, batch3[0])
    rl, rv = chessref.net_forward(p, blocks, batch3[0].reshape(-1, 19, 8, 8))
    assert np.abs(lg - rl).max() <= 1e-10 * max(1.0, np.abs(rl).max()) and np.abs(v - rv).max() <= 1e-12


def _drop_tap(x):
    cols = LR._im2col(x).copy()
    cols.reshape(len(cols), -1, 9)[:, :, 8] = 0.0    # the last tap never gathered
    return cols


FAULTS = {
    "dropped tap": ("_conv_cols", _drop_tap, "grad"),
    "lost head bias": ("_head_bias", lambda b: np.zeros_like(b), "grad"),
    "running mean loses (1-m)*old": ("_bn_running_mean", lambda old, mu, m: m * mu, "running"),
    "running mean not updated": ("_bn_running_mean", lambda old, mu, m: old, "running"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_show(sc, batch3, monkeypatch, fault):
    """a restatement with a device kernel's possible fault planted moves the gradient
    by >= 10 x the GPU bar (3e-3 of max|g|), or the running mean by >= 10 x
    check_learner_params' step-1 tolerance (1e-5 + 1e-4 |r|), from trained-like
    parameters at 1 block, B = 3; and check_learner_params rejects its parameters"""
    blocks = 1
    p = _params(sc, blocks, "trained")
    P, G, _ = LR.forward_backward(p, *batch3, blocks)
    P1 = LR.adam(P, G, 0.0, 0.0, 0)[0]
    hook, wrong, what = FAULTS[fault]
    monkeypatch.setattr(LR, hook, wrong)
    Pw, Gw, _ = LR.forward_backward(p, *batch3, blocks)
    Pw1 = LR.adam(Pw, Gw, 0.0, 0.0, 0)[0]
    convs, _, n = LR._layout(blocks)
    means = np.zeros(n, bool)
    for c in convs:
        means[c["mu"]:c["mu"] + c["co"]] = True
    if what == "grad":
        moved = np.abs(Gw - G).max() / np.abs(G).max() / GPU_GRAD_BAR
    else:
        moved = (np.abs(Pw[means] - P[means]) / (1e-5 + 1e-4 * np.abs(P[means]))).max()
    print("%-32s %9.3g x the bar" % (fault, moved))
    assert moved >= 10.0
    with pytest.raises(AssertionError):
        LR.check_learner_params(Pw1, P1, [G], blocks, 1, tol=1e-4)
    LR.check_learner_params(P1, P1, [G], blocks, 1, tol=1e-4)


def test_chess_learner_symbols(sc):
    import spai
    L = sc.lib()
    for s in NEW_SYMBOLS:
        assert s in spai.SYMBOLS and hasattr(L, s), s
    for m in ("train_batch", "train", "params", "grads", "activation", "last_batch", "close"):
        assert callable(getattr(sc.ChessLearner, m)), m
    assert callable(sc.ChessNet.set_params) and callable(sc.learn)


def test_chess_learner_null_arguments(sc):
    L = sc.lib()
    p = np.zeros(sc.num_params(0), np.float32)
    h = C.c_void_p()
    assert L.spai_chess_learner_create(None, 0, p.ctypes.data_as(C.c_void_p), p.size, None, C.byref(h)) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_chess_net_set_params(None, p.ctypes.data_as(C.c_void_p), p.size) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_chess_learner_destroy(None) == 0
    n = C.c_uint32()
    assert L.spai_chess_learner_last_batch(None, C.byref(n)) == -1


def test_chess_learner_needs_a_device(sc):
    """without a GPU there is no learner: creating the engine it runs on, and so the
    learner, fails with SPAI_ERR_DEVICE; nothing falls back to the CPU"""
    import spai
    if spai.device_count() > 0:   # as test_ttt_learner_needs_a_device
        pytest.skip("a GPU is visible")
    with pytest.raises(sc.SpaiError) as ei:
        eng = sc.ChessEngine(num_searches=1, max_trees=1)
        sc.ChessLearner(eng, 0, sc.init_params(0, 0))
    assert ei.value.code == -4
