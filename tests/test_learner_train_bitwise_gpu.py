"""Model::train on the device, to the bit, for all three learners.

The epoch loop (a fresh Adam, one choose_multiple permutation, epochs x ceil(n /
batch) gathered minibatches) is one function shared by the Connect4, TicTacToe
and chess learners (csrc/learner_common.h, train_epochs).  The epoch tests of each
learner compare train() with a float64 restatement within a tolerance; this one
compares device with device: train() must leave exactly what train_batch leaves
when it is fed the same minibatches in the same order from the same parameters.

Shapes (n, batch, epochs), the smallest at which the loop can go wrong:
  (5, 2, 2)  three steps per epoch, the last of one sample (the smallest BatchNorm
             population), and a second pass over the same permutation
  (5, 8, 1)  batch > n: the loop clamps its host buffers to n, one step of 5
Each at the default settings and at adam_ref.CONFIG_B, where every field of
spai_adam_config is off its default (the default cases keep their test ids).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEED = 5, 11
SHAPES = [(N, 2, 2), (N, 8, 1)]


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def st():
    import spai_ttt
    return spai_ttt


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


_INPUTS = {}   # game -> (x, pi, z) of N samples, made once and never written


def _open(game, spai, st, sc, adam=None):
    """the game's engine, its N samples, blocks = 1 parameters, a learner constructor
    (adam: its spai_adam_config fields, default none) and how to read a learner's last
    batch size"""
    adam = adam or {}
    if game == "connect4":
        from test_learner_shapes_gpu import _batches
        eng = spai.Engine(num_searches=1, max_trees=1)
        make = lambda: _batches(spai, eng, [N], seed=SEED)[0]   # noqa: E731
        p0 = spai.init_params(1, 64, seed=SEED)
        new, last = (lambda: spai.Learner(eng, 1, p0, **adam)), (lambda L: L.last_batch)
    elif game == "tictactoe":
        from test_ttt_learner_gpu import _device_batches
        eng = st.TTTEngine(num_searches=1, max_trees=1)
        make = lambda: _device_batches(eng, N, 1, SEED)[0]   # noqa: E731
        p0 = st.init_params(1, SEED)
        new, last = (lambda: st.TTTLearner(eng, 1, p0, **adam)), (lambda L: L.last_batch())
    else:
        from test_chess_learner_gpu import _device_batches, _engine
        eng = _engine(sc)
        make = lambda: _device_batches(sc, eng, N, 1, SEED)[0]   # noqa: E731
        p0 = sc.init_params(1, SEED)
        new, last = (lambda: sc.ChessLearner(eng, 1, p0, **adam)), (lambda L: L.last_batch())
    if game not in _INPUTS:
        _INPUTS[game] = tuple(np.ascontiguousarray(a) for a in make())
        for a in _INPUTS[game]:
            a.setflags(write=False)
    return eng, _INPUTS[game], new, last


def _check_train_is_its_train_batches(spai, st, sc, game, n, batch, epochs, adam):
    eng, (x, pi, z), new, last = _open(game, spai, st, sc, adam)
    assert len(z) == n
    A = new()
    loss_a = A.train(x, pi, z, epochs=epochs, batch=batch, seed=SEED)
    B = new()
    perm = spai.choose_multiple(n, n, seed=SEED, stream=0x7EA1B).astype(np.int64)
    assert sorted(perm) == list(range(n))
    steps = [perm[i:i + batch] for i in range(0, n, batch)] * epochs
    for idx in steps:
        loss_b = B.train_batch(x[idx], pi[idx], z[idx])
    print("%s n %d batch %d epochs %d: %d steps, last of %d, loss %s" % (game, n, batch, epochs, len(steps),
                                                                        len(steps[-1]), loss_a))
    assert np.array_equal(A.params(), B.params())
    assert np.array_equal(A.grads(), B.grads())
    assert np.array_equal(np.asarray(loss_a), np.asarray(loss_b))
    assert np.all(np.isfinite(loss_a))
    assert last(A) == last(B) == len(steps[-1])
    A.close()
    B.close()
    eng.close()


@pytest.mark.parametrize("n,batch,epochs", SHAPES)
@pytest.mark.parametrize("game", ["connect4", "tictactoe", "chess"])
def test_train_is_its_train_batches(spai, st, sc, game, n, batch, epochs):
    _check_train_is_its_train_batches(spai, st, sc, game, n, batch, epochs, None)


@pytest.mark.parametrize("n,batch,epochs", SHAPES)
@pytest.mark.parametrize("game", ["connect4", "tictactoe", "chess"])
def test_train_is_its_train_batches_at_config_b(spai, st, sc, game, n, batch, epochs):
    from adam_ref import CONFIG_B
    _check_train_is_its_train_batches(spai, st, sc, game, n, batch, epochs, CONFIG_B)
