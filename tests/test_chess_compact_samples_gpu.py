"""Compact chess self-play samples on the MI355X: self-play hands them over
(spai_chess_selfplay_compact), the learner expands them on its device
(k_samples_expand behind spai_chess_learner_train_batch_compact / _train_compact) and
spai_chess.learn(samples="compact") runs on them.

Everything here is an equality of bits, so there are no tolerances.  The dense route
(the existing self-play sink, train_batch, train and learn on dense arrays) is the
reference for the compact one; the dense form itself, spai_chess_samples_expand, is
pinned to the CPU oracle in tests/test_chess_compact_samples_cpu.py.  Sample sets
come from tests/chess_compact_ref.py: 26 positions (both colours, repeated roots,
promotions, en passant, 218 legal moves, one legal move) with random visit counts."""
import filecmp
import os

import numpy as np
import pytest

from chess_compact_ref import make_samples, positions, take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


@pytest.fixture(scope="module")
def pool(sc):
    """78 samples: the 26 positions three times over, every copy with visit counts of its own"""
    cs, _, _ = make_samples(sc, positions() * 3, seed=11)
    return cs


def _engine(sc):
    return sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_batch(L, cs):
    got, want = L.batch(), cs.expand()
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w))   # bit for bit: the zeros are +0.0


@pytest.mark.parametrize("window", [None, 2])
def test_self_play_compact_is_the_dense_run(sc, window):
    """hash evaluator, 6 games, 16 simulations, lockstep and through 2 tree slots: the compact
    run expanded on the host is the dense run, game by game in emission order, and so are the stats"""
    runs = []
    for mode in ("dense", "compact"):
        eng = sc.ChessEngine(num_searches=16, max_trees=6, eval_kind=sc.EVAL_HASH, seed=3)
        runs.append(eng.self_play(6, game_id_base=40, window=window, samples=mode))
        eng.close()
    (dense, dstats), (compact, cstats) = runs
    assert [g["game"] for g in dense] == [g["game"] for g in compact] and len(dense) == 6
    for d, c in zip(dense, compact):
        q = c["samples"]
        assert isinstance(q, sc.ChessSamples) and c["n"] == d["n"] == len(q)
        enc, pol, val = q.expand()
        assert np.array_equal(_bits(enc), _bits(d["enc"])) and np.array_equal(_bits(pol), _bits(d["policy"]))
        assert np.array_equal(_bits(val), _bits(d["value"])) and np.array_equal(q.samples["move"], d["moves"])
        assert np.all(q.game == d["game"]) and q.samples["first"][0] == 0
    for k in dstats:
        if k != "seconds":
            assert dstats[k] == cstats[k], k
    assert sum(g["n"] for g in dense) == dstats["positions"] > 0


def test_expand_kernel_alone(sc, pool):
    """after train_batch(ChessSamples) the device batch is samples.expand(), bit for bit: the 26
    positions in one batch, then batches of 2 and 1, each smaller than the one before it"""
    eng = _engine(sc)
    L = sc.ChessLearner(eng, 0, sc.init_params(0, 1))
    with pytest.raises(sc.SpaiError) as ei:
        L.batch()
    assert ei.value.code == -1
    for idx in (range(26), (24, 25), (24,), (51,), range(26, 59)):
        cs = take(sc, pool, list(idx))
        assert np.isfinite(L.train_batch(cs)).all() and L.last_batch() == len(cs)
        _same_batch(L, cs)
    z = np.zeros(1, np.float32)
    assert sc.lib().spai_chess_learner_batch(L.h, None, None, z.ctypes.data, 32) == -1   # the last step had 33
    dense = take(sc, pool, [3, 4, 5]).expand()
    L.train_batch(*dense)                                        # the window shows a dense step's batch too
    assert all(np.array_equal(a, b) for a, b in zip(L.batch(), dense))
    L.close()
    eng.close()


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 9, 33])
def test_step_dense_vs_compact(sc, pool, B, compute):
    """two learners from the same trained-like parameters, one fed dense arrays and one the
    compact samples, two steps: losses, gradients and parameters are the same bits"""
    import bf16_ref as R
    from learner_checks import start_params
    blocks = 1
    p0 = start_params(sc.init_params(blocks, 8), R.chess_layout(blocks), "trained", 61)
    eng = _engine(sc)
    steps = [take(sc, pool, range(k * B, (k + 1) * B)) for k in range(2)]
    out = []
    for mode in ("dense", "compact"):
        L = sc.ChessLearner(eng, blocks, p0, compute=compute)
        rec = []
        for cs in steps:
            rec += [L.train_batch(*cs.expand()) if mode == "dense" else L.train_batch(cs), L.grads(), L.params()]
        out.append(rec)
        L.close()
    eng.close()
    for a, b in zip(*out):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.abs(out[0][1]).max() > 0 and not np.array_equal(out[0][2], p0)


def test_train_dense_vs_compact(sc, pool):
    """Model::train over 21 samples, batch 8, 2 epochs: repeat=1 against the dense arrays,
    repeat=3 against the dense arrays tiled three times"""
    blocks = 1
    p0 = sc.init_params(blocks, 5)
    cs = take(sc, pool, range(30, 51))
    enc, pol, val = cs.expand()
    eng = _engine(sc)
    for repeat in (1, 3):
        res = []
        for mode in ("dense", "compact"):
            L = sc.ChessLearner(eng, blocks, p0)
            if mode == "dense":
                loss = L.train(np.tile(enc, (repeat, 1)), np.tile(pol, (repeat, 1)), np.tile(val, repeat),
                               epochs=2, batch=8, seed=13)
            else:
                loss = L.train(cs.with_repeat(repeat), epochs=2, batch=8, seed=13)
            res.append((loss, L.params(), L.last_batch(), L.batch()))
            L.close()
        (dl, dp, db, dbatch), (cl, cp, cb, cbatch) = res
        assert np.array_equal(_bits(dl), _bits(cl)) and np.array_equal(_bits(dp), _bits(cp))
        assert db == cb == (21 * repeat - 1) % 8 + 1
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dbatch, cbatch))
        assert not np.array_equal(dp, p0)
    eng.close()


def test_learn_dense_vs_compact(sc, tmp_path):
    """spai_chess.learn, 2 iterations of 4 games at 8 simulations, cloned 3 times over: the
    checkpoint files of the two modes are the same bytes, and the compact loop trains on
    ChessSamples only"""
    kw = dict(num_learn_iters=2, num_self_play_iters=3, num_parallel_self_play_games=4, batch_size=32, num_epochs=1,
              num_searches=8, blocks=1, seed=4)
    seen = {"dense": [], "compact": []}
    recs = {}
    for mode in seen:
        recs[mode] = sc.learn(checkpoint_dir=str(tmp_path / mode), samples=mode,
                              on_train_set=lambda i, *a, m=mode: seen[m].append(a), **kw)
    for d, c in zip(recs["dense"], recs["compact"]):
        assert d["samples"] == c["samples"] and d["games"] == c["games"] == 4 and d["loss"] == c["loss"]
        assert os.path.basename(d["checkpoint"]) == os.path.basename(c["checkpoint"])
        assert filecmp.cmp(d["checkpoint"], c["checkpoint"], shallow=False)
    assert len(seen["compact"]) == 2
    for (ds, dp, dv, dg), (cs, cp, cv, cg) in zip(seen["dense"], seen["compact"]):
        assert isinstance(cs, sc.ChessSamples) and cp is None and cv is None and isinstance(ds, np.ndarray)
        assert cs.repeat == 3 and len(cs) == len(dv) == 3 * cs.n and np.array_equal(cg, dg)
        assert cs.nbytes * 20 < ds[:cs.n].nbytes + dp[:cs.n].nbytes
        enc, pol, val = cs.expand()
        assert np.array_equal(enc, ds) and np.array_equal(pol, dp) and np.array_equal(val, dv)


def test_rejected_batch_changes_nothing(sc, pool):
    """a batch that validation rejects leaves the parameters, the moments and the step count as
    they were: the next step ends where it ends on a learner that never saw the batch"""
    blocks = 1
    p0 = sc.init_params(blocks, 2)
    a, b = take(sc, pool, range(0, 5)), take(sc, pool, range(5, 12))
    bad = sc.ChessSamples(b.samples.copy(), b.child_moves.copy(), b.child_visits.copy())
    bad.child_moves[int(bad.samples["first"][6]) + 1] = bad.child_moves[int(bad.samples["first"][6])]
    eng = _engine(sc)
    out = []
    for spoil in (False, True):
        L = sc.ChessLearner(eng, blocks, p0)
        rec = [L.train_batch(a), L.params()]
        if spoil:
            for call in (lambda: L.train_batch(bad), lambda: L.train(bad.with_repeat(2), epochs=1, batch=4)):
                with pytest.raises(sc.SpaiError) as ei:
                    call()
                assert ei.value.code == -1 and "sample 6" in str(ei.value) and "child_moves" in str(ei.value)
                assert np.array_equal(L.params(), rec[1]) and L.last_batch() == 5
            _same_batch(L, a)
        rec += [L.train_batch(b), L.grads(), L.params()]
        out.append(rec)
        L.close()
    eng.close()
    for x, y in zip(*out):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(out[0][4], out[0][1])
