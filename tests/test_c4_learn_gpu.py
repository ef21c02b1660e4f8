"""spai.learn: Learner::learn (learner.rs:98-196) for Connect4 on the device --
self-play, Model::train, checkpoint, with the self-play net refreshed in place
from the learner (Net.set_params).  Mirrors test_ttt_learn_end_to_end at a
1-block net, 32 games of 16 simulations, 3 self-play iterations, 2 learn
iterations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCKS, SEED, G, SIMS, ITERS = 1, 4, 32, 16, 3
KW = dict(num_learn_iters=2, num_self_play_iters=ITERS, num_parallel_self_play_games=G, batch_size=32,
          num_epochs=2, num_searches=SIMS, blocks=BLOCKS, seed=SEED)


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def _self_play_samples(spai, params, game_ids):
    import spai_learn
    eng = spai.Engine(num_searches=SIMS, max_trees=len(game_ids), seed=SEED)
    eng.set_net(spai.Net(eng, BLOCKS, params))
    games, _ = eng.self_play(len(game_ids), game_id_base=int(game_ids[0]))
    eng.close()
    return spai_learn._samples(games)


def _checkpoints(spai, rec, n):
    return [spai.load_params(r["checkpoint"], BLOCKS) for r in rec[:n]]


@pytest.fixture(scope="module")
def run(spai, tmp_path_factory):
    """the reference run: records, training sets, checkpoints"""
    sets = {}
    rec = spai.learn(checkpoint_dir=str(tmp_path_factory.mktemp("a")),
                     on_train_set=lambda i, *a: sets.__setitem__(i, a), **KW)
    return rec, sets, _checkpoints(spai, rec, 2)


def test_c4_learn_end_to_end(spai, run):
    """self-play -> train -> checkpoint, twice: records and checkpoints load, checkpoint i
    is a second learner's parameters after the captured training sets, Q8 tiling and
    disjoint game ids, and iteration 1 played from checkpoint 0 (the refresh reached
    the search, evaluation cache included)"""
    import spai_learn
    rec, sets, ck = run
    p0 = spai.init_params(BLOCKS, seed=SEED)
    assert [r["iteration"] for r in rec] == [0, 1] and all(np.isfinite(r["loss"]).all() for r in rec)
    e = spai.Engine(num_searches=1, max_trees=1)
    L = spai.Learner(e, BLOCKS, p0)
    for i in range(2):
        s, p, v, gid = sets[i]
        assert rec[i]["samples"] == len(v) and rec[i]["games"] == G
        L.train(s, p, v, epochs=2, batch=32, seed=spai_learn._iter_seed(SEED, i))
        assert np.array_equal(L.params(), ck[i])
    L.close()
    e.close()
    assert not np.array_equal(ck[0], p0) and not np.array_equal(ck[1], ck[0])
    # clone_self_play: one batch of G games, tiled num_self_play_iters times
    s1, p1, v1, gid1 = sets[1]
    m = len(v1) // ITERS
    assert len(v1) == ITERS * m
    for a in (s1, p1, v1, gid1):
        assert np.array_equal(a, np.concatenate([a[:m]] * ITERS))
    ids0, ids1 = np.unique(sets[0][3]), np.unique(gid1)
    assert len(ids0) == G and len(ids1) == G and not set(ids0) & set(ids1)
    # iteration 1's samples are the games played from checkpoint 0, not from the initial parameters
    want = _self_play_samples(spai, ck[0], ids1)
    assert all(np.array_equal(a[:m], b) for a, b in zip((s1, p1, v1), want))
    stale = _self_play_samples(spai, p0, ids1)
    assert len(stale[2]) != m or not np.array_equal(stale[1], p1[:m])


def test_c4_learn_is_deterministic(spai, run, tmp_path):
    rec2 = spai.learn(checkpoint_dir=str(tmp_path), **KW)
    for a, b in zip(_checkpoints(spai, rec2, 2), run[2]):
        assert np.array_equal(a, b)


def test_c4_learn_distinct_batches(spai, tmp_path):
    """clone_self_play=False: num_self_play_iters distinct batches, disjoint game ids"""
    sets = {}
    spai.learn(checkpoint_dir=str(tmp_path), clone_self_play=False,
               on_train_set=lambda i, *a: sets.__setitem__(i, a), **KW)
    all_ids = []
    for i in range(2):
        gid = sets[i][3]
        ids = np.unique(gid)
        assert len(ids) == ITERS * G and np.all(np.diff(gid) >= 0)
        all_ids += list(ids)
        parts = [sets[i][1][(gid >= ids[b * G]) & (gid <= ids[(b + 1) * G - 1])] for b in range(ITERS)]
        assert not any(len(parts[a]) == len(parts[b]) and np.array_equal(parts[a], parts[b])
                       for a in range(ITERS) for b in range(a))
    assert len(set(all_ids)) == 2 * ITERS * G


def test_c4_learn_refresh_routes_and_window(spai, run, tmp_path):
    """refresh="host" and a streamed window of 8 slots: the same checkpoints bit for bit
    (the two routes pack the same words; streamed games equal lockstep games per game)"""
    ck = run[2]
    host = spai.learn(checkpoint_dir=str(tmp_path / "h"), refresh="host", **KW)
    for a, b in zip(_checkpoints(spai, host, 2), ck):
        assert np.array_equal(a, b)
    win = spai.learn(checkpoint_dir=str(tmp_path / "w"), window=8, **KW)
    for a, b in zip(_checkpoints(spai, win, 2), ck):
        assert np.array_equal(a, b)
