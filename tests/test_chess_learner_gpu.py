"""The chess learner on the MI355X (spai_chess_learner_*, spai_chess_net_set_params,
spai_chess.learn) against the numpy float64 restatement of the step
(tests/chess_learner_ref.py, pinned to PyTorch float64 autograd and to
chessref.net_forward in tests/test_chess_learner_cpu.py).

Inputs are encodings of positions reached by random legal play on the device
(the moves come from a seeded host generator through oracle/chessref.py, so the
CPU measurement below saw the same positions), pi random and normalised over each
position's legal moves, and z in {-1, 0, 1}.

Shapes (blocks, B, steps).  The kernels' sizes that B can straddle: a conv
workgroup owns ONE sample (so there is no partial-sample tile; B = 1, 2, 3 cover
one, two and an odd count of workgroups), and the weight gradient cuts the batch
into chunks of kWgSamples = 8 samples: B = 7 (a short single chunk), 8 (one full
chunk), 9 (the first B that needs a second chunk, which holds one sample).
B = 33 is five chunks, the last of one sample; (10, 2, 1) the reference's depth.
Channel chunks do not depend on B: every shape runs the 19-channel stem (a masked
second chunk of 16) and the 73-channel policy conv (a masked second tile of 64).

Bars are the Connect4 / TicTacToe learner tests': loss rtol 1e-4 at step 1 and
1e-3 later, gradient 3e-4 max|g| under the device's own ReLU masks (flips only
within 1e-4 of the layer's scale of zero), parameters check_learner_params with
1e-4 x steps, running statistics rtol 1e-4 + 1e-5 at step 1 (lr x steps later).
K = 2304 sums are longer than anything those learners see, so for every shape
the distance of PyTorch CPU fp32 from the float64 restatement was measured on the
CPU, on these inputs and seeds (chess_learner_ref.torch_fp32_distance; loss:
relative, worst step; gradient: / max|g| at step 1, the step whose gradient is
checked; well-conditioned parameters: absolute at the last step; running
statistics: absolute at the last step):

    start    (blocks, B, steps)  loss      gradient  parameters  running stats
    init     ( 0,   1, 1)         4.9e-08   3.1e-07   1.3e-08     5.6e-08
    init     ( 1,   1, 1)         1.6e-07   7.6e-07   1.3e-08     5.8e-08
    init     ( 1,   2, 2)         2.6e-05   1.0e-06   7.7e-04*    3.4e-04 (bound 2e-3)
    init     ( 1,   3, 1)         2.7e-08   1.2e-06   1.3e-08     5.7e-08
    init     ( 2,   5, 2)         1.3e-07   4.3e-07   4.5e-07     1.9e-04 (bound 2e-3)
    init     ( 1,  33, 1)         6.8e-08   5.0e-07   1.3e-08     5.4e-08
    init     (10,   2, 1)         3.7e-07   6.8e-06   1.3e-08     2.4e-07
    init     ( 1,   7, 1)         3.8e-08   6.1e-07   1.3e-08     5.4e-08
    init     ( 1,   8, 1)         1.0e-07   4.8e-07   1.3e-08     5.7e-08
    init     ( 1,   9, 1)         2.1e-08   3.0e-07   1.3e-08     5.5e-08
    trained  ( 1,   5, 2)         1.0e-07   5.0e-07   1.1e-07     1.9e-04 (bound 2e-3)
    trained  ( 2,   9, 1)         8.3e-08   7.0e-07   4.8e-08     1.6e-07

Where a figure is under a third of its bar (1e-4, 3e-4, 1e-4 x steps, 1e-5 at step
1 or lr x steps later) the bar stands: every figure but one.  At (1, 2, 2) PyTorch
fp32 itself ends 7.7e-4 from the restatement (BatchNorm over 128 values, second
step), above a third of 2e-4, so that shape's parameter bar is 3 x 7.7e-4 = 2.3e-3
(marked *; _bars below applies the rule to the table).  No bar comes from the
device's output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# measured on the CPU: (start, blocks, B, steps) -> loss, gradient, parameters, running statistics
MEASURED = {
    ("init", 0, 1, 1): (4.9e-08, 3.1e-07, 1.3e-08, 5.6e-08),
    ("init", 1, 1, 1): (1.6e-07, 7.6e-07, 1.3e-08, 5.8e-08),
    ("init", 1, 2, 2): (2.6e-05, 1.0e-06, 7.7e-04, 3.4e-04),
    ("init", 1, 3, 1): (2.7e-08, 1.2e-06, 1.3e-08, 5.7e-08),
    ("init", 2, 5, 2): (1.3e-07, 4.3e-07, 4.5e-07, 1.9e-04),
    ("init", 1, 33, 1): (6.8e-08, 5.0e-07, 1.3e-08, 5.4e-08),
    ("init", 10, 2, 1): (3.7e-07, 6.8e-06, 1.3e-08, 2.4e-07),
    ("init", 1, 7, 1): (3.8e-08, 6.1e-07, 1.3e-08, 5.4e-08),
    ("init", 1, 8, 1): (1.0e-07, 4.8e-07, 1.3e-08, 5.7e-08),
    ("init", 1, 9, 1): (2.1e-08, 3.0e-07, 1.3e-08, 5.5e-08),
    ("trained", 1, 5, 2): (1.0e-07, 5.0e-07, 1.1e-07, 1.9e-04),
    ("trained", 2, 9, 1): (8.3e-08, 7.0e-07, 4.8e-08, 1.6e-07),
}
PROJECT = dict(loss=1e-4, grad=3e-4, par=1e-4, run=1e-5)   # run: step 1; lr * steps later


def _bars(start, blocks, B, steps):
    """the project's bar, or 3 x the measured PyTorch fp32 distance where that is not under a third of it"""
    el, eg, ep, er = MEASURED[start, blocks, B, steps]
    run = PROJECT["run"] if steps == 1 else 1e-3 * steps
    pick = lambda m, bar: bar if m < bar / 3 else 3 * m   # noqa: E731
    return dict(loss=pick(el, PROJECT["loss"]), grad=pick(eg, PROJECT["grad"]), par=pick(ep, PROJECT["par"] * steps) / steps,
                run=pick(er, run))


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


def _engine(sc):
    return sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)


def _play_on_device(eng, games, order, want):
    """the positions after the move lists `games` (longest first), played with the
    device's rules from the start position; their encodings [n][1216] in `order`,
    equal to the restatement's"""
    n = len(games)
    eng.games_resize(n)
    for k in range(len(games[0])):
        moving = sum(1 for g in games if len(g) > k)   # a prefix: the list is longest first
        rc = eng.apply(np.array([g[k] for g in games[:moving]], np.uint16))
        assert not rc.any()
    assert np.all(eng.status(n)[0] == 0)
    x = eng.encode(n).reshape(n, 1216)[order]
    assert np.array_equal(x, want)
    return x


_BATCHES = {}


def _device_batches(sc, eng, B, steps, seed):
    import chess_learner_ref as LR
    if (B, steps, seed) not in _BATCHES:
        _BATCHES[B, steps, seed] = LR.make_batches(B, steps, seed)
    games, order, batches = _BATCHES[B, steps, seed]
    x = _play_on_device(eng, games, order, np.concatenate([b[0] for b in batches]))
    return [(x[k * B:(k + 1) * B], b[1], b[2]) for k, b in enumerate(batches)]


def _check_grads_same_masks(L, g, p0, batch, blocks, bar):
    """fp32 device gradient vs the float64 restatement run with the DEVICE's ReLU masks
    (activation > 0), the method of learner_checks.check_grads_same_masks: the masks
    may differ from the restatement's own (pre > 0) only where its pre-activation is
    within 1e-4 of its layer's scale of zero; every entry within bar * max|g|"""
    import chess_learner_ref as LR
    nl = 2 * blocks + 4
    masks = [L.activation(l) > 0 for l in range(nl)]
    diag = {}
    n = len(p0)
    _, _, _, _, ref = LR.train_step(p0, np.zeros(n), np.zeros(n), 0, *batch, blocks, masks=masks, diag=diag)
    flips = 0
    for l in range(nl):
        pre = diag["pre"][l]
        diff = masks[l].reshape(pre.shape) != (pre > 0)
        flips += int(diff.sum())
        assert np.all(np.abs(pre[diff]) <= 1e-4 * np.abs(pre).max()), (l, np.abs(pre[diff]).max())
    d, m = np.abs(g - ref), np.abs(ref).max()
    print("grad vs f64 (device masks) %.3g of max|g|, flips %d, bar %.3g" % (d.max() / m, flips, bar))
    assert d.max() <= bar * m, (d.max() / m, flips)
    return flips


def _vs_restatement(sc, start, blocks, B, steps, seed_base):
    import bf16_ref as R
    import chess_learner_ref as LR
    from learner_checks import check_momentum_blend_is_tested, start_params
    bars = _bars(start, blocks, B, steps)
    eng = _engine(sc)
    batches = _device_batches(sc, eng, B, steps, seed_base * blocks + B)
    p0 = start_params(sc.init_params(blocks, blocks + 7), R.chess_layout(blocks), start, 60 + blocks)
    L = sc.ChessLearner(eng, blocks, p0)
    dev_losses = [L.train_batch(*batches[0])]
    assert L.last_batch() == B
    _check_grads_same_masks(L, L.grads(), p0, batches[0], blocks, bars["grad"])   # reads the first step's activations
    dev_losses += [L.train_batch(*b) for b in batches[1:]]
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks)
    print("loss", np.array(dev_losses), ref_losses, "bars", bars)
    np.testing.assert_allclose(dev_losses[0], ref_losses[0], rtol=bars["loss"], atol=1e-5)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=max(1e-3, bars["loss"]), atol=1e-4)
    LR.check_learner_params(L.params(), P_ref, ref_grads, blocks, steps, tol=bars["par"], run_atol=bars["run"])
    if start == "trained":
        P1_ref = P_ref if steps == 1 else LR.train(p0, batches[:1], blocks)[0]
        print("running mean vs 0.1 * batch mean / vs old: %.3g / %.3g x the tolerance" % tuple(
            check_momentum_blend_is_tested(p0, P1_ref, LR._layout(blocks)[0])))
    L.close()
    eng.close()


@pytest.mark.parametrize("blocks,B,steps", [(0, 1, 1), (1, 1, 1), (1, 2, 2), (1, 3, 1), (2, 5, 2), (1, 33, 1),
                                            (10, 2, 1), (1, 7, 1), (1, 8, 1), (1, 9, 1)])
def test_chess_learner_vs_restatement(sc, blocks, B, steps):
    """the heads alone on one sample; one block, one sample; two workgroups, two steps;
    an odd count; two blocks over two steps; five weight-gradient chunks, the last of
    one sample; the reference's depth; then the chunk of 8 samples: 7 (short), 8
    (full), 9 (the first B with a second chunk)"""
    _vs_restatement(sc, "init", blocks, B, steps, 1000)


@pytest.mark.parametrize("blocks,B,steps", [(1, 5, 2), (2, 9, 1)])
def test_chess_learner_trained_like_vs_restatement(sc, blocks, B, steps):
    """the same check from bf16_ref.trained_like parameters: conv biases (the heads'
    too), beta and the running mean away from 0, the running variance away from 1,
    gammas above 1 and below 0, so the running-statistic blend, the head biases and
    every factor of the BN backward count"""
    _vs_restatement(sc, "trained", blocks, B, steps, 2000)


def test_chess_learner_deterministic(sc):
    """two learners, the same parameters, the same two batches of 17: bit-identical"""
    blocks = 2
    eng = _engine(sc)
    batches = _device_batches(sc, eng, 17, 2, 5)
    p0 = sc.init_params(blocks, 3)
    out = []
    for _ in range(2):
        L = sc.ChessLearner(eng, blocks, p0)
        rec = []
        for b in batches:
            rec += [L.train_batch(*b), L.grads(), L.params()]
        out.append(rec)
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][1]).max() > 0 and not np.array_equal(out[0][2], p0)
    assert not np.array_equal(out[0][5], out[0][2])
    eng.close()


def test_chess_learner_train_epochs(sc):
    """Model::train: a fresh Adam per call, one permutation of the samples, epochs x
    ceil(n/B) steps with a short last batch, vs the restatement fed the same permutation"""
    import chess_learner_ref as LR
    import spai
    blocks, n, B, epochs, seed = 1, 70, 32, 2, 9
    eng = _engine(sc)
    (x, pi, z), = _device_batches(sc, eng, n, 1, 70)
    p0 = sc.init_params(blocks, 5)
    L = sc.ChessLearner(eng, blocks, p0)
    L.train(x, pi, z, epochs=epochs, batch=B, seed=seed)
    assert L.last_batch() == 6
    loss = L.train(x, pi, z, epochs=1, batch=B, seed=seed + 1)   # second call: Adam starts over
    assert L.last_batch() == 6
    P = L.params()
    ref, all_grads = p0.astype(np.float64), []
    for s_, ep in ((seed, epochs), (seed + 1, 1)):
        perm = spai.choose_multiple(n, n, seed=s_, stream=0x7EA1B).astype(np.int64)
        batches = [(x[perm[i:i + B]], pi[perm[i:i + B]], z[perm[i:i + B]]) for i in range(0, n, B)] * ep
        ref, ref_losses, grads = LR.train(ref, batches, blocks)
        all_grads += grads
    np.testing.assert_allclose(loss, ref_losses[-1], rtol=1e-3, atol=1e-4)
    LR.check_learner_params(P, ref, all_grads, blocks, len(all_grads), tol=2e-4)
    L.close()
    eng.close()


def test_chess_net_set_params(sc):
    """after a train step, net.set_params(L.params()) == ChessNet(eng, blocks, L.params()), bit for bit"""
    blocks = 2
    eng = _engine(sc)
    (x, pi, z), = _device_batches(sc, eng, 17, 1, 64)
    p0 = sc.init_params(blocks, 1)
    net = sc.ChessNet(eng, blocks, p0)
    lg0, v0 = net.forward(x)
    L = sc.ChessLearner(eng, blocks, p0)
    L.train_batch(x, pi, z)
    P = L.params()
    net.set_params(P)
    lg1, v1 = net.forward(x)
    fresh = sc.ChessNet(eng, blocks, P)
    lg2, v2 = fresh.forward(x)
    assert np.array_equal(lg1, lg2) and np.array_equal(v1, v2)
    assert not np.array_equal(lg0, lg1) and not np.array_equal(v0, v1)
    with pytest.raises(sc.SpaiError) as ei:
        net.set_params(P[:-1])
    assert ei.value.code == -1
    L.close()
    fresh.close()
    net.close()
    eng.close()


def _self_play_samples(sc, params, blocks, game_ids, seed, sims):
    eng = sc.ChessEngine(num_searches=sims, max_trees=len(game_ids), seed=seed)
    eng.set_net(sc.ChessNet(eng, blocks, params))
    games, _ = eng.self_play(len(game_ids), game_id_base=int(game_ids[0]))
    eng.close()
    return sc._samples(games)


def test_chess_learn_end_to_end(sc, tmp_path):
    """Learner::learn: self-play -> train -> checkpoint, twice, on the device"""
    import spai
    blocks, seed, G, sims, iters = 1, 4, 4, 8, 2
    kw = dict(num_learn_iters=2, num_self_play_iters=iters, num_parallel_self_play_games=G, batch_size=32,
              num_epochs=1, num_searches=sims, blocks=blocks, seed=seed)
    p0 = sc.init_params(blocks, seed)
    sets = {}
    rec = sc.learn(checkpoint_dir=str(tmp_path / "a"), on_train_set=lambda i, *a: sets.__setitem__(i, a), **kw)
    assert [r["iteration"] for r in rec] == [0, 1] and all(np.isfinite(r["loss"]).all() for r in rec)
    ck = [spai.load_params(r["checkpoint"], blocks, hidden=256, game=spai.GAME_CHESS, n=len(p0)) for r in rec]
    assert all(np.isfinite(c).all() for c in ck)
    # checkpoint i is the learner's parameters after iteration i: a second learner fed the
    # same training sets (the step is deterministic) ends at the same bits
    eng = _engine(sc)
    L = sc.ChessLearner(eng, blocks, p0)
    for i in range(2):
        s, p, v, gid = sets[i]
        assert rec[i]["samples"] == len(v) and rec[i]["games"] == G
        L.train(s, p, v, epochs=1, batch=32, seed=sc._iter_seed(seed, i))
        assert np.array_equal(L.params(), ck[i])
    L.close()
    eng.close()
    assert not np.array_equal(ck[0], p0) and not np.array_equal(ck[1], ck[0])
    # clone_self_play: one batch of G games, tiled num_self_play_iters times
    s1, p1, v1, gid1 = sets[1]
    m = len(v1) // iters
    assert len(v1) == iters * m
    for a in (s1, p1, v1, gid1):
        assert np.array_equal(a, np.concatenate([a[:m]] * iters))
    ids0, ids1 = np.unique(sets[0][3]), np.unique(gid1)
    assert len(ids0) == G and len(ids1) == G and not set(ids0) & set(ids1)
    # the refresh reached self-play: iteration 1's samples are the games played from checkpoint 0
    want = _self_play_samples(sc, ck[0], blocks, ids1, seed, sims)
    assert all(np.array_equal(a[:m], b) for a, b in zip((s1, p1, v1), want))
    stale = _self_play_samples(sc, p0, blocks, ids1, seed, sims)
    assert len(stale[2]) != m or not np.array_equal(stale[1], p1[:m])
    # two runs: bit-identical checkpoints
    rec2 = sc.learn(checkpoint_dir=str(tmp_path / "b"), **kw)
    for r, c in zip(rec2, ck):
        assert np.array_equal(spai.load_params(r["checkpoint"], blocks, hidden=256, game=spai.GAME_CHESS, n=len(p0)), c)
