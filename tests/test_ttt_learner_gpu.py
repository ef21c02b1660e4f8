"""The TicTacToe learner on the MI355X (spai_ttt_learner_*, spai_ttt_net_set_params,
spai_ttt.learn) against the PyTorch CPU fp32 golden and the numpy float64
restatement of the step (tests/ttt_learner_ref.py).

Inputs are encodings of positions reached by random legal play on the device
(the moves come from a seeded host generator, so the CPU measurement below saw
the same positions), random normalised pi, and z in {-1, 0, 1}.

Tolerances are the Connect4 learner tests' (same dtype, same 2*blocks+3 depth):
loss rtol 1e-4 at step 1 and 1e-3 later, gradient 3e-4 max|g|, parameters the
check_learner_params structure.  BatchNorm over 9 B values is worse conditioned
at B <= 2 than anything those tests see, so for every shape below the distance
of PyTorch CPU fp32 from the float64 restatement was measured on the CPU, on
these inputs and seeds (loss: relative; gradient: / max|g|; well-conditioned
parameters: absolute; running statistics: absolute at the last step):

    (blocks, B, steps)  loss      gradient  parameters  running stats
    (0,   1, 1)         5.8e-08   7.0e-07   1.3e-08     5.4e-08
    (1,   2, 1)         8.2e-08   3.4e-07   1.3e-08     5.3e-08
    (1,   5, 2)         1.3e-07   3.6e-07   4.2e-08     8.7e-05 (bound 2e-3)
    (2,  17, 2)         9.8e-08   2.7e-07   4.3e-08     8.2e-05 (bound 2e-3)
    (4,  32, 1)         1.1e-07   6.9e-07   1.3e-08     8.5e-08
    (2,  33, 1)         4.6e-08   4.1e-07   1.3e-08     5.4e-08
    (4, 128, 1)         2.5e-08   5.1e-07   1.3e-08     9.0e-08

Every one is far below a third of its bound (1e-4, 3e-4, 1e-4 x steps, 1e-5 at
step 1), so the Connect4 bounds stand unchanged for every shape."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    import spai_ttt
    return spai_ttt


def _play_on_device(eng, games, order):
    """the positions after the move lists `games` (longest first), played with the
    device's rules from the empty board; their encodings [n][27] in `order`"""
    import ttt_learner_ref as LR
    n = len(games)
    eng.games_resize(n)
    for k in range(len(games[0])):
        moving = sum(1 for g in games if len(g) > k)   # a prefix: the list is longest first
        rc = eng.apply([g[k] for g in games[:moving]])
        assert not rc.any()
    assert np.all(eng.games_read(n)["status"] == 0)
    x = eng.encode(n).reshape(n, 27)[order]
    assert np.array_equal(x, np.array([LR.encode_moves(g) for g in games])[order])
    return x


def _device_batches(eng, B, steps, seed):
    import ttt_learner_ref as LR
    games, order, batches = LR.make_batches(B, steps, seed)
    x = _play_on_device(eng, games, order)
    return [(x[k * B:(k + 1) * B], b[1], b[2]) for k, b in enumerate(batches)]


def test_ttt_learner_vs_torch_golden(st):
    """device train step (fp32) vs PyTorch CPU fp32: 3 Adam steps of the 1x64 net, B = 32"""
    import ttt_learner_ref as LR
    z = np.load(os.path.join(GOLDEN, "learner_ttt_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    batches = _device_batches(eng, B, K, seed)
    assert np.array_equal(np.array([b[0] for b in batches]), z["states"])   # the golden's inputs, from the device
    L = st.TTTLearner(eng, blocks, st.init_params(blocks, seed))
    losses = []
    for k in range(K):
        losses.append(L.train_batch(batches[k][0], z["policies"][k], z["values"][k]))
        if k == 0:
            g1, P1 = L.grads(), L.params()
    P3 = L.params()
    print("loss", np.array(losses), z["loss"])
    np.testing.assert_allclose(losses[0], z["loss"][0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(losses), z["loss"], rtol=1e-3, atol=1e-4)
    g_ref = z["grads1"]
    print("grad", np.abs(g1 - g_ref).max() / np.abs(g_ref).max())
    assert np.abs(g1 - g_ref).max() <= 3e-4 * np.abs(g_ref).max()
    LR.check_learner_params(P1, z["params1"], [g_ref], blocks, 1)
    params3 = np.load(os.path.join(GOLDEN, "learner_ttt_1x64_step3.npz"))["params3"]
    LR.check_learner_params(P3, params3, [g_ref], blocks, 3, tol=1e-4)
    L.close()
    eng.close()


def _check_grads_same_masks(L, g, p0, batch, blocks):
    """fp32 device gradient vs the float64 restatement run with the DEVICE's ReLU masks
    (activation > 0), the method of test_gpu_parity._check_grads_same_masks: the masks
    may differ from the restatement's own (pre > 0) only where its pre-activation is
    within 1e-4 of its layer's scale of zero; every entry within 3e-4 max|g|"""
    import ttt_learner_ref as LR
    nl = 2 * blocks + 3
    masks = [L.activation(l) > 0 for l in range(nl)]
    diag = {}
    n = len(p0)
    _, _, _, _, ref = LR.train_step(p0, np.zeros(n), np.zeros(n), 0, *batch, blocks, masks=masks, diag=diag)
    flips = 0
    for l in range(nl):
        pre = diag["pre"][l]
        diff = masks[l] != (pre > 0)
        flips += int(diff.sum())
        assert np.all(np.abs(pre[diff]) <= 1e-4 * np.abs(pre).max()), (l, np.abs(pre[diff]).max())
    d, m = np.abs(g - ref), np.abs(ref).max()
    print("grad vs f64 (device masks)", d.max() / m, "flips", flips)
    assert d.max() <= 3e-4 * m, (d.max() / m, flips)
    return flips


@pytest.mark.parametrize("blocks,B,steps", [(0, 1, 1), (1, 2, 1), (1, 5, 2), (2, 17, 2), (4, 32, 1), (2, 33, 1),
                                            (4, 128, 1)])
def test_ttt_learner_vs_restatement(st, blocks, B, steps):
    """one partial tile; a tile straddling two samples; 45 rows; 9 full tiles + 9 rows;
    the reference batch of 32; one more than a batch; full depth at 128"""
    import ttt_learner_ref as LR
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    batches = _device_batches(eng, B, steps, 1000 * blocks + B)
    p0 = st.init_params(blocks, blocks + 7)
    L = st.TTTLearner(eng, blocks, p0)
    dev_losses = [L.train_batch(*batches[0])]
    assert L.last_batch() == B
    g1 = L.grads()
    _check_grads_same_masks(L, g1, p0, batches[0], blocks)   # reads the first step's activations
    dev_losses += [L.train_batch(*b) for b in batches[1:]]
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks)
    print("loss", np.array(dev_losses), ref_losses)
    np.testing.assert_allclose(dev_losses[0], ref_losses[0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=1e-3, atol=1e-4)
    LR.check_learner_params(L.params(), P_ref, ref_grads, blocks, steps, tol=1e-4)
    L.close()
    eng.close()


@pytest.mark.parametrize("blocks,B,steps", [(1, 5, 2), (2, 33, 1), (2, 130, 1)])
def test_ttt_learner_trained_like_vs_restatement(st, blocks, B, steps):
    """the same check from bf16_ref.trained_like parameters: conv biases, beta and the
    running mean away from 0, the running variance away from 1, gammas above 1 and
    below 0, so the running-statistic blend and every factor of k_lc_bn_bwd count
    (from init_params the old running mean is 0 and drops out of the blend).  The
    restatement is pinned to PyTorch float64 autograd from such parameters in
    tests/test_learner_ref_cpu.py.  The bars are the ones above, unchanged."""
    import bf16_ref as R
    import ttt_learner_ref as LR
    from learner_checks import check_momentum_blend_is_tested, start_params
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    batches = _device_batches(eng, B, steps, 2000 * blocks + B)
    p0 = start_params(st.init_params(blocks, blocks + 7), R.c4_layout(blocks, 64, (3, 3, 3, 9)), "trained", 60 + blocks)
    L = st.TTTLearner(eng, blocks, p0)
    dev_losses = [L.train_batch(*batches[0])]
    assert L.last_batch() == B
    _check_grads_same_masks(L, L.grads(), p0, batches[0], blocks)   # reads the first step's activations
    dev_losses += [L.train_batch(*b) for b in batches[1:]]
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks)
    print("loss", np.array(dev_losses), ref_losses)
    np.testing.assert_allclose(dev_losses[0], ref_losses[0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=1e-3, atol=1e-4)
    LR.check_learner_params(L.params(), P_ref, ref_grads, blocks, steps, tol=1e-4)
    P1_ref = P_ref if steps == 1 else LR.train(p0, batches[:1], blocks)[0]
    print("running mean vs 0.1 * batch mean / vs old: %.3g / %.3g x the tolerance" % tuple(
        check_momentum_blend_is_tested(p0, P1_ref, LR._layout(blocks)[0])))
    L.close()
    eng.close()


def test_ttt_learner_deterministic(st):
    """two learners, the same parameters, the same two batches of 17: bit-identical"""
    blocks = 2
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    batches = _device_batches(eng, 17, 2, 5)
    p0 = st.init_params(blocks, 3)
    out = []
    for _ in range(2):
        L = st.TTTLearner(eng, blocks, p0)
        rec = []
        for b in batches:
            rec += [L.train_batch(*b), L.grads(), L.params()]
        out.append(rec)
        L.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][1]).max() > 0 and not np.array_equal(out[0][2], p0)
    eng.close()


def test_ttt_learner_train_epochs(st):
    """Model::train: a fresh Adam per call, one permutation of the samples, epochs x
    ceil(n/B) steps with a short last batch, vs the restatement fed the same permutation"""
    import spai
    import ttt_learner_ref as LR
    blocks, n, B, epochs, seed = 1, 70, 32, 2, 9
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    (x, pi, z), = _device_batches(eng, n, 1, 70)
    p0 = st.init_params(blocks, 5)
    L = st.TTTLearner(eng, blocks, p0)
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


def test_ttt_net_set_params(st):
    """after a train step, net.set_params(L.params()) == TTTNet(eng, blocks, L.params()), bit for bit"""
    blocks = 2
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    (x, pi, z), = _device_batches(eng, 64, 1, 64)
    p0 = st.init_params(blocks, 1)
    net = st.TTTNet(eng, blocks, p0)
    lg0, v0 = net.forward(x)
    L = st.TTTLearner(eng, blocks, p0)
    L.train_batch(x, pi, z)
    P = L.params()
    net.set_params(P)
    lg1, v1 = net.forward(x)
    fresh = st.TTTNet(eng, blocks, P)
    lg2, v2 = fresh.forward(x)
    assert np.array_equal(lg1, lg2) and np.array_equal(v1, v2)
    assert not np.array_equal(lg0, lg1)
    with pytest.raises(st.SpaiError) as ei:
        net.set_params(P[:-1])
    assert ei.value.code == -1
    L.close()
    fresh.close()
    net.close()
    eng.close()


def _self_play_samples(st, params, blocks, game_ids, seed, sims):
    eng = st.TTTEngine(num_searches=sims, max_trees=len(game_ids), seed=seed)
    eng.set_net(st.TTTNet(eng, blocks, params))
    games, _ = eng.self_play(len(game_ids), game_id_base=int(game_ids[0]))
    eng.close()
    return st._samples(games)


def test_ttt_learn_end_to_end(st, tmp_path):
    """Learner::learn: self-play -> train -> checkpoint, twice, on the device"""
    import spai
    blocks, seed, G, sims, iters = 1, 4, 32, 16, 3
    kw = dict(num_learn_iters=2, num_self_play_iters=iters, num_parallel_self_play_games=G, batch_size=32,
              num_epochs=2, num_searches=sims, blocks=blocks, seed=seed)
    p0 = st.init_params(blocks, seed)
    sets = {}
    rec = st.learn(checkpoint_dir=str(tmp_path / "a"), on_train_set=lambda i, *a: sets.__setitem__(i, a), **kw)
    assert [r["iteration"] for r in rec] == [0, 1] and all(np.isfinite(r["loss"]).all() for r in rec)
    ck = [spai.load_params(r["checkpoint"], blocks, game=spai.GAME_TICTACTOE, n=len(p0)) for r in rec]
    # checkpoint i is the learner's parameters after iteration i: a second learner fed the
    # same training sets (the step is deterministic) ends at the same bits
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    L = st.TTTLearner(eng, blocks, p0)
    for i in range(2):
        s, p, v, gid = sets[i]
        assert rec[i]["samples"] == len(v) and rec[i]["games"] == G
        L.train(s, p, v, epochs=2, batch=32, seed=st._iter_seed(seed, i))
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
    want = _self_play_samples(st, ck[0], blocks, ids1, seed, sims)
    assert all(np.array_equal(a[:m], b) for a, b in zip((s1, p1, v1), want))
    stale = _self_play_samples(st, p0, blocks, ids1, seed, sims)
    assert len(stale[2]) != m or not np.array_equal(stale[1], p1[:m])
    # two runs: bit-identical checkpoints
    rec2 = st.learn(checkpoint_dir=str(tmp_path / "b"), **kw)
    for r, c in zip(rec2, ck):
        assert np.array_equal(spai.load_params(r["checkpoint"], blocks, game=spai.GAME_TICTACTOE, n=len(p0)), c)
    # clone_self_play=False: num_self_play_iters distinct batches, disjoint game ids
    sets_d = {}
    st.learn(checkpoint_dir=str(tmp_path / "c"), clone_self_play=False,
             on_train_set=lambda i, *a: sets_d.__setitem__(i, a), **kw)
    all_ids = []
    for i in range(2):
        gid = sets_d[i][3]
        ids = np.unique(gid)
        assert len(ids) == iters * G and np.all(np.diff(gid) >= 0)
        all_ids += list(ids)
        parts = [sets_d[i][1][(gid >= ids[b * G]) & (gid <= ids[(b + 1) * G - 1])] for b in range(iters)]
        assert not any(len(parts[a]) == len(parts[b]) and np.array_equal(parts[a], parts[b])
                       for a in range(iters) for b in range(a))
    assert len(set(all_ids)) == 2 * iters * G
