"""The chess learner's bf16 compute type on the MI355X (spai_chess_learner_set_compute,
the capture window, spai_chess.learn(compute="bf16")) against the float64
restatement that carries its rounding points (tests/chess_learner_bf16_ref.py;
with round = identity it is the fp32 restatement, pinned to PyTorch float64).

Why layer by layer: a whole bf16 step cannot be held tighter than about 2e-3 of
max|g| (another fp32 summation order of the same quantised step already ends
3e-4 .. 7e-4 away, through rare rounding flips that propagate), and truncation
instead of rounding, or a residual read from a bf16 copy, move it by no more than
that.  So every GEMM is recomputed in float64 from the DEVICE's own tensors (its
activations, its captured gradients), rounded as the contract says, and compared
at the fp32 learner tests' bars: activations within 1e-4 max|pre-activation| under
the device's ReLU mask (flips only inside that window), logits 1e-4 max|logit|,
running statistics rtol 1e-4 + 1e-5, weight / data gradients and dlogits 3e-4
max|tensor|, gamma / beta / bias / value-head gradients 3e-4 max|g|.  One bar is
not a tolerance but a rounding bound: the gradient of a conv bias under a
BatchNorm is exactly 0 in exact arithmetic, and is held to what fp32 can leave of
it (chess_learner_bf16_ref.zero_bias_bound), in both compute types.
tests/test_chess_learner_bf16_cpu.py shows, on these inputs, that three fp32
summation orders stay under 1 % of those bars and which planted faults trip them.

Shapes (blocks, B): a conv workgroup owns one sample (B = 1, 2, 3); the weight
gradient cuts the batch into chunks of 8 samples (7, 8, 9; 33 = five chunks, the
last of one sample); two blocks (a skip path under a skip path) and the
reference's depth.  Every shape runs the 19-channel stem (one K chunk of 64, 45
channels of zeros) and the 73-channel policy conv (a masked second row tile
forward, a K padded to 128 backward).  The same checker with round = identity
runs on the fp32 path at the same shapes and bars: the control."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (1, 3), (1, 7), (1, 8), (1, 9), (1, 33), (2, 5), (10, 2)]


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


def _engine(sc):
    return sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)


_BATCHES = {}


def _device_batches(sc, eng, B, steps, seed):
    """positions of random legal play, replayed with the device's rules (as tests/test_chess_learner_gpu.py)"""
    import chess_learner_ref as LR
    if (B, steps, seed) not in _BATCHES:
        _BATCHES[B, steps, seed] = LR.make_batches(B, steps, seed)
    games, order, batches = _BATCHES[B, steps, seed]
    n = len(games)
    eng.games_resize(n)
    for k in range(len(games[0])):
        moving = sum(1 for g in games if len(g) > k)   # a prefix: the list is longest first
        assert not eng.apply(np.array([g[k] for g in games[:moving]], np.uint16)).any()
    x = eng.encode(n).reshape(n, 1216)[order]
    assert np.array_equal(x, np.concatenate([b[0] for b in batches]))
    return [(x[k * B:(k + 1) * B], b[1], b[2]) for k, b in enumerate(batches)]


def _start(sc, blocks, start):
    import bf16_ref as R
    from learner_checks import start_params
    return start_params(sc.init_params(blocks, blocks + 7), R.chess_layout(blocks), start, 60 + blocks)


def _record(L, blocks, loss):
    """the device's tensors of the last (captured) step, as chess_learner_bf16_ref.check_local reads them"""
    nt = 2 * blocks + 1
    return dict(a=[L.activation(l) for l in range(nt)], ap1=L.activation(nt), vc=L.activation(nt + 1),
                h1=L.activation(nt + 2), logits=L.logits(), dz=[L.gradient(l) for l in range(nt)],
                dp1=L.gradient(nt), dlogits=L.gradient(nt + 1), G=L.grads(), P1=L.params(), loss=loss)


def _layer_local(sc, start, blocks, B, compute):
    import chess_learner_bf16_ref as Q
    eng = _engine(sc)
    (batch,) = _device_batches(sc, eng, B, 1, (1000 if start == "init" else 2000) * blocks + B)
    p0 = _start(sc, blocks, start)
    L = sc.ChessLearner(eng, blocks, p0, compute=compute)
    assert L.compute() == compute
    L.set_capture(True)
    loss = L.train_batch(*batch)
    checks = Q.check_local(p0, *batch, blocks, _record(L, blocks, loss),
                           round=Q.bf16_round if compute == "bf16" else Q.identity)
    L.close()
    eng.close()
    worst = sorted(((e / b, k) for k, (e, b) in checks.items()), reverse=True)[:5]
    print("%s %s (%d, %d): worst error / bar %s" % (compute, start, blocks, B, ["%s %.3g" % (k, r) for r, k in worst]))
    print("   gradient of the conv biases under BatchNorm / its fp32 bound: %.3g"
          % max(e / b for k, (e, b) in checks.items() if k.startswith("zero_bias")))
    assert not Q.failures(checks), Q.failures(checks)
    return checks


@pytest.mark.parametrize("start", ["init", "trained"])
@pytest.mark.parametrize("blocks,B", SHAPES)
def test_bf16_step_layer_by_layer(sc, blocks, B, start):
    _layer_local(sc, start, blocks, B, "bf16")


@pytest.mark.parametrize("start", ["init", "trained"])
@pytest.mark.parametrize("blocks,B", SHAPES)
def test_control_fp32_step_layer_by_layer(sc, blocks, B, start):
    """the same checker, round = identity, on the fp32 path: it is the checker that is trusted"""
    _layer_local(sc, start, blocks, B, "f32")


def test_checker_tells_the_compute_types_apart(sc):
    """the bf16 step misses the unrounded recomputation, the fp32 step the rounded one"""
    import chess_learner_bf16_ref as Q
    blocks, B = 1, 9
    eng = _engine(sc)
    (batch,) = _device_batches(sc, eng, B, 1, 1000 * blocks + B)
    p0 = _start(sc, blocks, "init")
    for compute, wrong in (("bf16", Q.identity), ("f32", Q.bf16_round)):
        L = sc.ChessLearner(eng, blocks, p0, compute=compute)
        L.set_capture(True)
        loss = L.train_batch(*batch)
        bad = Q.failures(Q.check_local(p0, *batch, blocks, _record(L, blocks, loss), round=wrong), 3.0)
        L.close()
        assert any(k.startswith("g_w") for k in bad) and "logits" in bad, sorted(bad)
    eng.close()


def test_capture_errors(sc):
    blocks, B = 0, 2
    eng = _engine(sc)
    (batch,) = _device_batches(sc, eng, B, 1, 77)
    L = sc.ChessLearner(eng, blocks, sc.init_params(blocks, 1))

    def invalid(f):
        with pytest.raises(sc.SpaiError) as ei:
            f()
        assert ei.value.code == -1

    lib = sc.lib()
    buf = np.zeros(B * 4672, np.float32)
    invalid(lambda: sc._check(lib.spai_chess_learner_logits(L.h, sc._p(buf), buf.size)))   # no step yet
    L.train_batch(*batch)
    assert L.logits().shape == (B, 4672)
    invalid(lambda: L.gradient(0))                                                        # capture off
    L.set_capture(True)
    invalid(lambda: L.gradient(0))                                                        # the last step: not captured
    L.train_batch(*batch)
    assert L.gradient(0).shape == (B, 256, 8, 8) and L.gradient(2).shape == (B, 4672)
    invalid(lambda: L.gradient(3))                                                        # past the last layer
    invalid(lambda: L.gradient(-1))
    invalid(lambda: sc._check(lib.spai_chess_learner_gradient(L.h, 0, sc._p(buf), buf.size - 1)))   # wrong n
    invalid(lambda: sc._check(lib.spai_chess_learner_logits(L.h, sc._p(buf), buf.size - 1)))
    invalid(lambda: sc._check(lib.spai_chess_learner_set_compute(L.h, 2)))
    assert L.compute() == "f32"
    L.set_capture(False)
    invalid(lambda: L.gradient(0))
    L.close()
    eng.close()


def test_bf16_whole_step(sc):
    """step-1 loss within 4 x the spread of three fp32 summation orders of the quantised
    restatement around its float64 form (the bound is computed here; it must come out
    under 1e-3 relative); parameters after 2 steps within Adam's 2 lr steps + 1e-5"""
    import chess_learner_bf16_ref as Q
    blocks, B, steps, lr = 2, 5, 2, 1e-3
    eng = _engine(sc)
    batches = _device_batches(sc, eng, B, steps, 1000 * blocks + B)
    p0 = _start(sc, blocks, "init")
    ref = Q.step(p0, *batches[0], blocks, round=Q.bf16_round)["loss"]
    orders = [Q.step(p0, *batches[0], blocks, round=Q.bf16_round, mm=mm, store=Q.to_f32)["loss"] for mm in Q.F32_ORDERS]
    bound = 4 * max(np.abs(o - ref).max() for o in orders) / np.abs(ref).max()
    L = sc.ChessLearner(eng, blocks, p0, compute="bf16")
    losses = [L.train_batch(*b) for b in batches]
    P = L.params()
    L.close()
    eng.close()
    d = np.abs(losses[0] - ref).max() / np.abs(ref).max()
    print("step-1 loss %s vs %s: %.3g relative, bound 4 x fp32-order spread = %.3g" % (losses[0], ref, d, bound))
    assert bound < 1e-3
    assert d <= bound
    P_ref, _ = Q.train(p0, batches, blocks, lr=lr, round=Q.bf16_round)
    dp = np.abs(P - P_ref).max()
    print("parameters after %d steps: %.3g (bound %.3g)" % (steps, dp, 2 * lr * steps + 1e-5))
    assert np.isfinite(P).all() and dp <= 2 * lr * steps + 1e-5


def test_bf16_train_lowers_the_loss(sc):
    """Model::train in bf16: 3 epochs x (32, 32, 6) = 9 steps with short last batches"""
    blocks, n = 1, 70
    eng = _engine(sc)
    (x, pi, z), = _device_batches(sc, eng, n, 1, 70)
    L = sc.ChessLearner(eng, blocks, sc.init_params(blocks, 5), compute="bf16")
    L.train(x, pi, z, epochs=3, batch=32, seed=9)
    assert L.last_batch() == 6
    after = L.train_batch(x, pi, z)      # the loss of the whole set under the trained parameters
    P = L.params()
    L.close()
    L = sc.ChessLearner(eng, blocks, sc.init_params(blocks, 5), compute="bf16")
    before = L.train_batch(x, pi, z)
    L.close()
    eng.close()
    print("loss of the set before %s, after 9 steps %s" % (before, after))
    assert np.isfinite(after).all() and np.isfinite(P).all() and after[0] < before[0]


def _run(L, batches, computes=None, capture=None):
    rec = []
    for k, b in enumerate(batches):
        if computes is not None:
            L.set_compute(computes[k])
        if capture is not None:
            L.set_capture(capture[k])
        rec += [L.train_batch(*b), L.grads(), L.params()]
    return rec


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_determinism_and_isolation(sc):
    blocks, B = 2, 17
    eng = _engine(sc)
    batches = _device_batches(sc, eng, B, 3, 5)
    p0 = sc.init_params(blocks, 3)

    def learner(**kw):
        return sc.ChessLearner(eng, blocks, p0, **kw)

    # two bf16 learners: bit-identical; capture on = capture off
    A, Bq, Cq = learner(compute="bf16"), learner(compute="bf16"), learner(compute="bf16")
    ra, rb = _run(A, batches), _run(Bq, batches)
    rc = _run(Cq, batches, capture=[True, False, True])
    assert _same(ra, rb) and _same(ra, rc)
    # compute="f32" set explicitly = the default, bit for bit; and it is not the bf16 step
    D, E, F = learner(), learner(compute="f32"), learner()
    rd, re = _run(D, batches), _run(E, batches)
    rf = _run(F, batches, capture=[True, True, False])
    assert _same(rd, re) and _same(rd, rf)
    assert not np.array_equal(rd[1], ra[1]) and not np.array_equal(rd[0], ra[0])
    # f32 -> bf16 -> f32 on one learner keeps parameters, Adam moments and step count: the
    # same as a learner created in bf16 and told each step's compute type before it
    mix = ["f32", "bf16", "f32"]
    G, H = learner(), learner(compute="bf16")
    rg = [G.train_batch(*batches[0]), G.grads(), G.params()]
    G.set_compute("bf16")
    rg += [G.train_batch(*batches[1]), G.grads(), G.params()]
    G.set_compute("f32")
    rg += [G.train_batch(*batches[2]), G.grads(), G.params()]
    rh = _run(H, batches, computes=mix, capture=[False, True, False])
    assert _same(rg, rh)
    assert _same(rg[:3], rd[:3]) and not np.array_equal(rg[4], rd[4])
    # the moments were kept: a fresh f32 learner from the parameters after step 2 takes another third step
    fresh = sc.ChessLearner(eng, blocks, rg[5])
    fresh.train_batch(*batches[2])
    assert np.array_equal(fresh.grads(), rg[7]) and not np.array_equal(fresh.params(), rg[8])
    for l in (A, Bq, Cq, D, E, F, G, H, fresh):
        l.close()
    eng.close()


def _self_play_samples(sc, params, blocks, game_ids, seed, sims):
    eng = sc.ChessEngine(num_searches=sims, max_trees=len(game_ids), seed=seed)
    eng.set_net(sc.ChessNet(eng, blocks, params))
    games, _ = eng.self_play(len(game_ids), game_id_base=int(game_ids[0]))
    eng.close()
    return sc._samples(games)


def test_chess_learn_bf16_end_to_end(sc, tmp_path):
    """Learner::learn with the bf16 train step, at the size of test_chess_learn_end_to_end"""
    import spai
    blocks, seed, G, sims, iters = 1, 4, 4, 8, 2
    kw = dict(num_learn_iters=2, num_self_play_iters=iters, num_parallel_self_play_games=G, batch_size=32,
              num_epochs=1, num_searches=sims, blocks=blocks, seed=seed)
    p0 = sc.init_params(blocks, seed)
    sets = {}
    rec = sc.learn(checkpoint_dir=str(tmp_path / "a"), on_train_set=lambda i, *a: sets.__setitem__(i, a),
                   compute="bf16", **kw)
    assert [r["iteration"] for r in rec] == [0, 1] and all(np.isfinite(r["loss"]).all() for r in rec)
    ck = [spai.load_params(r["checkpoint"], blocks, hidden=256, game=spai.GAME_CHESS, n=len(p0)) for r in rec]
    assert all(np.isfinite(c).all() for c in ck)
    # checkpoint i is a bf16 learner's parameters after iteration i, and not an fp32 learner's
    eng = _engine(sc)
    L, L32 = sc.ChessLearner(eng, blocks, p0, compute="bf16"), sc.ChessLearner(eng, blocks, p0)
    for i in range(2):
        s, p, v, gid = sets[i]
        L.train(s, p, v, epochs=1, batch=32, seed=sc._iter_seed(seed, i))
        assert np.array_equal(L.params(), ck[i])
    s, p, v, gid = sets[0]
    L32.train(s, p, v, epochs=1, batch=32, seed=sc._iter_seed(seed, 0))
    assert not np.array_equal(L32.params(), ck[0])
    L.close()
    L32.close()
    eng.close()
    # the refreshed self-play net equals a fresh one: iteration 1's samples are the games played from checkpoint 0
    s1, p1, v1, gid1 = sets[1]
    m = len(v1) // iters
    want = _self_play_samples(sc, ck[0], blocks, np.unique(gid1), seed, sims)
    assert all(np.array_equal(a[:m], b) for a, b in zip((s1, p1, v1), want))
