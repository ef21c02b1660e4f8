"""Weight refresh of a chess net in place, packed on the device
(spai_chess_net_set_params, spai_chess_net_set_params_from_learner;
chess_net_pack.hip): HIP kernels fold BatchNorm in double and pack the bf16 MFMA
fragments (or lay out the fp32 net's buffer) from the flat fp32 parameters, which
are a host array or a learner's own device buffer.  The yardstick everywhere is a
fresh ChessNet(eng, blocks, P, dtype=...), that is spai_chess_net_create's host
packing, and every comparison is np.array_equal: of the packed weights themselves
(ChessNet.image: a zero input plane or a discarded output row would hide a wrong
padded lane from forward), of forward and predict, of whole self-play runs and of
spai_chess.learn's checkpoints.

Parameters: init_params, and bf16_ref.trained_like ones (non-identity BatchNorm
statistics, biases, negative gammas).  The rounding test puts policy-head weights
(scale exactly 1) on exact bf16 ties in both directions around 1.0 and 2^-120, and
-0.0, fp32 denormals and +-inf (under a non-zero finite scale) among the weights.
NaN parameters are outside the bit-equality claim: a host NaN's sign and payload
need not match the device's.

Shapes: blocks 0 (the w_res / b_res placeholders are left alone), 1 and 2 (the
trunk launch's layer stride) in both dtypes, and 20 blocks in bf16 (the size the
refresh is for: every trunk layer offset, 24 M elements).  forward runs 5 dense
inputs and one batch of 71, more than a workgroup's position split (70)."""
import numpy as np
import pytest

import bf16_ref as R

pytestmark = pytest.mark.gpu

CASES = [(d, b) for d in ("bf16", "f32") for b in (0, 1, 2)] + [("bf16", 20)]


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


def _engine(sc, **kw):
    return sc.ChessEngine(num_searches=kw.pop("num_searches", 1), max_trees=kw.pop("max_trees", 1), max_moves=64, **kw)


_PARAMS = {}


def _params(sc, blocks):
    """P1: init parameters; P2: trained-like ones of another seed (computed once, never written)"""
    if blocks not in _PARAMS:
        p1 = sc.init_params(blocks, 1)
        p2 = R.trained_like(sc.init_params(blocks, 2), R.chess_layout(blocks), 7 + blocks)
        for p in (p1, p2):
            p.setflags(write=False)
        _PARAMS[blocks] = p1, p2
    return _PARAMS[blocks]


def _x():
    return R.chess_probe_inputs(5), R.binary_planes(71, 19, 8, 8, seed=14, density=0.3)


def _slots(eng, n=3, plies=4):
    """n game slots, slot i after plies + i applied legal moves"""
    eng.games_resize(n)
    for k in range(plies + n):
        mv, cnt = eng.legal_moves(n)
        assert cnt.min() > 0
        for i in range(n):
            if k < plies + i:
                eng.apply(mv[i:i + 1, (3 * k + i) % cnt[i]], first=i)


def _outputs(net):
    """forward on the dense inputs and the batch of 71, predict over the engine's 3 slots"""
    out = []
    for x in _x():
        out += list(net.forward(x))
    return out + list(net.predict(3))


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg="%s, array %d" % (what, i))


def _assert_image(net, fresh, what):
    a, b = net.image(), fresh.image()
    assert a.shape == b.shape and a.size > 0
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d image bytes differ, the first at byte %d of %d" % (what, bad.size, bad[0], a.size))


@pytest.mark.parametrize("dtype,blocks", CASES)
def test_host_refresh_equals_fresh_net(sc, dtype, blocks):
    p1, p2 = _params(sc, blocks)
    eng = _engine(sc)
    fresh1, fresh2 = sc.ChessNet(eng, blocks, p1, dtype=dtype), sc.ChessNet(eng, blocks, p2, dtype=dtype)
    assert not np.array_equal(fresh1.image(), fresh2.image())
    net = sc.ChessNet(eng, blocks, p1, dtype=dtype)
    h = net.h.value
    net.set_params(p2)
    assert net.h.value == h
    _assert_image(net, fresh2, "after set_params(P2)")
    if blocks <= 2:
        _slots(eng)
        want1, want2 = _outputs(fresh1), _outputs(fresh2)
        assert all(np.isfinite(a).all() for a in want1 + want2)
        assert not any(np.array_equal(a, b) for a, b in zip(want1, want2))
        _assert_same(_outputs(net), want2, "outputs after set_params(P2)")
    net.set_params(p1)
    _assert_image(net, fresh1, "after set_params(P1) again")
    if blocks <= 2:
        _assert_same(_outputs(net), want1, "outputs after set_params(P1) again")
    for n in (net, fresh1, fresh2):
        n.close()
    eng.close()


@pytest.mark.parametrize("blocks", [0, 1])
def test_rounding_and_padding(sc, blocks):
    """bf16 ties both ways, signed zeros, denormals and infinities pack as on the host"""
    p1, p2 = _params(sc, blocks)
    p = np.array(p2, np.float32, copy=True)
    d = R.unflatten(p, R.chess_layout(blocks))
    # 1 + m * 2^-8, m odd, is halfway between two bf16 values: m = 1, 5, 9, ... tie towards the
    # even neighbour below, m = 3, 7, 11, ... towards the even neighbour above
    m = np.arange(1, 129, 2, dtype=np.float64)
    ties = np.concatenate([1.0 + m * 2.0 ** -8, -(1.0 + m * 2.0 ** -8)])
    ties = np.concatenate([ties, ties * 2.0 ** -120]).astype(np.float32)
    for name in ("p1.w", "p2.w"):
        w = d[name].reshape(-1)
        w[:ties.size] = ties
        w[-ties.size:] = ties[::-1]      # the last output channels too: p2's 73rd borders the padding
        w[1000:1004] = [-0.0, 1e-40, -3e-39, 0.0]
    special = np.array([-0.0, 1e-40, -3e-39, 1.1754942e-38, np.inf, -np.inf, 0.0, -1e-45], np.float32)
    for name in ["stem.w"] + ["res%d.w" % i for i in range(2 * blocks)]:
        w = d[name].reshape(-1)
        w[5:5 + special.size] = special
        w[-special.size:] = special[::-1]
        assert np.isfinite(d[name[:-1] + "g"]).all() and (d[name[:-1] + "g"] != 0).all()
    assert not np.isnan(p).any()
    eng = _engine(sc)
    fresh = sc.ChessNet(eng, blocks, p)
    net = sc.ChessNet(eng, blocks, p1)
    net.set_params(p)
    _assert_image(net, fresh, "special values")
    img = fresh.image()
    plain = sc.ChessNet(eng, blocks, p2)
    assert not np.array_equal(img, plain.image())
    plain.close()
    # the ties really went both ways on the yardstick: both roundings of 1 + m * 2^-8 appear in w_p1
    n_stem, n_res = 9 * 16 * 512, max(2 * blocks * 9 * 8 * 16 * 512, 8)
    w_p1 = img[2 * (n_stem + n_res):][:2 * 8 * 16 * 512].view(np.uint16)
    assert (w_p1 == 0x3F80).any() and (w_p1 == 0x3F82).any() and (w_p1 == 0xBF82).any()
    net.close()
    fresh.close()
    eng.close()


def _batch(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 19 * 64)) < 0.3).astype(np.float32)
    pi = rng.random((n, 4672)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    return x, pi, rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32)


@pytest.mark.parametrize("dtype,compute,full", [("bf16", "f32", True), ("bf16", "bf16", False), ("f32", "f32", False)])
def test_device_refresh_equals_fresh_net(sc, dtype, compute, full):
    blocks = 1
    p0 = _params(sc, blocks)[0]
    eng = _engine(sc)
    _slots(eng)
    net, net_h = sc.ChessNet(eng, blocks, p0, dtype=dtype), sc.ChessNet(eng, blocks, p0, dtype=dtype)
    before = net.image()
    batch = _batch(17, 3)
    L = sc.ChessLearner(eng, blocks, p0, compute=compute)
    L.train_batch(*batch)
    net.set_params(L)            # straight behind the step, no host call in between
    got_img, got = net.image(), _outputs(net)
    p = L.params()
    d, d0 = R.unflatten(p, R.chess_layout(blocks)), R.unflatten(p0, R.chess_layout(blocks))
    assert np.abs(d["stem.mu"] - d0["stem.mu"]).max() > 1e-3 and np.abs(d["res1.var"] - d0["res1.var"]).max() > 1e-3
    fresh = sc.ChessNet(eng, blocks, p, dtype=dtype)
    net_h.set_params(p)
    assert not np.array_equal(got_img, before)
    _assert_image(net, fresh, "set_params(learner)")
    _assert_image(net_h, fresh, "set_params(learner.params())")
    want = _outputs(fresh)
    _assert_same(got, want, "set_params(learner) against a fresh net")
    _assert_same(_outputs(net_h), want, "set_params(learner.params()) against a fresh net")
    if full:   # a snapshot, not an alias
        L.train_batch(*batch)
        assert np.array_equal(net.image(), got_img)
        net.set_params(L)
        assert not np.array_equal(net.image(), got_img)
        fresh2 = sc.ChessNet(eng, blocks, L.params(), dtype=dtype)
        _assert_image(net, fresh2, "the second set_params(learner)")
        fresh2.close()
    L.close()
    for n in (net, net_h, fresh):
        n.close()
    eng.close()


def test_refresh_reaches_self_play(sc):
    """self-play on the engine's current net after set_params(learner) is self-play of a fresh
    engine with a fresh net of the learner's parameters"""
    blocks, G, sims, seed, base = 1, 4, 8, 3, 8
    p0 = _params(sc, blocks)[0]
    eng = sc.ChessEngine(num_searches=sims, max_trees=G, seed=seed)
    eng.set_net(sc.ChessNet(eng, blocks, p0))
    L = sc.ChessLearner(eng, blocks, p0)
    L.train_batch(*_batch(17, 3))
    eng.net.set_params(L)
    games, _ = eng.self_play(G, game_id_base=base)
    p = L.params()
    L.close()
    eng.close()
    ref = sc.ChessEngine(num_searches=sims, max_trees=G, seed=seed)
    ref.set_net(sc.ChessNet(ref, blocks, p))
    want, _ = ref.self_play(G, game_id_base=base)
    ref.close()
    assert [g["game"] for g in sorted(games, key=lambda g: g["game"])] == list(range(base, base + G))
    _assert_same(sc._samples(games), sc._samples(want), "self-play samples")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_errors_leave_the_weights_alone(sc, dtype):
    p1, p2 = _params(sc, 1)
    eng, eng2 = _engine(sc), _engine(sc)
    net = sc.ChessNet(eng, 1, p1, dtype=dtype)
    before = net.image()
    Lo = sc.ChessLearner(eng2, 1, p2)                          # another engine
    with pytest.raises(sc.SpaiError) as ei:
        net.set_params(Lo)
    assert ei.value.code == -1 and "engine" in str(ei.value)
    Lo.close()
    L2 = sc.ChessLearner(eng, 2, _params(sc, 2)[1])            # another block count
    with pytest.raises(sc.SpaiError) as ei:
        net.set_params(L2)
    assert ei.value.code == -1 and "blocks" in str(ei.value)
    L2.close()
    with pytest.raises(sc.SpaiError) as ei:                    # a short host array
        net.set_params(p2[:-1])
    assert ei.value.code == -1
    assert np.array_equal(net.image(), before)
    small = np.zeros(before.size - 1, np.uint8)                # image: a short buffer is refused
    n = sc.C.c_size_t()
    assert sc.lib().spai_chess_net_image(net.h, sc._p(small), small.size, sc.C.byref(n)) == -1 and n.value == before.size
    net.close()
    eng.close()
    eng2.close()


def test_learn_device_and_host_refresh_agree(sc, tmp_path):
    import spai
    blocks = 1
    kw = dict(num_learn_iters=2, num_self_play_iters=1, num_parallel_self_play_games=4, batch_size=32, num_epochs=1,
              num_searches=8, blocks=blocks, seed=4)
    runs = {}
    for how in ("device", "host"):
        sets, phases = {}, []
        rec = sc.learn(checkpoint_dir=str(tmp_path / how), refresh=how,
                       on_train_set=lambda i, *a: sets.__setitem__(i, a), on_phase=lambda *a: phases.append(a[:2]), **kw)
        n = sc.num_params(blocks)
        ck = [spai.load_params(r["checkpoint"], blocks, hidden=256, game=spai.GAME_CHESS, n=n) for r in rec]
        assert phases == [(0, "self_play"), (0, "train"), (1, "refresh"), (1, "self_play"), (1, "train")]
        runs[how] = sets, ck
    (sets_d, ck_d), (sets_h, ck_h) = runs["device"], runs["host"]
    for i in range(2):
        _assert_same(sets_d[i], sets_h[i], "training set %d" % i)
        np.testing.assert_array_equal(ck_d[i], ck_h[i], err_msg="checkpoint %d" % i)
    assert not np.array_equal(ck_d[0], ck_d[1])
