"""The Connect4 search's opt-in Dirichlet root noise on the MI355X: the draws
(csrc/dirichlet.h through k_noise_draws), k_root_noise at its launch points in every
launch regime, the keyed search, self-play's keys, the net path and the cache.

Yardsticks (tests/c4_noise_ref.py, pinned on the CPU by test_c4_root_noise_cpu.py), none
of which runs the device code under test:
  (a) NoisedSearch   the oracle's Mcts::search with the hash evaluator as a callback that
                     mixes eta at the roots (fresh roots)
  (b) PyTree         mcts.rs:196-332 and self-play restated on float32 numpy (reused
                     roots, every launch regime, self-play)
  mix                spai.h's float32 mix (chess_noise_ref)
  check_draws        the draws' distribution (dirichlet_stats)
eta always comes from spai_root_noise; everything but check_draws is compared bit for bit.
The launch regimes run at 8 simulations: by 32 a mix enqueued after the first selection
has usually visited the same nodes again (test_c4_root_noise_cpu.py, SEED), at 8 it shows
in most trees, and the test asserts that the yardstick itself tells the two apart.
"""
import os

import numpy as np
import pytest

import c4_noise_ref as NR
import c4_search_ref as R
import dirichlet_stats as DS

pytestmark = pytest.mark.gpu

ALPHA, EPS, SEED, NPOS, SIMS = 0.3, 0.25, 16, 12, 32
REG_SIMS = 8
TAIL_ENV = {"SPAI_TAIL_LEAVES": "0", "SPAI_TAIL_TREE_EVALS": "1000", "SPAI_TAIL_RUN": "3"}


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine(spai, n, sims=SIMS, noise=(ALPHA, EPS), seed=5, kind=None, **kw):
    return spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH if kind is None else kind, seed=seed,
                       root_noise=noise, **kw)


def plant(eng, roots):
    eng.trees_create(len(roots))
    for t, s in enumerate(roots):
        eng.tree_reset(t, R.key_of(s) + (0,))


def keys_of(trees, move=0):
    """the test's keys of these trees: game ids above 2^32, move numbers that differ between trees"""
    t = np.asarray(trees).astype(np.int64)
    return ((1 << 33) + 100 + t).astype(np.uint64), (move + t % 3).astype(np.uint32)


def draws_for(eng, trees, keys, nch):
    eta = eng.root_noise_draws(keys[0], keys[1], nch)
    return [eta[i, :nch[i]].copy() for i in range(len(trees))]


def device_record(eng, t, root_id=0):
    """(root N, root W, children (N, W, P)) of tree t as the device holds them"""
    ids, vis, w, pr = eng.tree_child_stats(t)
    _, n, rw = eng.tree_node(t, root_id)
    return n, np.float32(rw), vis, w, pr


def assert_tree_is(eng, t, tr, what, root_id=0):
    n, w, cvis, cw, cpr = device_record(eng, t, root_id)
    acts, rn, rw, rp = tr.children()
    assert (n, bits(w)) == (tr.root_record()[0], bits(tr.root_record()[1])), (what, t, "root")
    assert np.array_equal(cvis, rn), (what, t, cvis, rn)
    assert np.array_equal(bits(cw), bits(rw)), (what, t, "W")
    assert np.array_equal(bits(cpr), bits(rp)), (what, t, "P", int((bits(cpr) != bits(rp)).sum()))


def assert_search_is(got, i, tr, what):
    pol, ids, vis, nc = got
    k = len(tr.root.children)
    assert nc[i] == k and np.array_equal(vis[i, :k], tr.visits()) and not vis[i, k:].any(), (what, i, vis[i], tr.visits())
    assert pol[i].tobytes() == tr.policy().tobytes(), (what, i)


@pytest.fixture(scope="module")
def pos(spai):
    p = R.positions(NPOS, SEED)
    assert any(s.n == 0 for s in p) and any(R.has_full_column(s) for s in p) and any(R.wins_in_one(s) for s in p)
    return p


# ---- 2. the draws
def test_draws_equal_the_chess_engines(spai):
    import spai_chess as sc
    seed = 77
    c4 = engine(spai, 1, sims=1, noise=None, seed=seed)
    ch = sc.ChessEngine(num_searches=1, max_trees=1, eval_kind=sc.EVAL_HASH, seed=seed)
    rng = np.random.default_rng(1)
    gid = np.concatenate([rng.integers(0, 1000, 32), rng.integers(1 << 32, 1 << 63, 32)]).astype(np.uint64)
    mv = rng.integers(0, 42, 64).astype(np.uint32)
    for n in range(1, 8):
        for alpha in (0.03, 0.3, 1.0, 3.0):
            a = c4.root_noise_draws(gid, mv, np.full(64, n), alpha)
            b = ch.root_noise_draws(gid, mv, np.full(64, n), alpha)
            assert a.shape == (64, 7) and not a[:, n:].any() and not b[:, n:].any(), (n, alpha)
            assert np.array_equal(bits(a[:, :n]), bits(b[:, :n])), (n, alpha)
            if n == 1:
                assert bits(a[:, 0]).tolist() == [0x3F800000] * 64, alpha      # exactly 1.0
    other = engine(spai, 1, sims=1, noise=None, seed=seed + 1)
    assert not np.array_equal(bits(other.root_noise_draws(gid, mv, np.full(64, 7), 0.3)),
                              bits(c4.root_noise_draws(gid, mv, np.full(64, 7), 0.3)))
    for e in (c4, ch, other):
        e.close()


def test_draws_do_not_depend_on_the_batch(spai):
    eng = engine(spai, 1, sims=1, noise=None)
    N = 20000
    rng = np.random.default_rng(3)
    gid = rng.integers(0, 1 << 40, N, dtype=np.uint64)
    mv = rng.integers(0, 42, N).astype(np.uint32)
    n = rng.integers(1, 8, N).astype(np.uint32)
    a = eng.root_noise_draws(gid, mv, n, ALPHA)
    for i in (0, 1, 4097, N - 1):
        alone = eng.root_noise_draws(gid[i:i + 1], mv[i:i + 1], n[i:i + 1], ALPHA)
        assert alone[0].tobytes() == a[i].tobytes(), i
    perm = rng.permutation(N)
    assert eng.root_noise_draws(gid[perm], mv[perm], n[perm], ALPHA).tobytes() == a[perm].tobytes()
    assert eng.root_noise_draws(gid[:1], mv[:1], n[:1]).tobytes() == a[0].tobytes()   # the engine's alpha: 0.3
    eng.close()


@pytest.mark.parametrize("n,alpha", [(7, 0.3), (7, 1.0), (2, 1.0)])
def test_draws_are_dirichlet(spai, n, alpha):
    eng = engine(spai, 1, sims=1, noise=None)
    N = 20000
    rng = np.random.default_rng([n, int(alpha * 10)])
    eta = eng.root_noise_draws(rng.integers(0, 1 << 63, N, dtype=np.uint64), rng.integers(0, 42, N), np.full(N, n), alpha)
    eng.close()
    assert not eta[:, n:].any()
    m = DS.check_draws(np.ascontiguousarray(eta[:, :n]), alpha)
    print(n, alpha, {k: m[k] for k in ("sum_err", "sum_bound", "z_max", "var_ratio", "ks_p")})


def test_validation(spai):
    eng = engine(spai, 2, sims=4, noise=None)
    assert eng.get_root_noise() == (np.float32(0.3), 0.0)      # a new engine: alpha 0.3, off
    eng.set_root_noise(0.5, 0.25)
    for alpha, eps, field in ((0.009, 0.25, "alpha"), (100.5, 0.25, "alpha"), (float("nan"), 0.25, "alpha"),
                              (0.3, -0.01, "epsilon"), (0.3, 1.01, "epsilon"), (0.3, float("nan"), "epsilon"),
                              (-1.0, 0.0, "alpha")):
        with pytest.raises(spai.SpaiError) as ex:
            eng.set_root_noise(alpha, eps)
        assert ex.value.code == -1 and ("root noise: " + field) in str(ex.value), (alpha, eps, str(ex.value))
        assert eng.get_root_noise() == (np.float32(0.5), np.float32(0.25))   # a refused call changes nothing
    for alpha, eps in ((0.01, 0.0), (100.0, 1.0)):
        eng.set_root_noise(alpha, eps)
        assert eng.get_root_noise() == (np.float32(alpha), np.float32(eps))
    for n in (0, 8, 218):
        with pytest.raises(spai.SpaiError) as ex:
            eng.root_noise_draws([1], [0], [n], 0.3)
        assert ex.value.code == -1 and "n_children[0]" in str(ex.value), n
    with pytest.raises(spai.SpaiError) as ex:
        eng.root_noise_draws([1], [0], [7], 0.001)
    assert "alpha" in str(ex.value)
    with pytest.raises(spai.SpaiError):
        engine(spai, 2, noise=(0.3, 2.0))
    eng.set_root_noise(0.3, 0.5)
    eng.trees_create(2)
    with pytest.raises(spai.SpaiError) as ex:                 # a tree listed twice would be mixed twice in one call
        eng.search([1, 1], noise_keys=([0, 1], [0, 0]))
    assert ex.value.code == -1 and "listed twice" in str(ex.value)
    eng.set_root_noise(0.3, 0.0)
    eng.search([1, 1], noise_keys=([0, 1], [0, 0]))           # epsilon 0 is spai_search, which allows it
    eng.close()


# ---- 3. epsilon 0 is the unconfigured engine
def _off_run(spai, pos, kind, configure):
    net = kind == "net"
    eng = engine(spai, 160, sims=12, noise=None, seed=9, kind=spai.EVAL_NET if net else spai.EVAL_HASH)
    if net:
        eng.set_net(spai.Net(eng, 1, spai.init_params(1, seed=3)))
    if configure:
        eng.set_root_noise(0.3, 0.25)   # on, then off again: nothing may linger
        eng.set_root_noise(0.3, 0.0)
    eng.set_timing(True, stride=1)
    games, stats = eng.self_play(160, game_id_base=3, window=130)       # two chains, a refill, the tail
    out = [tuple(g[k].tobytes() for g in sorted(games, key=lambda g: g["game"]) for k in ("enc", "policy", "value", "moves"))]
    out.append(tuple(stats[k] for k in ("sims", "evals", "games", "positions", "moves")))
    out.append(tuple(v["launches"] for v in eng.timing().values()))
    plant(eng, pos)
    trees = np.arange(len(pos), dtype=np.uint32)
    keyed = eng.search(trees, num_searches=12, noise_keys=keys_of(trees))
    out.append(tuple(x.tobytes() for x in keyed))
    out.append(tuple(x.tobytes() for t in trees for x in eng.tree_child_stats(t)))
    plant(eng, pos)
    plain = eng.search(trees, num_searches=12)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keyed, plain))    # spai_search_keyed at epsilon 0 is spai_search
    out.append(tuple(x.tobytes() for t in trees for x in eng.tree_child_stats(t)))
    assert out[-1] == out[-2]
    out.append(tuple(v["launches"] for v in eng.timing().values()))
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_epsilon_zero_is_the_unconfigured_engine(spai, pos, kind):
    a, b = _off_run(spai, pos, kind, False), _off_run(spai, pos, kind, True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, i
    print(kind, "timed launches (select, evaluate, expand):", a[2], a[-1])


# ---- 4. fresh roots
@pytest.fixture(scope="module")
def fresh(spai, pos):
    plain, noisy = engine(spai, NPOS, noise=None), engine(spai, NPOS)
    trees = np.arange(NPOS, dtype=np.uint32)
    nch = np.array([len(s.valid_actions()) for s in pos], np.uint32)
    keys = keys_of(trees)
    eta = draws_for(noisy, trees, keys, nch)
    plant(plain, pos)
    plain.search(trees, num_searches=1)
    prior = [device_record(plain, t) for t in trees]
    ref = NR.noised_search(pos, SIMS, eta=eta, eps=EPS)
    assert ref["mixed"] == list(range(NPOS))
    yield dict(plain=plain, noisy=noisy, trees=trees, nch=nch, keys=keys, eta=eta, prior=prior, ref=ref,
               unnoised=NR.noised_search(pos, SIMS))
    plain.close()
    noisy.close()


def test_fresh_root_priors_are_the_mix(pos, fresh):
    noisy, trees = fresh["noisy"], fresh["trees"]
    plant(noisy, pos)
    noisy.search(trees, num_searches=1, noise_keys=fresh["keys"])
    for t in trees:
        n, w, vis, cw, pr = device_record(noisy, t)
        pn, pw, pvis, pcw, ppr = fresh["prior"][t]
        assert len(pr) == fresh["nch"][t], t
        want = NR.mix(ppr, fresh["eta"][t], EPS)
        assert np.array_equal(bits(pr), bits(want)), (t, int((bits(pr) != bits(want)).sum()))
        assert (n, bits(w)) == (pn, bits(pw)) and n == 1 and not vis.any() and not bits(cw).any(), t
        if len(pr) > 1:
            assert not np.array_equal(bits(pr), bits(ppr)), t          # the noise did something


def _assert_search_is_ref(eng, got, ref, order):
    pol, ids, vis, nc = got
    for i, t in enumerate(order):
        k = int(ref["nc"][t])
        assert nc[i] == k and np.array_equal(vis[i, :k], ref["visits"][t, :k]), (t, vis[i], ref["visits"][t])
        assert pol[i].tobytes() == ref["policy"][t].tobytes(), t
        n, w, cvis, cw, cpr = device_record(eng, t)
        acts, rn, rw, rp = ref["records"][t]
        assert (n, bits(w)) == (ref["roots"][t][0], bits(ref["roots"][t][1])), t
        assert np.array_equal(cvis, rn) and np.array_equal(bits(cw), bits(rw)) and np.array_equal(bits(cpr), bits(rp)), t
        assert np.array_equal(ids[i, :k], ids[i, 0] + np.arange(k)), t


def test_fresh_root_search_is_the_oracles_noised_search(pos, fresh):
    noisy, trees, ref = fresh["noisy"], fresh["trees"], fresh["ref"]
    plant(noisy, pos)
    _assert_search_is_ref(noisy, noisy.search(trees, num_searches=SIMS, noise_keys=fresh["keys"]), ref, trees)
    moved = [t for t in trees if ref["visits"][t].tobytes() != fresh["unnoised"]["visits"][t].tobytes()]
    print(f"trees whose visit counts the noise moved: {len(moved)} of {NPOS}")
    assert moved
    # the same trees in another order (another wave and block each), and two of them alone
    order = np.random.default_rng(4).permutation(NPOS).astype(np.uint32)
    plant(noisy, pos)
    got = noisy.search(order, num_searches=SIMS, noise_keys=(fresh["keys"][0][order], fresh["keys"][1][order]))
    _assert_search_is_ref(noisy, got, ref, order)
    two = np.array([7, 3], np.uint32)
    plant(noisy, pos)
    got = noisy.search(two, num_searches=SIMS, noise_keys=(fresh["keys"][0][two], fresh["keys"][1][two]))
    _assert_search_is_ref(noisy, got, ref, two)
    assert len(noisy.tree_child_stats(0)[0]) == 0          # a tree not searched was not touched


# ---- 9. plain searches and matches never see it
def test_plain_search_and_match_ignore_root_noise(spai, pos, fresh):
    noisy, trees = fresh["noisy"], fresh["trees"]
    plant(noisy, pos)
    _assert_search_is_ref(noisy, noisy.search(trees, num_searches=SIMS), fresh["unnoised"], trees)

    def match(noise):
        eng = engine(spai, 16, sims=8, noise=noise, seed=3)
        games, _ = eng.match((spai.EVAL_HASH, None, 8), (spai.EVAL_UNIFORM, None, 6), n_games=8, seed=2)
        eng.close()
        return [(g["game"], g["result_a"], tuple(g["moves"])) for g in games]

    assert match((ALPHA, 0.5)) == match(None)


# ---- 5. reused roots
def test_reused_roots(spai, pos):
    eps = 0.5
    eng = engine(spai, NPOS, noise=(ALPHA, eps))
    plant(eng, pos)
    trees = np.arange(NPOS, dtype=np.uint32)
    nch = np.array([len(s.valid_actions()) for s in pos], np.uint32)
    k0 = keys_of(trees, 0)
    py = NR.py_search(pos, SIMS, eta=draws_for(eng, trees, k0, nch), eps=eps)
    pol, ids, vis, nc = eng.search(trees, noise_keys=k0)
    live, roots = [], {}
    for t in trees:
        assert_tree_is(eng, t, py[t], "first search")
        k = R.most_visited_last(vis[t], int(nc[t]))
        if py[t].root.children[k].state.status == 0:
            eng.use_subtree(t, ids[t, k])
            py[t].use_subtree(k)
            live.append(int(t))
            roots[int(t)] = int(ids[t, k])
    assert len(live) >= NPOS // 2
    live = np.array(live, np.uint32)
    with_children = [t for t in live if py[t].root.children]
    assert with_children
    before = {t: device_record(eng, t, roots[t]) for t in live}
    for rnd in (1, 2):          # the second keyed search follows without a move: it mixes again
        kk = keys_of(live, rnd)
        eta = draws_for(eng, live, kk, np.array([NR.n_root_children(py[t]) for t in live], np.uint32))
        got = eng.search(live, noise_keys=kk)
        for i, t in enumerate(live):
            if rnd == 1 and py[t].root.children:
                # priors = mix(before, eta): the selections never write them
                assert np.array_equal(bits(eng.tree_child_stats(t)[3]), bits(NR.mix(before[t][4], eta[i], eps))), t
            py[t].search(SIMS, eta[i], eps)
            assert_tree_is(eng, t, py[t], f"reused, call {rnd}", roots[t])
            assert_search_is(got, i, py[t], f"reused, call {rnd}")
    eng.close()


# ---- 6. every launch regime
def _regime(spai, roots, sims, regime):
    n = len(roots)
    eng = engine(spai, n, sims=max(sims, 2))
    eng.set_timing(True, stride=1)
    trees = np.arange(n, dtype=np.uint32)
    nch = np.array([len(s.valid_actions()) for s in roots], np.uint32)
    keys = keys_of(trees)
    eta = draws_for(eng, trees, keys, nch)
    env = TAIL_ENV if regime == "tail" else {}
    os.environ.update(env)
    try:
        plant(eng, roots)
        if regime == "tail":                    # the first call gives the tail policy its statistics
            eng.search(trees, num_searches=2)
            for t, s in enumerate(roots):
                eng.tree_reset(t, R.key_of(s) + (0,))
        before = eng.timing()["select"]["launches"]
        got = eng.search(trees, num_searches=sims, noise_keys=keys)
        launches = eng.timing()["select"]["launches"] - before
    finally:
        for k in env:
            del os.environ[k]
    # tail mode samples no launch; one chain samples sims selects, two chains twice as many
    assert launches == dict(tail=0, one=sims, two=2 * sims, single=1)[regime], (regime, launches)
    good = NR.py_search(roots, sims, eta=eta, eps=EPS)
    for t in trees:
        assert_tree_is(eng, t, good[t], regime)
        assert_search_is(got, t, good[t], regime)
    eng.close()
    if sims > 1:        # the yardstick tells a mix behind the first selection from this one
        late = NR.py_search(roots, sims, eta=eta, eps=EPS, late=True)
        moved = [t for t in trees if late[t].visits().tobytes() != good[t].visits().tobytes()]
        print(f"{regime}: a late mix would change the visit counts of {len(moved)} of {n} trees")
        assert moved, regime


@pytest.mark.parametrize("regime", ["one", "two", "tail", "single"])
def test_launch_regimes(spai, pos, regime):
    roots = R.positions(128, SEED, duplicates=12) if regime == "two" else pos
    _regime(spai, roots, 1 if regime == "single" else REG_SIMS, regime)


# ---- 7. self-play
@pytest.fixture(scope="module")
def selfplay(spai):
    n = 8

    def run(noise=(ALPHA, EPS), seed=21, base=0, games=n, **kw):
        eng = engine(spai, games, noise=noise, seed=seed)
        out, _ = eng.self_play(games, game_id_base=base, **kw)
        eng.close()
        return {g["game"]: g for g in out}

    return dict(n=n, run=run, lock=run())


def test_self_play_is_the_yardsticks(spai, selfplay):
    n = selfplay["n"]
    eng = engine(spai, 1, sims=1, noise=None, seed=21)
    eta_fn = lambda gid, move, k: eng.root_noise_draws([gid], [move], [k], ALPHA)[0, :k]
    ref = NR.py_self_play(n, SIMS, 21, eta_fn=eta_fn, eps=EPS)
    eng.close()
    assert sorted(selfplay["lock"]) == sorted(ref) == list(range(n))
    for g in range(n):
        for k in ("enc", "policy", "value", "moves"):
            assert selfplay["lock"][g][k].tobytes() == ref[g][k].astype(selfplay["lock"][g][k].dtype).tobytes(), (g, k)


def test_self_play_modes_play_the_same_games(selfplay):
    n, run, lock = selfplay["n"], selfplay["run"], selfplay["lock"]
    split = dict(run(games=3))
    split.update(run(base=3, games=n - 3))
    for name, other in (("window 3", run(window=3)), ("game_id_base split", split)):
        assert sorted(other) == list(range(n)), name
        for g in range(n):
            for k in ("enc", "policy", "value", "moves"):
                assert other[g][k].tobytes() == lock[g][k].tobytes(), (name, g, k)


def test_self_play_noise_depends_on_seed_and_can_be_told_from_none(selfplay):
    n, run, lock = selfplay["n"], selfplay["run"], selfplay["lock"]
    other, off = run(seed=22), run(noise=None)
    assert any(other[g]["policy"].tobytes() != lock[g]["policy"].tobytes() for g in range(n))
    # without noise every game's first search is the same search; with it, the keys differ
    assert len({off[g]["policy"][0].tobytes() for g in range(n)}) == 1
    assert len({lock[g]["policy"][0].tobytes() for g in range(n)}) > 1
    assert any(off[g]["moves"].tobytes() != lock[g]["moves"].tobytes() or
               off[g]["policy"].tobytes() != lock[g]["policy"].tobytes() for g in range(n))


# ---- 8. the net and the cache
def test_net_self_play_does_not_depend_on_the_cache(spai):
    params = spai.init_params(1, seed=3)
    runs, keep = {}, None
    for name, cap in (("default", None), ("one bucket", 8), ("off", 0)):
        eng = engine(spai, 16, sims=24, seed=8, kind=spai.EVAL_NET)
        if cap is not None:
            eng.set_eval_cache(cap)
        net = spai.Net(eng, 1, params)
        eng.set_net(net)
        games, _ = eng.self_play(16, window=6)
        runs[name] = {g["game"]: g for g in games}
        cs = eng.eval_cache_stats()
        print(name, "cache hits %.0f of %.0f lookups" % (cs["hits"], cs["lookups"]))
        assert cs["hits"] == 0 if cap == 0 else cap is not None or cs["hits"] > 0, name
        if cap is None:
            keep = (eng, net)
        else:
            eng.close()
    for name in ("one bucket", "off"):
        for g in range(16):
            for k in ("enc", "policy", "value", "moves"):
                assert runs[name][g][k].tobytes() == runs["default"][g][k].tobytes(), (name, g, k)
    # no noised prior reached the cache: with epsilon back at 0, a fresh empty board holds the net's own priors
    eng, net = keep
    eng.set_root_noise(ALPHA, 0.0)
    eng.trees_create(1)
    hits = eng.eval_cache_stats()["hits"]
    eng.search([0], num_searches=1)
    assert eng.eval_cache_stats()["hits"] == hits + 1          # served from the cache the noisy games filled
    pr, _ = net.predict([(0, 0, 0, 0)])
    assert np.array_equal(bits(eng.tree_child_stats(0)[3]), bits(pr[0]))
    eng.close()


# ---- 10. learn
def test_learn_with_root_noise(spai, tmp_path):
    kw = dict(num_learn_iters=2, num_self_play_iters=1, num_parallel_self_play_games=16, batch_size=32, num_epochs=1,
              num_searches=12, blocks=1, seed=4)

    def run(name, noise):
        rec = spai.learn(checkpoint_dir=str(tmp_path / name), root_noise=noise, **kw)
        return [spai.load_params(r["checkpoint"], 1) for r in rec]

    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b"), os.makedirs(tmp_path / "off")
    a, b, off = run("a", (ALPHA, EPS)), run("b", (ALPHA, EPS)), run("off", None)
    assert len(a) == 2
    for i in range(2):
        assert np.array_equal(a[i], b[i]), i                    # reproducible run to run, bit for bit
        assert not np.array_equal(a[i], off[i]), i              # and not the noise-free checkpoints
