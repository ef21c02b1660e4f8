"""The chess search's opt-in Dirichlet root noise on the MI355X: the device sampler
(csrc/dirichlet.h), k_croot_noise at its two launch points, the keyed search and
self-play's keys.

Yardsticks, none of which runs the device code under test:
  dirichlet_stats.check_draws    the draws' distribution (shown fair on the CPU by
                                 tests/test_chess_root_noise_cpu.py)
  chess_noise_ref.mix            spai.h's float32 mix, restated in numpy
  chess_noise_ref.NoisedHashSearch
                                 the oracle's Mcts::search with the hash evaluator
                                 as a callback that mixes the same eta at the roots
  chess_noise_ref.get_ucb        mcts.rs:91-100 in numpy float32, for a root that
                                 kept its subtree (the oracle evaluates no such root)
Everything compared is compared bit for bit; the only statistics are check_draws'.
"""
import numpy as np
import pytest

import chess_noise_ref as NR
import chess_search_ref as R
import dirichlet_stats as DS
from chess_match_ref import abi_from_state

pytestmark = pytest.mark.gpu

ALPHA = 0.3
I218, IONE = R.N_POSITIONS, R.N_POSITIONS + 1   # the two extra positions' indices
NP = R.N_POSITIONS + 2


def load_slots(eng, sc, pos):
    """game slots [0, len(pos)) = the positions: lines applied from the start position (the
    slot holds the history), FEN positions written (empty history)"""
    eng.games_resize(len(pos))
    for i, (seq, fen, s) in enumerate(pos):
        if fen is not None:
            eng.games_write(np.array([abi_from_state(s.st, sc.STATE_DTYPE)], sc.STATE_DTYPE), first=i)
    for p in range(max(len(seq) for seq, _, _ in pos if seq is not None)):
        given = [seq is not None and p < len(seq) for seq, _, _ in pos]
        rc = eng.apply(np.array([seq[p] if g else 0 for g, (seq, _, _) in zip(given, pos)], np.uint16), check=False)
        assert all(rc[i] == 0 for i in range(len(pos)) if given[i]), (p, rc)


def reset(eng, n=NP):
    eng.trees_create(n)
    for t in range(n):
        eng.tree_reset(t, t)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y) for x, y in zip(a, b))


def keys_of(trees, move):
    """the test's keys of these trees: game id 100 + tree, the given move number"""
    t = np.asarray(trees)
    return (100 + t).astype(np.uint64), np.full(len(t), move, np.uint32)


@pytest.fixture(scope="module")
def S():
    import chessref as ch
    import spai_chess as sc
    ch.lib()
    big, one = NR.extra_states()
    pos = R.positions() + [(None, NR.FEN_218, big), (None, NR.FEN_ONE, one)]
    states = [s for _, _, s in pos]
    nch = np.array([len(s.valid_actions()) for s in states], np.uint32)
    assert len(pos) == NP and nch[I218] == 218 and nch[IONE] == 1
    plain = sc.ChessEngine(num_searches=48, max_trees=NP, eval_kind=sc.EVAL_HASH, seed=5)
    noisy = sc.ChessEngine(num_searches=48, max_trees=NP, eval_kind=sc.EVAL_HASH, seed=5, root_noise=(ALPHA, 0.25))
    for e in (plain, noisy):
        load_slots(e, sc, pos)
    d = dict(ch=ch, sc=sc, pos=pos, states=states, nch=nch, plain=plain, noisy=noisy)
    yield d
    ch.arena_reset()
    plain.close()
    noisy.close()


# ---- 1. the draws
@pytest.mark.parametrize("n,alpha", DS.GRID)
def test_draws_are_dirichlet(S, n, alpha):
    N = DS.N_DRAWS
    rng = np.random.default_rng([n, int(alpha * 10)])
    gid = rng.integers(0, 2 ** 63, N, dtype=np.uint64)
    mv = rng.integers(0, 600, N).astype(np.uint32)
    eta = S["plain"].root_noise_draws(gid, mv, np.full(N, n), alpha)
    assert eta.shape == (N, S["sc"].MAX_MOVES) and not eta[:, n:].any()
    m = DS.check_draws(np.ascontiguousarray(eta[:, :n]), alpha)
    print(n, alpha, {k: m[k] for k in ("sum_err", "sum_bound", "z_max", "var_ratio", "ks_p")})


def test_draws_single_child_and_determinism(S):
    eng = S["plain"]
    N = DS.N_DRAWS
    one = eng.root_noise_draws(np.arange(50), np.arange(50) % 7, np.ones(50), ALPHA)
    assert bits(one[:, 0]).tolist() == [0x3F800000] * 50 and not one[:, 1:].any()
    rng = np.random.default_rng(3)
    gid = rng.integers(0, 2 ** 40, N, dtype=np.uint64)
    mv = rng.integers(0, 300, N).astype(np.uint32)
    n = rng.integers(1, 219, N).astype(np.uint32)
    a = eng.root_noise_draws(gid, mv, n, ALPHA)
    b = eng.root_noise_draws(gid, mv, n, ALPHA)
    assert a.tobytes() == b.tobytes()
    # a key's draw alone, in the batch, and at another index of the batch (another wave, block and lane group)
    for i in (0, 1, 4097, N - 1):
        alone = eng.root_noise_draws(gid[i:i + 1], mv[i:i + 1], n[i:i + 1], ALPHA)
        assert alone[0].tobytes() == a[i].tobytes(), i
    perm = rng.permutation(N)
    c = eng.root_noise_draws(gid[perm], mv[perm], n[perm], ALPHA)
    assert c.tobytes() == a[perm].tobytes()
    # another engine of the same seed draws the same, of another seed something else
    sc = S["sc"]
    for seed, equal in ((5, True), (6, False)):
        other = sc.ChessEngine(num_searches=1, max_trees=1, eval_kind=sc.EVAL_HASH, seed=seed)
        o = other.root_noise_draws(gid[:64], mv[:64], n[:64], ALPHA)
        assert (o.tobytes() == a[:64].tobytes()) == equal, seed
        other.close()


def test_draws_of_neighbouring_keys_are_uncorrelated(S):
    eng = S["plain"]
    N, n = DS.N_DRAWS, 20
    g = (2 * np.arange(N) + 11).astype(np.uint64)
    m = (np.arange(N) % 40).astype(np.uint32)
    k = np.full(N, n)
    x = eng.root_noise_draws(g, m, k, ALPHA)[:, 0].astype(np.float64)
    y = eng.root_noise_draws(g, m + 1, k, ALPHA)[:, 0].astype(np.float64)
    z = eng.root_noise_draws(g + 1, m, k, ALPHA)[:, 0].astype(np.float64)
    for name, (p, q) in dict(move=(x, y), game=(x, z), both=(y, z)).items():
        r = float(np.corrcoef(p, q)[0, 1])
        print(f"correlation of component 0 across {name}: {r:+.5f} (bound {5 / np.sqrt(N):.5f})")
        assert abs(r) <= 5 / np.sqrt(N), (name, r)


# ---- 2. validation
def test_validation(S):
    sc = S["sc"]
    eng = sc.ChessEngine(num_searches=4, max_trees=2, eval_kind=sc.EVAL_HASH)
    assert eng.root_noise()[1] == 0.0                      # the default is off
    eng.set_root_noise(0.3, 0.25)
    assert eng.root_noise() == (np.float32(0.3), np.float32(0.25))
    for alpha, eps in ((0.009, 0.25), (100.5, 0.25), (float("nan"), 0.25), (0.3, -0.01), (0.3, 1.01),
                       (0.3, float("nan")), (-1.0, 0.0)):
        with pytest.raises(sc.SpaiError) as ex:
            eng.set_root_noise(alpha, eps)
        assert ex.value.code == -1, (alpha, eps)
        assert eng.root_noise() == (np.float32(0.3), np.float32(0.25))   # a refused call changes nothing
    for alpha, eps in ((0.01, 0.0), (100.0, 1.0)):
        eng.set_root_noise(alpha, eps)
        assert eng.root_noise() == (np.float32(alpha), np.float32(eps))
    for n in (0, 219, 256):
        with pytest.raises(sc.SpaiError) as ex:
            eng.root_noise_draws([1], [0], [n], 0.3)
        assert ex.value.code == -1, n
    with pytest.raises(sc.SpaiError):
        eng.root_noise_draws([1], [0], [20], 0.001)
    with pytest.raises(sc.SpaiError):
        sc.ChessEngine(num_searches=4, max_trees=2, eval_kind=sc.EVAL_HASH, root_noise=(0.3, 2.0))
    eng.set_root_noise(0.3, 0.5)
    eng.trees_create(2)
    with pytest.raises(sc.SpaiError):                      # a tree listed twice would be mixed twice in one call
        eng.search([1, 1], noise_keys=([0, 1], [0, 0]))
    eng.close()


# ---- 3. off means off
def _off_runs(sc, pos, make):
    """what an engine returns from a keyed search, a plain search and self-play, as comparable tuples"""
    eng, net = make()
    load_slots(eng, sc, pos)
    reset(eng, len(pos))
    trees = np.arange(len(pos), dtype=np.uint32)
    out = [eng.search(trees, num_searches=6, noise_keys=keys_of(trees, 2))]
    out.append(tuple(x for t in trees for x in eng.tree_child_stats(t)))
    eng.advance(trees[:4], [0, 1, 0, 1])
    out.append(eng.search(trees, num_searches=6))
    out.append(eng.search(trees, num_searches=5, noise_keys=keys_of(trees, 3)))
    out.append(tuple(x for t in trees for x in eng.tree_child_stats(t)))
    games, _ = eng.self_play(2, game_id_base=3)
    out.append(tuple(g[k] for g in sorted(games, key=lambda g: g["game"]) for k in ("enc", "policy", "value", "moves")))
    if net is not None:
        net.close()
    eng.close()
    return out


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_epsilon_zero_is_the_unconfigured_engine(S, kind):
    sc, pos = S["sc"], S["pos"][:8] + S["pos"][-2:]

    def make(configure):
        def f():
            eng = sc.ChessEngine(num_searches=6, max_trees=len(pos), seed=9, max_moves=2048,
                                 eval_kind=sc.EVAL_HASH if kind == "hash" else sc.EVAL_NET)
            net = None
            if kind == "net":
                net = sc.ChessNet(eng, 1, sc.init_params(1, 5))
                eng.set_net(net)
            if configure:
                eng.set_root_noise(0.3, 0.25)   # on, then off again: nothing may linger
                eng.set_root_noise(0.3, 0.0)
            return eng, net
        return f

    a, b = _off_runs(sc, pos, make(False)), _off_runs(sc, pos, make(True))
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same(x, y), i


# ---- 4. fresh roots, exact
@pytest.fixture(scope="module")
def fresh(S):
    """the keys, the draws, the plain priors and the oracle's noised search of the 26 fresh roots"""
    plain, noisy, nch = S["plain"], S["noisy"], S["nch"]
    trees = np.arange(NP, dtype=np.uint32)
    gid, _ = keys_of(trees, 0)
    mv = (trees % 5).astype(np.uint32)
    eta = noisy.root_noise_draws(gid, mv, nch)
    reset(plain)
    plain.search(trees, num_searches=1)
    prior = [plain.tree_child_stats(t) for t in trees]
    root = [plain.tree_root(t)[1:] for t in trees]
    ref =NR.noised_hash_search(S["states"], 48, eta=[eta[t, :nch[t]] for t in trees], eps=0.25)
    assert ref["mixed"] == list(range(NP))
    unnoised = NR.noised_hash_search(S["states"], 48)
    return dict(trees=trees, gid=gid, mv=mv, eta=eta, prior=prior, root=root, ref=ref, unnoised=unnoised)


def test_fresh_root_priors_are_the_mix(S, fresh):
    noisy, nch = S["noisy"], S["nch"]
    trees = fresh["trees"]
    reset(noisy)
    noisy.search(trees, num_searches=1, noise_keys=(fresh["gid"], fresh["mv"]))
    for t in trees:
        mv, vis, w, pr = noisy.tree_child_stats(t)
        pmv, pvis, pw, ppr = fresh["prior"][t]
        assert len(pr) == nch[t] and np.array_equal(mv, pmv), t
        want = NR.mix(ppr, fresh["eta"][t, :nch[t]], 0.25)
        assert np.array_equal(bits(pr), bits(want)), (t, int((bits(pr) != bits(want)).sum()))
        assert np.array_equal(vis, pvis) and np.array_equal(bits(w), bits(pw)), t
        assert noisy.tree_root(t)[1:] == fresh["root"][t], t
        if nch[t] > 1:
            assert not np.array_equal(bits(pr), bits(ppr)), t          # the noise did something


def _assert_search_is_ref(got, ref, trees):
    pol, ids, vis, mv, nc = got
    for i, t in enumerate(trees):
        k = int(nc[i])
        assert k == ref["nc"][t], t
        assert np.array_equal(mv[i, :k], ref["moves"][t, :k].astype(np.uint16)), t
        assert np.array_equal(vis[i, :k], ref["visits"][t, :k]), (t, vis[i, :k], ref["visits"][t, :k])
        assert pol[i].tobytes() == ref["policy"][t].tobytes(), t


def test_fresh_root_search_is_the_oracles_noised_search(S, fresh):
    noisy, trees, ref = S["noisy"], fresh["trees"], fresh["ref"]
    reset(noisy)
    got = noisy.search(trees, num_searches=48, noise_keys=(fresh["gid"], fresh["mv"]))
    _assert_search_is_ref(got, ref, trees)
    moved = [t for t in trees if R.visit_table(ref)[t] != R.visit_table(fresh["unnoised"])[t]]
    print(f"trees whose visit table the noise moved: {len(moved)} of {NP}")
    assert moved
    # the same trees in another order (another wave, block and key slot each), and two of them alone
    order = np.random.default_rng(4).permutation(NP).astype(np.uint32)
    reset(noisy)
    got = noisy.search(order, num_searches=48, noise_keys=(fresh["gid"][order], fresh["mv"][order]))
    _assert_search_is_ref(got, ref, order)
    two = np.array([I218, 3], np.uint32)
    reset(noisy)
    got = noisy.search(two, num_searches=48, noise_keys=(fresh["gid"][two], fresh["mv"][two]))
    _assert_search_is_ref(got, ref, two)
    # the trees not searched were not touched
    assert len(noisy.tree_child_stats(IONE)[0]) == 0 and noisy.tree_root(IONE)[1] == 0


def test_plain_search_on_a_noisy_engine_has_no_noise(S, fresh):
    noisy, trees = S["noisy"], fresh["trees"]
    reset(noisy)
    got = noisy.search(trees, num_searches=48)
    _assert_search_is_ref(got, fresh["unnoised"], trees)


# ---- 5. roots that kept their subtree
def test_reused_roots(S):
    sc, nch0 = S["sc"], S["nch"]
    eps = 0.5
    eng = sc.ChessEngine(num_searches=48, max_trees=NP, eval_kind=sc.EVAL_HASH, seed=5, root_noise=(ALPHA, eps))
    load_slots(eng, sc, S["pos"])
    reset(eng)
    trees = np.arange(NP, dtype=np.uint32)
    first = eng.search(trees, num_searches=48, noise_keys=(trees, np.zeros(NP, np.uint32)))
    picks = [R.most_visited_last(first[2][t], first[4][t]) for t in trees]
    status, _ = eng.advance(trees, picks)
    before = [eng.tree_child_stats(t) for t in trees]
    root_n = [eng.tree_root(t)[1] for t in trees]
    live = np.array([t for t in trees if status[t] == 0 and len(before[t][0]) > 0], np.uint32)
    assert len(live) >= NP // 2, (status, [len(b[0]) for b in before])
    n_live = np.array([len(before[t][0]) for t in live], np.uint32)
    eta = eng.root_noise_draws(live, np.ones(len(live)), n_live)
    eng.search(live, num_searches=1, noise_keys=(live, np.ones(len(live), np.uint32)))
    differ = []
    for i, t in enumerate(live):
        mv, vis, w, pr = eng.tree_child_stats(t)
        bmv, bvis, bw, bpr = before[t]
        assert np.array_equal(mv, bmv), t
        want = NR.mix(bpr, eta[i, :n_live[i]], eps)
        assert np.array_equal(bits(pr), bits(want)), (t, int((bits(pr) != bits(want)).sum()))
        gain = vis.astype(np.int64) - bvis.astype(np.int64)
        assert gain.min() == 0 and gain.sum() == 1, (t, gain)
        chosen = int(np.argmax(gain))
        assert chosen == NR.last_argmax(NR.get_ucb(root_n[t], bvis, bw, want)), t
        if chosen != NR.last_argmax(NR.get_ucb(root_n[t], bvis, bw, bpr)):
            differ.append(int(t))
        assert eng.tree_root(t)[1] == root_n[t] + 1, t
    print(f"reused roots whose first selection the noise (eps {eps}) changed: {len(differ)} of {len(live)}: {differ}")
    assert len(differ) >= 1
    eng.search(live, num_searches=47, noise_keys=(live, np.ones(len(live), np.uint32)))
    for t in live:
        mv, vis, w, pr = eng.tree_child_stats(t)
        assert eng.tree_root(t)[1] == root_n[t] + 48, t
        assert int(vis.sum()) == root_n[t] + 48 - 1, t
    eng.close()


def test_reused_root_after_compaction(S):
    """an engine whose arena half fills within a few dozen plies: in the call that compacts,
    k_croot_noise runs behind k_ccompact and mixes the children where they now stand"""
    sc = S["sc"]
    sims, eps = 17, 0.5
    eng = sc.ChessEngine(num_searches=sims, max_trees=1, eval_kind=sc.EVAL_HASH, seed=5, root_noise=(ALPHA, eps))
    eng.trees_create(1)
    compacted_at = None
    for ply in range(120):
        before = eng.tree_child_stats(0)
        root_n = eng.tree_root(0)[1]
        pol, ids, vis, mv, nc = eng.search([0], num_searches=sims, noise_keys=([9], [ply]))
        # the root's children stand right behind it only in a fresh tree or after a copy
        if ply > 0 and ids[0, 0] == 1 and compacted_at is None:
            compacted_at = ply
        after = eng.tree_child_stats(0)
        if len(before[0]):
            n = len(before[0])
            eta = eng.root_noise_draws([9], [ply], [n])
            want = NR.mix(before[3], eta[0, :n], eps)
            assert np.array_equal(after[0], before[0]), ply
            assert np.array_equal(bits(after[3]), bits(want)), (ply, compacted_at)
            assert eng.tree_root(0)[1] == root_n + sims and int(after[1].sum()) == root_n + sims - 1, ply
        if compacted_at is not None:
            break
        st, _ = eng.advance([0], [R.most_visited_last(after[1], len(after[1]))])
        assert st[0] == 0, ply
    assert compacted_at is not None
    eng.close()


# ---- 6. the net path
def test_net_root_priors_are_the_mix_of_predict(S):
    sc, nch, states = S["sc"], S["nch"], S["states"]
    eps = 0.25
    eng = sc.ChessEngine(num_searches=4, max_trees=NP, eval_kind=sc.EVAL_NET, seed=5, root_noise=(ALPHA, eps))
    net = sc.ChessNet(eng, 1, sc.init_params(1, 5))
    eng.set_net(net)
    load_slots(eng, sc, S["pos"])
    pred, _ = net.predict(NP)
    reset(eng)
    trees = np.arange(NP, dtype=np.uint32)
    gid, mv = keys_of(trees, 7)
    eta = eng.root_noise_draws(gid, mv, nch)
    eng.search(trees, num_searches=1, noise_keys=(gid, mv))
    for t in trees:
        moves, vis, w, pr = eng.tree_child_stats(t)
        idx = [sc.move_index(states[t].side, m) for m in states[t].valid_actions()]
        assert list(moves) == states[t].valid_actions(), t
        want = NR.mix(pred[t][idx], eta[t, :nch[t]], eps)
        assert np.array_equal(bits(pr), bits(want)), (t, int((bits(pr) != bits(want)).sum()))
    net.close()
    eng.close()


# ---- 7. self-play
@pytest.fixture(scope="module")
def selfplay(S):
    sc = S["sc"]
    n, sims = 4, 16

    def run(noise, **kw):
        eng = sc.ChessEngine(num_searches=sims, max_trees=n, eval_kind=sc.EVAL_HASH, seed=21, max_moves=2048,
                             root_noise=noise)
        games, stats = eng.self_play(n, **kw)
        eng.close()
        return {g["game"]: g for g in games}, stats

    noise = (ALPHA, 0.25)
    return dict(n=n, sims=sims, noise=noise, lock=run(noise)[0], stream=run(noise, window=2)[0],
                compact=run(noise, samples="compact")[0], base7=run(noise, game_id_base=7)[0], off=run(None)[0])


def test_self_play_plies_are_keyed_searches(S, selfplay):
    sc, n, sims = S["sc"], selfplay["n"], selfplay["sims"]
    for base, games in ((0, selfplay["lock"]), (7, selfplay["base7"])):
        eng = sc.ChessEngine(num_searches=sims, max_trees=n, eval_kind=sc.EVAL_HASH, seed=21, max_moves=2048,
                             root_noise=selfplay["noise"])
        eng.trees_create(n)
        live = list(range(n))
        for ply in range(8):
            live = [g for g in live if games[base + g]["n"] > ply]
            if not live:
                break
            t = np.array(live, np.uint32)
            pol, ids, vis, mv, nc = eng.search(t, noise_keys=(base + t.astype(np.uint64), np.full(len(t), ply)))
            picks = []
            for i, g in enumerate(live):
                assert pol[i].tobytes() == games[base + g]["policy"][ply].tobytes(), (base, g, ply)
                played = int(games[base + g]["moves"][ply])
                picks.append(int(np.flatnonzero(mv[i, :nc[i]] == played)[0]))
            eng.advance(t, picks)
        assert ply >= 1
        eng.close()


def test_self_play_modes_play_the_same_games(selfplay):
    lock, n = selfplay["lock"], selfplay["n"]
    assert sorted(lock) == sorted(selfplay["stream"]) == sorted(selfplay["compact"]) == list(range(n))
    for g in range(n):
        a, b = lock[g], selfplay["stream"][g]
        assert a["n"] == b["n"], g
        for k in ("enc", "policy", "value", "moves"):
            assert a[k].tobytes() == b[k].tobytes(), (g, k)
        enc, pol, val = selfplay["compact"][g]["samples"].expand()
        assert enc.tobytes() == a["enc"].tobytes() and pol.tobytes() == a["policy"].tobytes(), g
        assert val.tobytes() == a["value"].tobytes(), g
        assert np.array_equal(selfplay["compact"][g]["samples"].samples["move"], a["moves"]), g


def test_self_play_noise_depends_on_game_id_and_can_be_told_from_none(selfplay):
    lock, n = selfplay["lock"], selfplay["n"]
    assert sorted(selfplay["base7"]) == list(range(7, 7 + n))
    # base 7's game 7 + g shares nothing with base 0's game g but the start position
    assert any(selfplay["base7"][7 + g]["policy"][0].tobytes() != lock[g]["policy"][0].tobytes() for g in range(n))
    # without noise every game's first search is the same search; with it, the keys differ
    off = selfplay["off"]
    assert len({off[g]["policy"][0].tobytes() for g in range(n)}) == 1
    assert len({lock[g]["policy"][0].tobytes() for g in range(n)}) > 1
    assert any(off[g]["moves"].tobytes() != lock[g]["moves"].tobytes() or
               off[g]["policy"].tobytes() != lock[g]["policy"].tobytes() for g in range(n))


# ---- 8. matches never see it
def test_matches_ignore_root_noise(S):
    sc = S["sc"]

    def run(noise):
        eng = sc.ChessEngine(num_searches=8, max_trees=8, eval_kind=sc.EVAL_HASH, seed=3, root_noise=noise)
        players = ((sc.EVAL_HASH, None, 8), (sc.EVAL_UNIFORM, None, 6))
        games, _ = eng.match(*players, n_games=4, max_plies=24, seed=2)
        eng.close()
        return [(g["game"], g["result_a"], g["n_moves"], g["moves"].tobytes()) for g in games]

    assert run((ALPHA, 0.5)) == run(None)
