"""GPU parity tests: the HIP path (libspai.so via its C ABI) against the CPU
oracle and the golden fixtures.  Run on the MI355X box: pytest -m gpu.

Bars: rules, search and self-play with the deterministic stub evaluators are
bit-exact; the bf16 net is compared with libtorch fp32 / the fp32 oracle at the
tolerances stated in each test.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from learner_checks import check_grads_same_masks as _check_grads_same_masks   # shared with test_learner_shapes_gpu.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def eng(spai):
    e = spai.Engine(num_searches=64, max_trees=512, eval_kind=spai.EVAL_HASH, seed=7)
    yield e
    e.close()


def _random_games(n, plies, seed):
    """random action sequences (may contain illegal moves, which must be reported)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 7, size=(n, plies)).astype(np.int32)


# ------------------------------------------------------------------ rules
def test_rules_lockstep_random_games(spai, oracle):
    """1M+ positions: play 32768 random legal games in lockstep on the GPU and
    compare every ply's legal mask / status / bitboards with the oracle."""
    n, P = 32768, 42
    e = spai.Engine(num_searches=1, max_trees=1, eval_kind=spai.EVAL_HASH)
    e.games_resize(n)
    rng = np.random.default_rng(0)
    acts = np.full((n, P), -1, np.int32)
    legal_hist, status_hist, x_hist, o_hist = [], [], [], []
    alive = np.ones(n, bool)
    for p in range(P + 1):
        lm = e.legal_mask(n)
        st = e.games_read(n)
        v, t = e.value_terminated(n)
        legal_hist.append(lm)
        status_hist.append(st["status"].copy())
        x_hist.append(st["x"].copy())
        o_hist.append(st["o"].copy())
        assert np.array_equal(t.astype(bool), st["status"] != 0)
        assert np.all(v[st["status"] == spai.WON] == -1.0) and np.all(v[st["status"] != spai.WON] == 0.0)
        if p == P:
            break
        alive &= lm != 0
        # pick a random legal column per live game
        r = rng.random((n, 7)) * ((lm[:, None] >> np.arange(7)) & 1)
        a = np.where(alive, np.argmax(r, axis=1), 0).astype(np.int32)
        acts[alive, p] = a[alive]
        rc = e.apply(a, check=False)
        assert np.all(rc[alive] == 0)
        assert np.all(rc[~alive] == -3)  # Game has already ended
    ref = oracle.c4_replay(acts)
    for p in range(P + 1):
        live = np.array([True] * n)
        np.testing.assert_array_equal(legal_hist[p][live], ref["legal"][:, p][live])
        np.testing.assert_array_equal(status_hist[p], ref["status"][:, p])
        np.testing.assert_array_equal(x_hist[p], ref["x"][:, p])
        np.testing.assert_array_equal(o_hist[p], ref["o"][:, p])
    e.close()


def test_rules_subranges_and_encoding_vs_oracle(spai, oracle):
    """Slot sub-ranges at every alignment (the 4-games-per-lane kernels take
    ranges starting at a multiple of 4, the scalar ones the rest; tails of 1-3
    games) and the LDS-staged encoder against the oracle's get_encoding."""
    n = 203
    e = spai.Engine(num_searches=1, max_trees=1)
    e.games_resize(n)
    rng = np.random.default_rng(3)
    for p in range(rng.integers(5, 30)):
        lm = e.legal_mask(n)
        r = rng.random((n, 7)) * ((lm[:, None] >> np.arange(7)) & 1)
        e.apply(np.argmax(r, axis=1).astype(np.int32), check=False)
    snap = e.games_read(n)
    states = [_oracle_state(oracle, int(g["x"]), int(g["o"]), int(g["n"]), int(g["status"])) for g in snap]
    enc = e.encode(n)
    lm = e.legal_mask(n)
    for i, s in enumerate(states):
        assert np.array_equal(enc[i], s.encoding()), i
        assert lm[i] == s.legal_mask(), i
    acts = rng.integers(-1, 8, n).astype(np.int32)
    for first in (0, 1, 2, 3, 4, 5, 8):
        for cnt in (1, 3, 4, 7, 64, 65, 130):
            if first + cnt > n:
                continue
            e.games_write(snap)
            assert np.array_equal(e.legal_mask(cnt, first), lm[first:first + cnt])
            assert np.array_equal(e.encode(cnt, first), enc[first:first + cnt])
            rc = e.apply(acts[first:first + cnt], first=first, check=False)
            after = e.games_read(n)
            for k in range(n):
                if first <= k < first + cnt:
                    a = int(acts[k])
                    s = states[k]
                    if s.status != 0:
                        assert rc[k - first] == -3
                        exp = snap[k]
                    elif not 0 <= a < 7:
                        assert rc[k - first] == -1
                        exp = snap[k]
                    elif not (s.legal_mask() >> a) & 1:
                        assert rc[k - first] == -2
                        exp = snap[k]
                    else:
                        assert rc[k - first] == 0
                        t = s.next_state(a)
                        exp = _c4_record(spai, t)
                    assert after[k].tobytes() == exp.tobytes(), (first, cnt, k)
                else:
                    assert after[k].tobytes() == snap[k].tobytes(), (first, cnt, k)
    e.close()


def _c4_record(spai, s):
    x = o = 0
    for col in range(7):
        for row in range(6):
            b = 1 << (col * 7 + row)
            if s.st.board[row][col] == 1:
                x |= b
            elif s.st.board[row][col] == 2:
                o |= b
    return spai.states_array([(x, o, s.n, s.status)])[0]


def test_rules_encode_mask_and_errors(spai, oracle):
    with open(os.path.join(GOLDEN, "rules_c4.json")) as f:
        traces = json.load(f)["traces"]
    states, refs = [], []
    for g in traces[:80]:
        for p in g["plies"]:
            states.append((int(p["x"]), int(p["o"]), p["n"], p["status"]))
            refs.append(p)
    n = len(states)
    e = spai.Engine(num_searches=1, max_trees=1, eval_kind=spai.EVAL_HASH)
    e.games_resize(n)
    e.games_write(states)
    enc = e.encode(n)
    lm = e.legal_mask(n)
    for i, p in enumerate(refs):
        assert float(enc[i].ravel() @ np.arange(126)) == p["enc_sum"]
        assert lm[i] == p["legal"]
    rng = np.random.default_rng(1)
    pol = rng.random((n, 7)).astype(np.float32)
    got = e.mask_invalid(pol)
    for i, (x, o, nn, st) in enumerate(states[:300]):
        s = _oracle_state(oracle, x, o, nn, st)
        if st == 0:
            np.testing.assert_array_equal(got[i], s.mask_invalid(pol[i]))
    with pytest.raises(spai.SpaiError):
        e.mask_invalid(np.ones((n, 6), np.float32))
    # full column -> ILLEGAL_MOVE, slot unchanged
    e.games_resize(1)
    for _ in range(6):
        e.apply([3])
    before = e.games_read(1)
    rc = e.apply([3], check=False)
    assert rc[0] == -2
    assert e.games_read(1).tobytes() == before.tobytes()
    # out-of-range action -> INVALID
    assert e.apply([7], check=False)[0] == -1
    e.close()


def test_rules_kernels_bench_runs(spai):
    e = spai.Engine(num_searches=1, max_trees=1)
    ms = e.rules_bench(1 << 20, iters=3)
    assert np.all(ms > 0)
    e.close()


# ------------------------------------------------------------------ net
BF16_TOL = dict(rtol=3e-2, atol=3e-2)   # bf16 weights/activations, fp32 accumulate


def test_net_forward_vs_libtorch_golden(spai):
    z = np.load(os.path.join(GOLDEN, "net_c4_2x64.npz"))
    blocks, hidden, seed = [int(v) for v in z["meta"]]
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, blocks, z["params"])
    lg, v = net.forward(z["x"])
    scale = np.abs(z["logits"]).max()
    assert np.abs(lg - z["logits"]).max() <= 3e-2 * max(1.0, scale), np.abs(lg - z["logits"]).max()
    np.testing.assert_allclose(v, z["value"], **BF16_TOL)
    # Model::predict: softmax -> mask -> renormalise (model/mod.rs:62-93)
    b = z["boards"]
    states = [(int(b[i, 0]), int(b[i, 1]), int(b[i, 2]), 0) for i in range(len(b))]
    pr, pv = net.predict(states)
    np.testing.assert_allclose(pr, z["priors"], rtol=0, atol=2e-2)
    np.testing.assert_allclose(pr.sum(1), 1.0, atol=1e-5)
    np.testing.assert_allclose(pv, z["value"], **BF16_TOL)
    legal = np.array([[(~(x | o) >> (7 * a + 5)) & 1 for a in range(7)] for x, o, _, _ in states])
    assert np.all(pr[legal == 0] == 0.0)
    net.close()
    e.close()


def test_net_6x64_vs_oracle_fp32(spai, oracle):
    p = spai.init_params(6, 64, seed=0)
    np.testing.assert_array_equal(p, oracle.init_params(1, 6, 64, 0))  # same init stream
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, 6, p)
    rng = np.random.default_rng(3)
    acts = rng.integers(0, 7, size=(48, 20)).astype(np.int32)
    ref = oracle.c4_replay(acts)
    xs = []
    for g in range(48):
        for ply in (0, 5, 11, 19):
            if ref["status"][g, ply] == 0:
                xs.append(_oracle_state(oracle, int(ref["x"][g, ply]), int(ref["o"][g, ply]), ply, 0).encoding())
    x = np.stack(xs)
    on = oracle.Net(1, 6, 64, p)
    rl, rv = on.forward(x)
    lg, v = net.forward(x)
    err = np.abs(lg - rl).max() / max(1.0, np.abs(rl).max())
    assert err < 3e-2, err
    np.testing.assert_allclose(v, rv, rtol=5e-2, atol=5e-2)
    net.close()
    e.close()


def test_net_partial_batches(spai):
    """batch sizes that are not multiples of the 8-position workgroup tile"""
    z = np.load(os.path.join(GOLDEN, "net_c4_2x64.npz"))
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, 2, z["params"])
    full_l, full_v = net.forward(z["x"])
    for n in (1, 3, 8, 9, 17, 255):
        lg, v = net.forward(z["x"][:n])
        np.testing.assert_array_equal(lg, full_l[:n])   # per-position results are batch independent
        np.testing.assert_array_equal(v, full_v[:n])
    net.close()
    e.close()


def _reachable_positions(spai, n, plies, seed):
    """ongoing positions after up to `plies` random legal moves (device rules)"""
    e = spai.Engine(num_searches=1, max_trees=1)
    rng = np.random.default_rng(seed)
    e.games_resize(n)
    for _ in range(plies):
        lm = e.legal_mask(n)
        r = rng.random((n, 7)) * ((lm[:, None] >> np.arange(7)) & 1)
        e.apply(np.argmax(r, 1).astype(np.int32), check=False)
    st = e.games_read(n)
    e.close()
    return [tuple(int(v) for v in (r["x"], r["o"], r["n"], r["status"])) for r in st if r["status"] == 0]


def test_net_group_size_invariance(spai):
    """the persistent forward picks 1..8 positions per workgroup group from the
    batch size (and three task orders with it); a position's priors and value
    must not depend on which group size or slot it ran in"""
    states = _reachable_positions(spai, 2600, 14, seed=9)
    assert len(states) > 2100
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, 6, spai.init_params(6, 64, seed=2))
    full_p, full_v = net.predict(states[:2100])      # 2 rounds of S = 5 on 256 CUs
    for n in (1, 40, 300, 700, 1000, 1300, 1500, 1700, 1800, 2048):   # S = 1..8
        p, v = net.predict(states[:n])
        np.testing.assert_array_equal(p, full_p[:n])
        np.testing.assert_array_equal(v, full_v[:n])
    p, v = net.predict(states[1000:1003])            # other slots than in the full batch
    np.testing.assert_array_equal(p, full_p[1000:1003])
    np.testing.assert_array_equal(v, full_v[1000:1003])
    net.close()
    e.close()


# ------------------------------------------------------------------ search
def test_search_chain_split_invariance(spai):
    """NET search over 200 trees runs as two chains (two streams, two batches);
    the same first 100 trees searched alone run as one chain and must get
    bit-identical visit counts"""
    roots = _reachable_positions(spai, 260, 6, seed=4)[:200]
    assert len(roots) == 200
    params = spai.init_params(6, 64, seed=5)
    out = []
    for n in (200, 100):
        e = spai.Engine(num_searches=64, max_trees=n, eval_kind=spai.EVAL_NET, max_moves=2)
        net = spai.Net(e, 6, params)
        e.set_net(net)
        e.trees_create(n)
        for i in range(n):
            e.tree_reset(i, roots[i])
        out.append(e.search(np.arange(n), 64))
        net.close()
        e.close()
    (pa, ia, va, na), (pb, ib, vb, nb) = out
    np.testing.assert_array_equal(na[:100], nb)
    np.testing.assert_array_equal(va[:100], vb)
    np.testing.assert_array_equal(pa[:100], pb)


def test_search_hash_matches_oracle(spai, oracle, eng):
    d = json.load(open(os.path.join(GOLDEN, "mcts_hash.json")))
    cases = d["search"]
    eng.trees_create(len(cases))
    for i, c in enumerate(cases):
        eng.tree_reset(i, (int(c["x"]), int(c["o"]), c["n"], 0))
    for i, c in enumerate(cases):
        pol, ids, vis, nc = eng.search([i], c["sims"])
        assert [int(v) for v in vis[0, :nc[0]]] == c["visits"], (i, c)
        np.testing.assert_array_equal(pol[0], np.array(c["policy"], np.float32))


def test_search_uniform_first_select(spai):
    e = spai.Engine(num_searches=2, max_trees=4, eval_kind=spai.EVAL_UNIFORM)
    e.trees_create(1)
    pol, ids, vis, nc = e.search([0], 2)
    assert list(vis[0, :nc[0]]) == [0, 0, 0, 0, 0, 0, 1]   # ties -> last child (column 6)
    e.close()


def test_search_batched_with_subtree_reuse(spai, oracle):
    """many trees searched together (two search chains), then re-rooted (use_subtree
    keeps N, W) and searched again"""
    n, sims = 160, 48
    rng = np.random.default_rng(5)
    roots = []
    for g in range(n):
        s = oracle.C4()
        for _ in range(int(rng.integers(0, 14))):
            va = s.valid_actions()
            if not va:
                break
            nx = s.next_state(int(rng.choice(va)))
            if nx.status != 0:
                break
            s = nx
        roots.append(s)
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, max_moves=4)
    e.trees_create(n)
    for i, s in enumerate(roots):
        x, o = s.bitboards()
        e.tree_reset(i, (x, o, s.n, 0))
    L = oracle.lib()
    trees = [L.or_tree_with_root(oracle.GAME_CONNECT4, oracle.C.byref(s.st)) for s in roots]
    for rnd in range(3):
        idx = np.arange(n)
        pol, ids, vis, nc = e.search(idx, sims)
        rc, rp, rids, rvis, rnc = oracle.search_c4(None, sims, trees=trees)
        np.testing.assert_array_equal(nc, rnc)
        np.testing.assert_array_equal(vis, rvis)
        np.testing.assert_array_equal(pol, rp)
        # re-root on the most visited non-terminal child (last max)
        for i in range(n):
            k = int(nc[i])
            if k == 0:
                continue
            j = int(np.flatnonzero(vis[i, :k] == vis[i, :k].max())[-1])
            st = oracle.C4(oracle.C4State.from_buffer_copy(
                oracle.C.string_at(L.or_tree_node_state(trees[i], int(rids[i, j])), oracle.C.sizeof(oracle.C4State))))
            if st.status != 0:
                continue
            e.use_subtree(i, ids[i, j])
            L.or_tree_use_subtree(trees[i], int(rids[i, j]))
            gs, gvis, gw = e.tree_node(i, ids[i, j])
            x, o = st.bitboards()
            assert (int(gs["x"]), int(gs["o"]), int(gs["n"])) == (x, o, st.n)
    for t in trees:
        L.or_tree_destroy(t)
    e.close()


# ------------------------------------------------------------------ self-play
def test_self_play_hash_matches_oracle(spai, oracle):
    # 160 games: the search runs as two chains (>= 128 active trees) until
    # enough games finish, then as one, all checked bit-exactly
    n, sims, seed = 160, 32, 11
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, seed=seed)
    games, stats = e.self_play(n)
    ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42)
    # same emission order: game by game as the reference removes finished trees
    k = 0
    for g in games:
        m = len(g["value"])
        assert list(ref["game"][k:k + m]) == [g["game"]] * m
        np.testing.assert_array_equal(g["policy"], ref["policy"][k:k + m])
        np.testing.assert_array_equal(g["value"], ref["value"][k:k + m])
        np.testing.assert_array_equal(g["enc"], ref["enc"][k:k + m])
        assert list(g["moves"]) == list(ref["moves"][g["game"], :m])
        k += m
    assert k == len(ref["value"])
    assert stats["games"] == n and stats["sims"] == ref["sims"]
    e.close()


@pytest.mark.parametrize("temperature", [0.7, 3.0])
def test_self_play_device_sampling_matches_oracle(spai, oracle, temperature):
    """the move step on the device (selfplay.hip k_advance: Philox uniform,
    WeightedIndex over the std::pow table of visits^T, the new root written in
    place): at temperatures other than the default, and for a second run on the
    same engine (the table reused) at another game-id base, the sample stream is
    the oracle's bit for bit"""
    n, sims, seed = 72, 24, 5
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, seed=seed, temperature=temperature)
    for base in (0, 1000):
        games, stats = e.self_play(n, game_id_base=base)
        ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42,
                               temperature=temperature, game_id_base=base)
        k = 0
        for g in games:   # (the oracle numbers its games from 0, the engine from the base)
            m = len(g["value"])
            assert [int(v) + base for v in ref["game"][k:k + m]] == [g["game"]] * m
            np.testing.assert_array_equal(g["policy"], ref["policy"][k:k + m])
            np.testing.assert_array_equal(g["value"], ref["value"][k:k + m])
            np.testing.assert_array_equal(g["enc"], ref["enc"][k:k + m])
            k += m
        assert k == len(ref["value"]) and stats["sims"] == ref["sims"] and stats["games"] == n
    e.close()


@pytest.mark.parametrize("temperature,window", [(0.7, 29), (3.0, 50)])
def test_self_play_stream_temperature_matches_oracle(spai, oracle, temperature, window):
    """spai_selfplay_stream at temperatures other than the default, twice on the
    same engine (the visits^T table reused; a second game-id base): each game is
    the oracle's lockstep game of the same id bit for bit"""
    n, sims, seed = 72, 24, 5
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, seed=seed, temperature=temperature)
    for base in (0, 1000):
        games, stats = e.self_play(n, game_id_base=base, window=window)
        ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42,
                               temperature=temperature, game_id_base=base)
        assert sorted(g["game"] for g in games) == list(range(base, base + n))
        for g in games:
            rows = np.nonzero(ref["game"] + base == g["game"])[0]
            k, m = int(rows[0]), len(rows)
            assert m == len(g["value"]) and np.all(np.diff(rows) == 1)
            np.testing.assert_array_equal(g["policy"], ref["policy"][k:k + m])
            np.testing.assert_array_equal(g["value"], ref["value"][k:k + m])
            np.testing.assert_array_equal(g["enc"], ref["enc"][k:k + m])
        assert stats["sims"] == ref["sims"] and stats["games"] == n
    e.close()


kTailChunk = 4   # search_internal.h: passes per host check


@pytest.mark.parametrize("tail_leaves,tail_tree,tail_run", [("8", "0", "64"), ("64", "0", "1000"), ("0", "1000", "64"),
                                                             ("0", "1000", "3")])
def test_self_play_tail_mode_matches_oracle(spai, oracle, tmp_path, tail_leaves, tail_tree, tail_run):
    """the tail mode (search.hip select_tree RUN_ON): once a search call averages
    fewer than SPAI_TAIL_LEAVES leaves per iteration (default 0.05), the next one
    lets every tree run its iterations on through terminal leaves inside one
    launch; or once no tree of the previous call evaluated SPAI_TAIL_TREE_EVALS
    leaves (default 160; "1000" here: every call after the first).  A tree runs
    at most SPAI_TAIL_RUN terminal descents per pass (default 128; 3 here: most
    passes end at the cap, and a pass that slots no leaf does not end the call).
    Self-play with the hash evaluator on 48 games (one search chain) must still
    equal the oracle's sample stream bit for bit -- at 8 leaves per
    iteration (the last moves, once fewer than 8 games are left) and at 64, where
    tail-mode moves still hold trees that need evaluations -- and the per-move
    trace must show tail-mode moves (a sixth column of search passes).  (At the
    default threshold these games never reach a search call without evaluations;
    the other self-play parity tests run the default.)"""
    n, sims, seed = 48, 96, 23
    trace = tmp_path / "moves.csv"
    env = {"SPAI_TRACE_MOVES": str(trace), "SPAI_TAIL_LEAVES": tail_leaves, "SPAI_TAIL_TREE_EVALS": tail_tree,
           "SPAI_TAIL_RUN": tail_run}
    os.environ.update(env)
    try:
        e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, seed=seed)
        games, stats = e.self_play(n)
        e.close()
    finally:
        for k in env:
            del os.environ[k]
    ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42)
    k = 0
    for g in games:
        m = len(g["value"])
        assert list(ref["game"][k:k + m]) == [g["game"]] * m
        np.testing.assert_array_equal(g["policy"], ref["policy"][k:k + m])
        np.testing.assert_array_equal(g["value"], ref["value"][k:k + m])
        np.testing.assert_array_equal(g["enc"], ref["enc"][k:k + m])
        assert list(g["moves"]) == list(ref["moves"][g["game"], :m])
        k += m
    assert k == len(ref["value"]) and stats["sims"] == ref["sims"]
    rows = [[float(v) for v in l.split(",")] for l in trace.read_text().splitlines()]
    tail = [r for r in rows if r[5] > 0]
    assert tail, "no move ran in tail mode"
    if tail_run == "3":   # every call needs at least sims / 3 passes
        assert min(r[5] for r in tail) >= sims // 3, [r[5] for r in tail]
    elif tail_leaves == "64" or tail_tree == "1000":
        assert min(r[5] for r in tail) < sims / 4, [r[5] for r in tail]   # passes, not one per iteration
        # a tail move whose trees still needed evaluations (more than one chunk of passes)
        assert max(r[5] for r in tail) > kTailChunk, [r[5] for r in tail]


def test_self_play_net_properties(spai, oracle):
    """bf16 net self-play: every game is a legal Connect4 game ending in the
    recorded outcome; values are +-1/0 by perspective; policies are normalised."""
    n, sims = 128, 16
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_NET, seed=3)
    net = spai.Net(e, 6, spai.init_params(6, 64, seed=1))
    e.set_net(net)
    games, stats = e.self_play(n)
    assert len(games) == n and stats["games"] == n
    for g in games:
        mv = g["moves"]
        s = oracle.C4()
        for a in mv:
            s = s.next_state(int(a))
        assert s.status != 0
        m = len(mv)
        last = 1.0 if s.status == 2 else 0.0
        # the player who made the last move won: positions where they were to move get +1
        exp = np.array([last if (m - 1 - i) % 2 == 0 else -last for i in range(m)], np.float32)
        np.testing.assert_array_equal(g["value"], exp)
        np.testing.assert_allclose(g["policy"].sum(1), 1.0, atol=1e-6)
    e.close()


def _oracle_state(oracle, x, o, n, status):
    st = oracle.C4State()
    oracle.lib().or_c4_init(oracle.C.byref(st))
    for col in range(7):
        for row in range(6):
            b = 1 << (col * 7 + row)
            if x & b:
                st.board[row][col] = oracle.X
            elif o & b:
                st.board[row][col] = oracle.O
    st.num_actions_played = n
    st.current_player = oracle.X if n % 2 == 0 else oracle.O
    st.status = status
    return oracle.C4(st)


# ------------------------------------------------------------------ learner
def test_learner_vs_torch_golden(spai):
    """device train step (fp32) vs PyTorch CPU fp32: 3 Adam steps of a 1x64 net"""
    from test_oracle_golden import check_learner_params
    z = np.load(os.path.join(GOLDEN, "learner_c4_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    e = spai.Engine(num_searches=1, max_trees=1)
    L = spai.Learner(e, blocks, spai.init_params(blocks, hidden, seed=seed), hidden=hidden)
    losses = []
    for k in range(K):
        losses.append(L.train_batch(z["states"][k], z["policies"][k], z["values"][k]))
        if k == 0:
            g1, P1 = L.grads(), L.params()
    P3 = L.params()
    # step 1 is tight; later steps inherit Adam's amplification of fp32 noise in the
    # ill-conditioned (tiny-gradient) entries, in the reference as much as here
    np.testing.assert_allclose(losses[0], z["loss"][0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(losses), z["loss"], rtol=1e-3, atol=1e-4)
    g_ref = z["grads1"]
    assert np.abs(g1 - g_ref).max() <= 1e-4 * np.abs(g_ref).max()
    check_learner_params(P1, z["params1"], [g_ref], blocks, hidden, 1)
    params3 = np.load(os.path.join(GOLDEN, "learner_c4_1x64_step3.npz"))["params3"]
    check_learner_params(P3, params3, [g_ref], blocks, hidden, 3, tol=1e-4)
    L.close()
    e.close()


@pytest.mark.parametrize("blocks,B,steps", [(2, 48, 2), (6, 128, 1), (2, 128, 1), (0, 5, 1)])
def test_learner_vs_oracle(spai, oracle, blocks, B, steps):
    """other depths and batch sizes (incl. the reference's 128 and a tiny odd one)
    vs the numpy float64 restatement"""
    import learner_ref as LR
    from test_oracle_golden import check_learner_params
    rng = np.random.default_rng(blocks * 100 + B)
    states = _reachable_positions(spai, 4 * B, 10, seed=B)
    e = spai.Engine(num_searches=1, max_trees=1)
    e.games_resize(len(states))
    e.games_write(states)
    x_all = e.encode(len(states)).reshape(len(states), 126)
    batches = []
    for k in range(steps):
        x = x_all[k * B:(k + 1) * B]
        pi = rng.random((B, 7)).astype(np.float32) ** 2
        batches.append((x, (pi / pi.sum(1, keepdims=True)).astype(np.float32),
                        rng.choice(np.array([-1, 0, 1], np.float32), B)))
    p0 = spai.init_params(blocks, 64, seed=blocks + 7)
    L = spai.Learner(e, blocks, p0)
    dev_losses = [L.train_batch(*b) for b in batches[:1]]
    g1 = L.grads()
    _check_grads_same_masks(L, g1, p0, batches[0], blocks)   # reads the first step's activations
    dev_losses += [L.train_batch(*b) for b in batches[1:]]
    P_ref, ref_losses, ref_grads = LR.train(p0, batches, blocks, 64)
    np.testing.assert_allclose(dev_losses[0], ref_losses[0], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np.array(dev_losses), ref_losses, rtol=1e-3, atol=1e-4)
    check_learner_params(L.params(), P_ref, ref_grads, blocks, 64, steps, tol=1e-4)
    L.close()
    e.close()


def test_learner_rccl_single_rank(spai):
    """the RCCL path (gradient all-reduce + running-stat average) on a 1-rank
    communicator must leave the step bit-identical to the plain step"""
    z = np.load(os.path.join(GOLDEN, "learner_c4_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    out = []
    for use_comm in (False, True):
        e = spai.Engine(num_searches=1, max_trees=1)
        L = spai.Learner(e, blocks, spai.init_params(blocks, hidden, seed=seed), hidden=hidden)
        if use_comm:
            L.set_comm(0, 1, spai.comm_unique_id())
        loss = [L.train_batch(z["states"][k], z["policies"][k], z["values"][k]) for k in range(K)]
        out.append((np.array(loss), L.params()))
        L.close()
        e.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_learner_rccl_weighting_and_broadcast(spai):
    """the data-parallel step weights each rank's mean gradient by B / sum(B): on
    a 1-rank communicator that weight is exactly 1 for any B (steps of 32 and 48
    samples stay bit-identical to the plain steps); the RCCL broadcast of the
    parameters (weight refresh) leaves a single replica unchanged"""
    z = np.load(os.path.join(GOLDEN, "learner_c4_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    s = np.concatenate(list(z["states"]))
    p = np.concatenate(list(z["policies"]))
    v = np.concatenate(list(z["values"]))
    out = []
    for use_comm in (False, True):
        e = spai.Engine(num_searches=1, max_trees=1)
        L = spai.Learner(e, blocks, spai.init_params(blocks, hidden, seed=seed), hidden=hidden)
        if use_comm:
            L.set_comm(0, 1, spai.comm_unique_id())
        l1 = L.train_batch(s[:32], p[:32], v[:32])
        l2 = L.train_batch(s[32:80], p[32:80], v[32:80])
        before = L.params()
        L.broadcast(0)
        np.testing.assert_array_equal(L.params(), before)
        out.append((np.array([l1, l2]), before))
        L.close()
        e.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ pipeline
def test_pipeline_concurrent(spai, tmp_path):
    """train_concurrent (main.rs:137-235) end to end on one GPU: a self-play worker
    thread feeding the replay ring, the learner training batches from it, weights
    published per iteration and picked up by self-play, checkpoints written"""
    from pipeline_model import check_events
    blocks = 1
    p0 = spai.init_params(blocks, 64, seed=11)
    events = []
    st = spai.pipeline_run(p0, selfplay_devices=(0,), learner_device=0, checkpoint_dir=str(tmp_path),
                           games_per_batch=32, num_searches=16, batch_size=32, batches_per_iter=3, train_iters=3,
                           replay_capacity=320, blocks=blocks, seed=2, events=events)
    assert st["batches_trained"] == 9
    assert st["weight_version_published"] == 3
    assert st["games"] >= 32 and st["positions"] > 0
    # every push / pop against the HeapRb model: subsample sizes, FIFO batches bit for
    # bit, ring sizes, overwrites, weight versions (tests/pipeline_model.py)
    r = check_events(events, st, capacity=320, batch_size=32, fraction=0.3, batches_expected=9, workers=1)
    assert r["pushes"] * 32 == st["games"]
    assert all(np.isfinite(st["last_loss"])) and st["last_loss"][0] > 0
    for it in range(3):
        p = spai.load_params(str(tmp_path / ("%d.safetensors" % it)), blocks)
        assert p.shape == p0.shape and np.isfinite(p).all()
    assert not np.array_equal(spai.load_params(str(tmp_path / "2.safetensors"), blocks), p0)


def test_learner_train_batches_equals_single_steps(spai):
    """spai_learner_train_batches(k) is k spai_learner_train_batch calls: the same
    kernels in the same order, only the host synchronisation moves to the end, so
    parameters and every step's losses are bit-identical (5 steps, batch 48, the
    staging halves alternating and refilled twice)"""
    blocks, B, k = 2, 48, 5
    rng = np.random.default_rng(8)
    n = B * k
    states = _reachable_positions(spai, 3 * n, 10, seed=17)[:n]
    e = spai.Engine(num_searches=1, max_trees=1)
    e.games_resize(n)
    e.games_write(states)
    x = e.encode(n).reshape(n, 126)
    pi = rng.random((n, 7)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.choice(np.array([-1, 0, 1], np.float32), n)
    p0 = spai.init_params(blocks, 64, seed=6)
    one = spai.Learner(e, blocks, p0)
    l1 = np.stack([one.train_batch(x[j * B:(j + 1) * B], pi[j * B:(j + 1) * B], z[j * B:(j + 1) * B])
                   for j in range(k)])
    grp = spai.Learner(e, blocks, p0)
    l2 = grp.train_batches(x, pi, z, k)
    np.testing.assert_array_equal(l1, l2)
    np.testing.assert_array_equal(one.params(), grp.params())
    one.close()
    grp.close()
    e.close()


def test_learner_model_train_epochs(spai, oracle):
    """Model::train (model/mod.rs:100-149): a fresh Adam per call, one permutation of
    the samples, epochs x ceil(n/B) steps (short last batch) — vs the numpy oracle
    fed the same permutation"""
    import learner_ref as LR
    from test_oracle_golden import check_learner_params
    blocks, n, B, epochs, seed = 1, 70, 32, 2, 9
    rng = np.random.default_rng(4)
    states = _reachable_positions(spai, 3 * n, 8, seed=13)[:n]
    e = spai.Engine(num_searches=1, max_trees=1)
    e.games_resize(n)
    e.games_write(states)
    x = e.encode(n).reshape(n, 126)
    pi = rng.random((n, 7)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.choice(np.array([-1, 0, 1], np.float32), n)
    p0 = spai.init_params(blocks, 64, seed=5)
    L = spai.Learner(e, blocks, p0)
    L.train(x, pi, z, epochs=epochs, batch=B, seed=seed)
    L.train(x, pi, z, epochs=1, batch=B, seed=seed + 1)   # second call: Adam starts over
    P = L.params()
    ref, all_grads = p0.astype(np.float64), []
    for s_, ep in ((seed, epochs), (seed + 1, 1)):
        perm = spai.choose_multiple(n, n, seed=s_, stream=0x7EA1B).astype(np.int64)
        batches = [(x[perm[i:i + B]], pi[perm[i:i + B]], z[perm[i:i + B]]) for i in range(0, n, B)] * ep
        ref, _, grads = LR.train(ref, batches, blocks, 64)
        all_grads += grads
    check_learner_params(P, ref, all_grads, blocks, 64, len(all_grads), tol=2e-4)
    L.close()
    e.close()


def test_self_play_sampling_frequencies(spai):
    """learner_concurrent.rs:189-193 draws each move from WeightedIndex over
    (visit_count as f32).powf(T) with the unseeded thread_rng, so against the
    reference the move draw can only match in distribution.  Over >= 10^5 draws
    of the device move step (k_advance: Philox uniform, WeightedIndex over the
    visits^T table; 6400 games, hash evaluator), the played child's rank among
    its position's children (by visits) must fit P(child) = N^T / sum N^T at
    T = 1.25 (chi-square, tests/sampling_stats.py), and the same draws must
    reject plain visit counts (T = 1) and T = 1.5 -- the exponent is applied.
    (The bit-exact streams of test_self_play_device_sampling_matches_oracle pin
    the arithmetic itself.)"""
    from sampling_stats import rank_chi2
    n_games, sims, T = 6400, 32, 1.25
    e = spai.Engine(num_searches=sims, max_trees=n_games, eval_kind=spai.EVAL_HASH, seed=17, temperature=T)
    games, _ = e.self_play(n_games)
    e.close()
    pol = np.concatenate([g["policy"] for g in games])
    mv = np.concatenate([g["moves"] for g in games])
    assert len(mv) >= 100_000, len(mv)
    assert (pol[np.arange(len(mv)), mv] > 0).all()   # the played column was visited
    c, p, obs, exp = rank_chi2(pol, mv, T)
    assert p > 1e-4, (c, p, obs, exp)
    for t_alt in (1.0, 1.5):
        c_alt, p_alt, _, _ = rank_chi2(pol, mv, t_alt)
        assert p_alt < 1e-12, (t_alt, c_alt, p_alt)


@pytest.mark.parametrize("window", [37, 64, 160])
def test_self_play_stream_matches_oracle_per_game(spai, oracle, window):
    """spai_selfplay_stream: 160 games through `window` tree slots, a slot taking
    the next game as soon as its game ends (each game's draws keyed by its id and
    its own move number).  Every game -- its positions, visit policies, signed
    values and moves -- must be the oracle's lockstep self-play of the same game
    id bit for bit; only the order in which games finish differs.  window = 160
    is spai_selfplay_run itself, emission order included"""
    n, sims, seed, base = 160, 24, 5, 300
    e = spai.Engine(num_searches=sims, max_trees=n, eval_kind=spai.EVAL_HASH, seed=seed)
    games, stats = e.self_play(n, game_id_base=base, window=window)
    e.close()
    ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42,
                           game_id_base=base)
    by_game = {}
    k = 0
    while k < len(ref["value"]):
        g = int(ref["game"][k])
        m = int(np.sum(ref["game"] == g))
        by_game[g + base] = (ref["enc"][k:k + m], ref["policy"][k:k + m], ref["value"][k:k + m])
        k += m
    assert sorted(g["game"] for g in games) == sorted(by_game) and len(games) == n
    for g in games:
        enc, pol, val = by_game[g["game"]]
        np.testing.assert_array_equal(g["enc"], enc)
        np.testing.assert_array_equal(g["policy"], pol)
        np.testing.assert_array_equal(g["value"], val)
    assert stats["games"] == n and stats["sims"] == ref["sims"]
    if window == n:   # lockstep: the reference's emission order as well
        assert [g["game"] for g in games] == [int(v) + base for v in dict.fromkeys(ref["game"].tolist())]
