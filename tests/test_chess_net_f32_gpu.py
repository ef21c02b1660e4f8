"""The fp32 chess net (ChessNet(dtype="f32"), csrc/chess_net_f32.hip) on the MI355X,
wherever a chess net is used: forward, predict, search, self-play and match.

Yardsticks, none of which runs the kernel's code:
  tests/chess_f32_ref.py   the float32 restatement of the kernel's summation order
      (anchored on the CPU by tests/test_chess_f32_ref_cpu.py): every logit bit for
      bit; the value within ULP_TOL of tanh in float64 of its pre-activation (device
      tanhf against libm, tests/test_gpu_fp32.py's bar)
  the CPU oracle's encoding through forward: the search's leaf planes, unrounded
  the CPU oracle's Mcts::search driven by the device's fp32 forward
      (tests/chess_search_ref.py), with the guard of tests/test_chess_search_net_gpu.py
  the per-tree public API (search, advance, tree_reset) for spai_chess_match_run

Measured on the MI355X (each test prints its figures):
  value against tanh64 of the restatement's pre-activation: equal in every forward
  test (0, 1, 2 and 20 blocks, predict), at most 7.5e-9 over the deep search's 16
  drawn encodings (bound ULP_TOL, atol 2e-7)
  predict's priors against softmax64 -> float32 -> mask_invalid of the restatement's
  logits over the 24 positions: at most 3.00 float32 ulp (bound PRIOR_ULP = 16)
  deep search: none of the 24 trees left out by the noise guard
"""
import os

import numpy as np
import pytest

import chess_f32_ref as F
import chess_search_ref as R
from bf16_ref import ULP_TOL
from chess_match_ref import EVAL_NET, ONGOING, WON, abi_from_state, opening_index, pick_last_max
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

N = R.N_POSITIONS
PRIOR_ULP = 16.0       # tests/test_chess_search_net_gpu.py: the same softmax and mask kernel
NOISE_ULP = 64
MAX_LEFT_OUT = 2
ERR_INVALID = -1


@pytest.fixture(scope="module")
def ch():
    import chessref
    chessref.lib()
    yield chessref
    chessref.arena_reset()


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


def params_of(sc, blocks):
    """trained-like: non-identity BatchNorm and non-zero conv biases"""
    return F.trained_like(sc.init_params(blocks, 7 + blocks), blocks, 61 + blocks)


@pytest.fixture(scope="module")
def inputs():
    """6 oracle encodings (the golden's x) and 6 dense inputs: every tap, cell and channel matters"""
    g = np.load(os.path.join(GOLDEN, "chess_net_b1.npz"))
    dense = np.random.default_rng(12).standard_normal((6, 19, 8, 8)).astype(np.float32)
    return np.concatenate([g["x"], dense])


def check_value(v, vpre):
    want = F.value_of(vpre)
    worst = float(np.abs(v.astype(np.float64) - want).max())
    print(f"value against tanh64 of the restatement's pre-activation: at most {worst:.3g}")
    np.testing.assert_allclose(v, want, **ULP_TOL)


# ---- 1
@pytest.mark.parametrize("blocks", [0, 1, 2])
def test_logits_bit_for_bit(sc, inputs, blocks):
    """no residual; one block; the in-place buffer reused twice"""
    p = params_of(sc, blocks)
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    net = sc.ChessNet(eng, blocks, p, dtype="f32")
    lg, v = net.forward(inputs)
    ref_l, ref_vpre = F.forward(p, blocks, inputs)
    np.testing.assert_array_equal(lg, ref_l)
    check_value(v, ref_vpre)
    net.close()
    eng.close()


def test_logits_bit_for_bit_20_blocks(sc, inputs):
    p = params_of(sc, 20)
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    net = sc.ChessNet(eng, 20, p, dtype="f32")
    lg, v = net.forward(inputs[2:3])
    ref_l, ref_vpre = F.forward(p, 20, inputs[2:3])
    assert np.isfinite(ref_l).all() and np.abs(ref_l).max() > 0
    np.testing.assert_array_equal(lg, ref_l)
    check_value(v, ref_vpre)
    net.close()
    eng.close()


# ---- 2
def test_batch_independence(sc, inputs):
    """300 positions exceed the CU count; a row never depends on its slot or its batch"""
    x = np.random.default_rng(13).standard_normal((300, 19, 8, 8)).astype(np.float32)
    x[:12] = inputs
    p = params_of(sc, 2)
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    net = sc.ChessNet(eng, 2, p, dtype="f32")
    lg, v = net.forward(x)
    lg37, v37 = net.forward(x[:37])
    lg1, v1 = net.forward(x[3:4])
    np.testing.assert_array_equal(lg37, lg[:37])
    np.testing.assert_array_equal(v37, v[:37])
    np.testing.assert_array_equal(lg1[0], lg[3])
    assert v1[0].tobytes() == v[3].tobytes()
    # the same row in another slot of another batch
    lgp, vp = net.forward(x[::-1])
    np.testing.assert_array_equal(lgp[::-1], lg)
    np.testing.assert_array_equal(vp[::-1], v)
    net.close()
    eng.close()


# ---- 3
def test_set_params_dtype_and_default(sc, inputs):
    import ctypes as C
    pa, pb = params_of(sc, 1), F.trained_like(sc.init_params(1, 3), 1, 5)
    eng = sc.ChessEngine(num_searches=4, max_trees=8)
    net = sc.ChessNet(eng, 1, pa, dtype="f32")
    fresh = sc.ChessNet(eng, 1, pb, dtype="f32")
    before = net.forward(inputs)
    net.set_params(pb)
    got, want = net.forward(inputs), fresh.forward(inputs)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert not np.array_equal(before[0], got[0])
    with pytest.raises(sc.SpaiError) as ei:
        net.set_params(pb[:-1])
    assert ei.value.code == ERR_INVALID
    # the dtype is reported as created; anything else is invalid
    other = sc.ChessNet(eng, 1, pa, dtype="bf16")
    assert net.dtype == "f32" and other.dtype == "bf16"
    h = C.c_void_p()
    for bad in (2, -1, 7):
        rc = sc.lib().spai_chess_net_create_dtype(eng.h, 1, pa.ctypes.data_as(C.c_void_p), pa.size, bad, C.byref(h))
        assert rc == ERR_INVALID and not h.value, bad
    with pytest.raises(ValueError):
        sc.ChessNet(eng, 1, pa, dtype="fp32")
    # without a dtype: the bf16 net of test_chess_net_vs_torch_golden, row for row
    g = np.load(os.path.join(GOLDEN, "chess_net_b1.npz"))
    blocks, p = int(g["blocks"]), sc.init_params(int(g["blocks"]), int(g["seed"]))
    default, bf16, f32 = sc.ChessNet(eng, blocks, p), sc.ChessNet(eng, blocks, p, dtype="bf16"), \
        sc.ChessNet(eng, blocks, p, dtype="f32")
    assert default.dtype == "bf16"
    lg, v = default.forward(g["x"])
    lb, vb = bf16.forward(g["x"])
    np.testing.assert_array_equal(lg, lb)
    np.testing.assert_array_equal(v, vb)
    assert np.abs(lg - g["logits"]).max() <= 3e-2 * max(1.0, np.abs(g["logits"]).max())
    assert np.abs(v - g["value"]).max() <= 2e-2
    lf, vf = f32.forward(g["x"])
    assert not np.array_equal(lf, lg)
    for n in (net, fresh, other, default, bf16, f32):
        n.close()
    eng.close()


# ---- 4, 5, 6: the 24 positions
def load_slots(eng, sc, pos):
    """game slots [0, N) = the positions (tests/test_chess_search_net_gpu.py's loader)"""
    eng.games_resize(len(pos))
    for i, (seq, fen, s) in enumerate(pos):
        if fen is not None:
            eng.games_write(np.array([abi_from_state(s.st, sc.STATE_DTYPE)], sc.STATE_DTYPE), first=i)
    for p in range(max(len(seq) for seq, _, _ in pos if seq is not None)):
        given = [seq is not None and p < len(seq) for seq, _, _ in pos]
        rc = eng.apply(np.array([seq[p] if g else 0 for g, (seq, _, _) in zip(given, pos)], np.uint16), check=False)
        assert all(rc[i] == 0 for i in range(len(pos)) if given[i]), (p, rc)


@pytest.fixture(scope="module")
def S(ch, sc):
    pos = R.positions()
    states = [s for _, _, s in pos]
    params = sc.init_params(1, 5)
    eng = sc.ChessEngine(num_searches=96, max_trees=N, eval_kind=sc.EVAL_NET)
    net = sc.ChessNet(eng, 1, params, dtype="f32")
    eng.set_net(net)
    load_slots(eng, sc, pos)
    x = np.stack([s.encoding() for s in states])
    assert np.array_equal(eng.encode(N), x)
    pred_p, pred_v = net.predict(N)
    logits, value = net.forward(x)
    ref_l, ref_vpre = F.forward(params, 1, x)      # the restatement, once for every test below
    moves = [s.valid_actions() for s in states]
    index = [[sc.move_index(s.side, m) for m in mv] for s, mv in zip(states, moves)]

    def reset():
        eng.trees_create(N)
        for t in range(N):
            eng.tree_reset(t, t)

    reset()
    order = np.random.default_rng(1).permutation(N).astype(np.uint32)   # batch slot != tree != game slot
    eng.search(order, num_searches=1)
    d = dict(eng=eng, net=net, params=params, states=states, x=x, pred_p=pred_p, pred_v=pred_v, logits=logits,
             value=value, ref_l=ref_l, ref_vpre=ref_vpre, moves=moves, index=index, reset=reset,
             one=[eng.tree_child_stats(t) for t in range(N)], one_root=[eng.tree_root(t) for t in range(N)])
    yield d
    net.close()
    eng.close()


def test_predict(S):
    """largest prior difference measured: 3.00 float32 ulp (24 positions, 1 block, init seed 5)"""
    np.testing.assert_array_equal(S["logits"], S["ref_l"])
    worst = 0.0
    for t, s in enumerate(S["states"]):
        ref = s.mask_invalid(R.softmax64(S["ref_l"][t]).astype(np.float32))
        got = S["pred_p"][t]
        assert np.array_equal(np.flatnonzero(got), np.sort(S["index"][t])), t     # exactly the legal moves
        assert np.array_equal(np.flatnonzero(ref), np.flatnonzero(got)), t
        worst = max(worst, float(R.ulps(got[S["index"][t]], ref[S["index"][t]]).max()))
    print(f"largest prior difference to softmax64 of the restatement's logits: {worst:.2f} float32 ulp")
    assert worst <= PRIOR_ULP, worst
    check_value(S["pred_v"], S["ref_vpre"])
    assert S["pred_v"].tobytes() == S["value"].tobytes()


def test_one_simulation_roots(S):
    """k_cleaf's fp32 planes, the batch slot and the expansion: every root holds predict's
    priors and value; the value is forward's of the oracle's own, unrounded encoding"""
    from bf16_ref import bf16_round
    x = S["x"]
    rounded = [t for t in range(N)
               if any(not np.array_equal(bf16_round(x[t, p]).astype(np.float32), x[t, p]) for p in (17, 18))]
    assert rounded, "no position whose fifty-move or move-count plane bf16 would round"
    for t, (mv, vis, w, pr) in enumerate(S["one"]):
        assert list(mv) == S["moves"][t] and not vis.any() and not w.any(), t
        want = S["pred_p"][t][S["index"][t]]
        assert pr.dtype == want.dtype == np.float32 and pr.tobytes() == want.tobytes(), t
    for t, (root, visits, value_sum) in enumerate(S["one_root"]):
        assert visits == 1, t
        assert np.float32(value_sum).tobytes() == S["pred_v"][t].tobytes(), (t, value_sum, S["pred_v"][t])
        assert np.float32(value_sum).tobytes() == S["value"][t].tobytes(), (t, value_sum, S["value"][t])


def test_deep_search_matches_oracle_with_device_forward(S):
    eng, net, states = S["eng"], S["net"], S["states"]
    sims = 48
    trees = np.arange(N, dtype=np.uint32)
    S["reset"]()
    dev1 = eng.search(trees, num_searches=sims)
    picks = [R.most_visited_last(dev1[2][t], dev1[4][t]) for t in range(N)]
    root1 = [eng.tree_root(t)[1] for t in range(N)]
    eng.advance(trees, picks)
    dev2 = eng.search(trees, num_searches=sims)
    root2 = [eng.tree_root(t)[1] for t in range(N)]

    ev = R.Evaluator(net.forward)
    runs = []
    for noise in (None, (1, NOISE_ULP), (2, NOISE_ULP), (3, NOISE_ULP)):
        rs = R.RefSearch(states, ev, c=2.0, fault=None, noise=noise)
        r1 = rs.search(sims)
        assert list(r1["nc"]) == list(dev1[4])
        rs.advance(picks)
        r2 = rs.search(sims)
        runs.append((rs, r1, r2))
        rs.close()
    ref, ref1, ref2 = runs[0]
    tables = [(R.visit_table(r1), R.visit_table(r2)) for _, r1, r2 in runs]
    left_out = [t for t in range(N) if any(tb[0][t] != tables[0][0][t] or tb[1][t] != tables[0][1][t]
                                           for tb in tables[1:])]
    print(f"left out as unstable under {NOISE_ULP} ulp of noise: {left_out}")
    assert len(left_out) <= MAX_LEFT_OUT, left_out
    assert ref.sides == {0, 1} and ref.path_rep2 >= 1 and len(ref.seen) > N * 20

    for t in range(N):
        if t in left_out:
            continue
        for (pol, ids, vis, mv, nc), r in ((dev1, ref1), (dev2, ref2)):
            k = int(nc[t])
            assert k == r["nc"][t], t
            assert np.array_equal(mv[t, :k], r["moves"][t, :k].astype(np.uint16)), t
            assert np.array_equal(vis[t, :k], r["visits"][t, :k]), (t, vis[t, :k], r["visits"][t, :k])
            assert np.array_equal(pol[t], r["policy"][t]), t
        assert root1[t] == sims
        assert root2[t] == int(ref1["visits"][t, picks[t]]) + sims

    # independence from the device: what drove the reference is the restatement's arithmetic
    keys = sorted(ev.cache)
    take = np.random.default_rng(6).choice(len(keys), 16, replace=False)
    enc = np.stack([np.frombuffer(keys[i], np.float32).reshape(19, 8, 8) for i in take])
    lg, v = net.forward(enc)
    ref_l, ref_vpre = F.forward(S["params"], 1, enc)
    np.testing.assert_array_equal(lg, ref_l)
    check_value(v, ref_vpre)


# ---- 7
def test_self_play(ch, sc):
    n, sims = 2, 4
    eng = sc.ChessEngine(num_searches=sims, max_trees=n, eval_kind=sc.EVAL_NET, seed=2, max_moves=2048)
    net = sc.ChessNet(eng, 1, sc.init_params(1, 4), dtype="f32")
    eng.set_net(net)
    games, stats = eng.self_play(n)
    streamed, stats_w = eng.self_play(n, window=1)
    assert stats["games"] == stats_w["games"] == n
    assert sorted(g["game"] for g in games) == sorted(g["game"] for g in streamed) == list(range(n))
    by_id = {g["game"]: g for g in streamed}
    for g in games:
        w = by_id[g["game"]]
        assert g["n"] == w["n"]
        for k in ("enc", "policy", "value", "moves"):
            assert np.array_equal(g[k], w[k]), (g["game"], k)
        assert np.allclose(g["policy"].sum(1), 1.0, atol=1e-5)
        s = ch.ChessState()
        for i, m in enumerate(g["moves"]):
            assert np.array_equal(g["enc"][i].reshape(19, 8, 8), s.encoding()), (g["game"], i)
            assert int(m) in s.valid_actions()
            s = s.next_state(int(m))
        assert s.value_terminated()[1]
    net.close()
    eng.close()


# ---- 8
def replay_match(sc, ch, a, b, n_games, opening_plies, max_plies, seed):
    """chess_match_ref.device_match's loop (one engine per player, one tree per call through
    search / advance / tree_reset) with each player's net in its own dtype.
    a, b: (params, dtype, num_searches)"""
    import oracle as _oracle
    _oracle.lib()
    players = (a, b)
    engs, nets = [], []
    for params, dtype, n_s in players:
        e = sc.ChessEngine(num_searches=n_s, max_trees=n_games, eval_kind=EVAL_NET, max_moves=256)
        nets.append(sc.ChessNet(e, 1, params, dtype=dtype))
        e.set_net(nets[-1])
        e.games_resize(n_games)
        e.trees_create(n_games)
        engs.append(e)
    opening = [[] for _ in range(n_games)]
    for k in range(opening_plies):
        mv, cnt = engs[0].legal_moves(n_games)
        pick = np.array([mv[g, opening_index(_oracle.lib().or_u01_f32(seed, g // 2, k), int(cnt[g]))]
                         for g in range(n_games)], np.uint16)
        for e in engs:
            e.apply(pick)
        for g in range(n_games):
            opening[g].append(int(pick[g]))
    for e in engs:
        for g in range(n_games):
            e.tree_reset(g, g)
    games = []
    for g in range(n_games):
        moves = list(opening[g])
        G = dict(game=g, a_moves_first=g % 2 == 0, result_a=0, status=ONGOING, adjudicated=False)
        searched = 0
        while True:
            if len(moves) >= max_plies:
                G["adjudicated"] = True
                break
            p = (g + searched) & 1
            E, O = engs[p], engs[p ^ 1]
            _, _, vis, mv, nc = E.search([g], players[p][2])
            k = pick_last_max(vis[0, :nc[0]])
            assert k is not None
            move = int(mv[0, k])
            status, _ = E.advance([g], [k])
            moves.append(move)
            searched += 1
            G["status"] = int(status[0])
            if status[0] != ONGOING:
                if status[0] == WON:
                    G["result_a"] = 1 if p == 0 else -1
                break
            for e in engs:
                e.apply(np.array([move], np.uint16), first=g)
            if O.tree_root(g)[1] == 0:   # a root never visited has no children: start the tree anew
                O.tree_reset(g, g)
            else:
                O.advance([g], [k])
            assert E.tree_root(g)[0].tobytes() == O.tree_root(g)[0].tobytes()
        G["n_moves"] = len(moves)
        G["moves"] = np.array(moves, np.uint16)
        games.append(G)
    for net in nets:
        net.close()
    for e in engs:
        e.close()
    return games


MATCH_CASES = {
    "f32_vs_f32": ((3, "f32"), (4, "f32")),
    "f32_vs_bf16": ((3, "f32"), (3, "bf16")),
    "bf16_vs_f32": ((3, "bf16"), (3, "f32")),
    "f32_vs_bf16_other_seed": ((4, "f32"), (4, "bf16")),
}


@pytest.mark.parametrize("case", list(MATCH_CASES))
def test_match_equals_per_tree_replay(ch, sc, case):
    """spai_chess_match_run with fp32 players, on two streams and on one: each chain's leaf
    batch follows its own player's net (mixed dtypes on the two chains, in both orders)"""
    n, sims, max_plies = 4, 8, 24
    (sa, da), (sb, db) = MATCH_CASES[case]
    pa, pb = sc.init_params(1, sa), sc.init_params(1, sb)
    want = replay_match(sc, ch, (pa, da, sims), (pb, db, sims), n, 2, max_plies, seed=5)
    eng = sc.ChessEngine(num_searches=sims, max_trees=2 * n, eval_kind=sc.EVAL_UNIFORM, max_moves=256)
    na, nb = sc.ChessNet(eng, 1, pa, dtype=da), sc.ChessNet(eng, 1, pb, dtype=db)
    for one_stream in (False, True):
        eng.match_one_stream(one_stream)
        games, stats = eng.match((EVAL_NET, na, sims), (EVAL_NET, nb, sims), n, opening_plies=2,
                                 max_plies=max_plies, seed=5)
        assert len(games) == len(want)
        for g, w in zip(games, want):
            assert np.array_equal(g["moves"], w["moves"]), (one_stream, g["game"], list(g["moves"]), list(w["moves"]))
            for k in ("game", "a_moves_first", "result_a", "status", "adjudicated", "n_moves"):
                assert g[k] == w[k], (one_stream, g["game"], k, g[k], w[k])
    eng.match_one_stream(False)
    for g in games:   # every move is legal
        s = ch.ChessState()
        for m in g["moves"]:
            assert int(m) in s.valid_actions()
            s = s.next_state(int(m))
    na.close()
    nb.close()
    eng.close()
