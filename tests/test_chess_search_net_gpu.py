"""The chess search's net path on the MI355X: the fused net input of k_cleaf, the
net branch of k_cexpand (softmax, gather through policy_index, renormalise, value
by batch slot) and their link through k_chess_forward, in partial and oversized
batches.  The stub evaluators never run this code, or run it on data that cannot
show an error.

Yardsticks, none of which runs the search's code:
  spai_chess_predict on the same game slots (k_encode, k_slots_softmax_mask):
      after one simulation the root's priors and value are predict's, bit for bit;
  the CPU oracle's encoding through the same device forward: the same value bit
      for bit, and its float64 softmax + mask_invalid within PRIOR_ULP;
  the CPU oracle's Mcts::search with that forward as its evaluator
      (tests/chess_search_ref.py): deep searches with the same visit counts.

PRIOR_ULP: the device's priors against float64 softmax -> float32 -> the
oracle's mask_invalid differ by the device's expf and its float32 softmax sum.
Measured over the 24 positions (1 block, init seed 5): at most 3 float32 ulp
(5 ulp with the renormalising sum in shuffle order, as it was before this test);
asserted 4 x that rounded up to a power of two = 16 ulp, which meets the
condition of the deep-search guard: <= 16 ulp, a quarter of its 64 ulp noise.

The deep search's guard: the reference's priors are the float64 ones, so a tree
whose reference visit counts move under 64 ulp of noise on every softmax entry
(three reruns from the cache) cannot be compared and is left out; at most 2 of
24 may be.  tests/test_chess_search_ref_cpu.py shows on the CPU that this noise
moves no tree while each fault of the net path moves at least a quarter."""
import numpy as np
import pytest

import chess_search_ref as R
from chess_match_ref import abi_from_state

pytestmark = pytest.mark.gpu

N = R.N_POSITIONS
PRIOR_ULP = 16.0
NOISE_ULP = 64
MAX_LEFT_OUT = 2


def load_slots(eng, sc, pos):
    """game slots [0, N) = the positions: lines applied from the start position (the slot
    holds the history), FEN positions written (empty history)"""
    eng.games_resize(len(pos))
    for i, (seq, fen, s) in enumerate(pos):
        if fen is not None:
            eng.games_write(np.array([abi_from_state(s.st, sc.STATE_DTYPE)], sc.STATE_DTYPE), first=i)
    for p in range(max(len(seq) for seq, _, _ in pos if seq is not None)):
        given = [seq is not None and p < len(seq) for seq, _, _ in pos]
        rc = eng.apply(np.array([seq[p] if g else 0 for g, (seq, _, _) in zip(given, pos)], np.uint16), check=False)
        assert all(rc[i] == 0 for i in range(len(pos)) if given[i]), (p, rc)


def child_stats(eng, trees):
    return [eng.tree_child_stats(t) for t in trees]


def same_stats(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def S():
    """the positions as slots and oracle states, a 1-block net, predict and the
    references on them, and the trees after one simulation"""
    import chessref as ch
    import spai_chess as sc
    ch.lib()
    pos = R.positions()
    states = [s for _, _, s in pos]
    eng = sc.ChessEngine(num_searches=96, max_trees=N, eval_kind=sc.EVAL_NET)
    net = sc.ChessNet(eng, 1, sc.init_params(1, 5))
    eng.set_net(net)
    load_slots(eng, sc, pos)
    pred_p, pred_v = net.predict(N)
    x = np.stack([s.encoding() for s in states])
    logits, value = net.forward(x)
    ref_p = np.stack([s.mask_invalid(R.softmax64(logits[i]).astype(np.float32)) for i, s in enumerate(states)])
    moves = [s.valid_actions() for s in states]
    index = [[sc.move_index(s.side, m) for m in mv] for s, mv in zip(states, moves)]

    def reset():
        eng.trees_create(N)
        for t in range(N):
            eng.tree_reset(t, t)

    reset()
    unexpanded = child_stats(eng, range(N))
    order = np.random.default_rng(1).permutation(N).astype(np.uint32)   # batch slot != tree != game slot
    eng.search(order, num_searches=1)
    d = dict(ch=ch, sc=sc, eng=eng, net=net, pos=pos, states=states, pred_p=pred_p, pred_v=pred_v, x=x,
             logits=logits, value=value, ref_p=ref_p, moves=moves, index=index, reset=reset, unexpanded=unexpanded,
             one=child_stats(eng, range(N)), one_root=[eng.tree_root(t) for t in range(N)])
    yield d
    ch.arena_reset()
    net.close()
    eng.close()


# ---- B1
def test_positions_cover_the_planes(S):
    states, eng = S["states"], S["eng"]
    assert len(states) == N and all(s.status == 0 for s in states)
    assert {s.side for s in states} == {0, 1}
    assert any(s.repetitions() == 2 for s in states)
    assert any(s.st.fifty > 0 for s in states)
    for p in (12, 13, 14, 15):
        assert {float(v) for v in S["x"][:, p, 0, 0]} == {0.0, 1.0}, p
    # the slots hold the same positions (k_encode is compared with orc_encoding elsewhere too)
    assert np.array_equal(eng.encode(N), S["x"])
    st, reps, _, _ = eng.status(N)
    assert not st.any() and list(reps) == [s.repetitions() for s in states]


# ---- A
def test_child_stats_accessor(S):
    eng, sc = S["eng"], S["sc"]
    for mv, vis, w, pr in S["unexpanded"]:
        assert len(mv) == len(vis) == len(w) == len(pr) == 0
    for t in (0, 7, N - 1):
        mv, vis, w, pr = eng.tree_child_stats(t)
        mv2, vis2 = eng.tree_children(t)
        assert np.array_equal(mv, mv2) and np.array_equal(vis, vis2)
        assert same_stats((mv, vis, w, pr), S["one"][t])     # reading changes nothing
    with pytest.raises(sc.SpaiError):
        eng.tree_child_stats(N)


def test_child_stats_after_compaction(S):
    """a tree whose arena half fills up is copied into the other half (k_ccompact);
    the accessor follows it: the same game on an engine whose arena never fills
    gives the same records at every move"""
    sc = S["sc"]
    sims = 16
    small = sc.ChessEngine(num_searches=sims, max_trees=1, eval_kind=sc.EVAL_NET)   # 16,384 nodes per half
    big = sc.ChessEngine(num_searches=96, max_trees=1, eval_kind=sc.EVAL_NET)       # 83,712
    nets = [sc.ChessNet(e, 1, sc.init_params(1, 5)) for e in (small, big)]
    for e, net in zip((small, big), nets):
        e.set_net(net)
        e.trees_create(1)
    compacted_at = None
    for ply in range(60):
        ids = small.search([0], num_searches=sims)[1]
        big.search([0], num_searches=sims)
        # the root's children stand right behind it only in a fresh tree or after a copy
        if ply > 0 and ids[0, 0] == 1 and compacted_at is None:
            compacted_at = ply
        a, b = small.tree_child_stats(0), big.tree_child_stats(0)
        assert same_stats(a, b), ply
        assert a[1].sum() == small.tree_root(0)[1] - 1 and small.tree_root(0)[1:] == big.tree_root(0)[1:], ply
        if compacted_at is not None and ply >= compacted_at + 2:
            break
        pick = R.most_visited_last(a[1], len(a[1]))
        st, _ = small.advance([0], [pick])
        big.advance([0], [pick])
        assert st[0] == 0, ply
    assert compacted_at is not None
    for e, net in zip((small, big), nets):
        net.close()
        e.close()


# ---- B2
def test_one_simulation_children_are_the_legal_moves(S):
    for t, (mv, vis, w, pr) in enumerate(S["one"]):
        assert list(mv) == S["moves"][t], t
        assert not vis.any() and not w.any(), t


def test_one_simulation_priors_equal_predict(S):
    """any wrong plane of k_cleaf, a batch slot taken for a tree and any other order
    of the renormalising sum show here"""
    bad_trees, bad, total = [], 0, 0
    for t, (mv, vis, w, pr) in enumerate(S["one"]):
        want = S["pred_p"][t][S["index"][t]]
        assert pr.dtype == want.dtype == np.float32 and len(pr) == len(want)
        diff = int((pr.view(np.uint32) != want.view(np.uint32)).sum())
        total += len(pr)
        if diff:
            bad_trees.append(t)
            bad += diff
    print(f"priors differing from predict: {bad} of {total} at {len(bad_trees)} of {N} positions")
    assert not bad, f"{bad} of {total} priors differ from predict's, at positions {bad_trees}"


def test_one_simulation_root_equals_predict_value(S):
    for t, (root, visits, value_sum) in enumerate(S["one_root"]):
        assert visits == 1, t
        assert np.float32(value_sum).tobytes() == S["pred_v"][t].tobytes(), (t, value_sum, S["pred_v"][t])


def test_one_simulation_value_equals_forward_of_oracle_encoding(S):
    for t, (root, visits, value_sum) in enumerate(S["one_root"]):
        assert np.float32(value_sum).tobytes() == S["value"][t].tobytes(), (t, value_sum, S["value"][t])


def test_one_simulation_priors_within_bound_of_float64(S):
    worst = 0.0
    for t, (mv, vis, w, pr) in enumerate(S["one"]):
        ref = S["ref_p"][t]
        assert np.array_equal(np.flatnonzero(ref), np.sort(S["index"][t])), t
        worst = max(worst, float(R.ulps(pr, ref[S["index"][t]]).max()))
    print(f"largest prior difference to the float64 reference: {worst:.2f} float32 ulp")
    assert worst <= PRIOR_ULP, worst


# ---- B4
def test_second_simulation_visits_last_argmax_of_priors(S):
    eng = S["eng"]
    S["reset"]()
    eng.search(np.arange(N, dtype=np.uint32), num_searches=2)
    skipped = []
    for t in range(N):
        mv, vis, w, pr = eng.tree_child_stats(t)
        ref = S["ref_p"][t][S["index"][t]]
        top = len(ref) - 1 - int(np.argmax(ref[::-1]))           # quirk Q2: the last of equal maxima
        rest = np.delete(ref, top)
        # each of the two may be off by the bound
        if len(rest) and float(R.ulps(rest.max(), ref[top])) <= 2 * PRIOR_ULP:
            skipped.append(t)
            continue
        assert vis.sum() == 1 and vis[top] == 1, (t, top, np.flatnonzero(vis))
        assert eng.tree_root(t)[1] == 2
    assert len(skipped) <= 2, skipped


# ---- B3
def test_more_positions_than_cus(S):
    """300 leaves in one forward: two positions per workgroup, a partial last block
    of k_cleaf / k_cexpand; every tree as in the 24-tree run of its position"""
    sc = S["sc"]
    big = 300
    eng = sc.ChessEngine(num_searches=2, max_trees=big, eval_kind=sc.EVAL_NET)
    net = sc.ChessNet(eng, 1, sc.init_params(1, 5))
    eng.set_net(net)
    load_slots(eng, sc, S["pos"])
    eng.trees_create(big)
    for t in range(N):
        eng.tree_reset(t, t)
    eng.search(np.arange(N, dtype=np.uint32), num_searches=2)
    small = child_stats(eng, range(N))
    small_root = [eng.tree_root(t)[1:] for t in range(N)]
    for t in range(N):
        assert same_stats(small[t][:1] + small[t][3:], S["one"][t][:1] + S["one"][t][3:]), t   # moves and priors
    for t in range(big):
        eng.tree_reset(t, t % N)
    eng.search(np.random.default_rng(2).permutation(big).astype(np.uint32), num_searches=2)
    for t in range(big):
        assert same_stats(eng.tree_child_stats(t), small[t % N]), t
        assert eng.tree_root(t)[1:] == small_root[t % N], t
    net.close()
    eng.close()


# ---- B5
def test_deep_search_matches_oracle_with_device_forward(S):
    eng, net, states = S["eng"], S["net"], S["states"]
    sims = 48
    trees = np.arange(N, dtype=np.uint32)
    S["reset"]()
    eng.set_timing(True)
    dev1 = eng.search(trees, num_searches=sims)
    picks = [R.most_visited_last(dev1[2][t], dev1[4][t]) for t in range(N)]
    root1 = [eng.tree_root(t)[1] for t in range(N)]
    eng.advance(trees, picks)
    dev2 = eng.search(trees, num_searches=sims)
    root2 = [eng.tree_root(t)[1] for t in range(N)]
    sampled = eng.timing()[2]   # trees and leaves of every 8th iteration of both searches
    eng.set_timing(False)

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

    # the reference walked what this test is about
    assert ref.sides == {0, 1}
    assert ref.path_rep2 >= 1
    assert len(ref.seen) > N * 20
    assert ref1["evals"] + ref2["evals"] == ref.evals
    # evaluation counts: the search call does not return the device's, its timer samples the
    # leaves of every 8th iteration; they are the reference's when no tree is left out
    assert len(ref1["batches"]) == len(ref2["batches"]) == sims
    assert sampled[0] == 2 * N * len(range(0, sims, 8))
    if not left_out:
        assert sampled[1] == sampled[2] == sum(ref1["batches"][0::8]) + sum(ref2["batches"][0::8])

    for t in range(N):
        if t in left_out:
            continue
        for (pol, ids, vis, mv, nc), r in ((dev1, ref1), (dev2, ref2)):
            k = int(nc[t])
            assert k == r["nc"][t], t
            assert np.array_equal(mv[t, :k], r["moves"][t, :k].astype(np.uint16)), t
            assert np.array_equal(vis[t, :k], r["visits"][t, :k]), (t, vis[t, :k], r["visits"][t, :k])
            assert np.array_equal(pol[t], r["policy"][t]), t
        # the root's visit count: every simulation passes it; the new root keeps its own
        assert root1[t] == sims
        assert root2[t] == int(ref1["visits"][t, picks[t]]) + sims
