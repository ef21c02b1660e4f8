"""Pins tests/match_ref.py, the CPU restatement of spai_match_run that the device
tests (test_match_gpu.py) are held to: the openings, the pairing of games, the
last-max move rule on a game worked out by hand, and how the second tree of a game
follows the moves.
"""
import numpy as np
import pytest

import match_ref


@pytest.fixture(scope="module")
def ref(oracle):
    return match_ref


def test_pairs_share_their_opening(ref, oracle):
    hash16 = (oracle.EVAL_HASH, None, 16)
    uni8 = (oracle.EVAL_UNIFORM, None, 8)
    for plies in (0, 1, 6):
        games, _ = ref.play_match(hash16, uni8, 6, plies, seed=5, game_id_base=2)
        for p in range(3):
            g0, g1 = games[2 * p], games[2 * p + 1]
            assert (g0["game"], g1["game"]) == (2 + 2 * p, 3 + 2 * p)
            assert g0["a_moves_first"] and not g1["a_moves_first"]
            assert g0["moves"][:plies] == g1["moves"][:plies] == ref.opening_moves(5, 1 + p, plies)[0]
    # the openings differ between pairs and with the seed
    six = [tuple(ref.opening_moves(5, p, 6)[0]) for p in range(8)]
    assert len(set(six)) > 1
    assert six != [tuple(ref.opening_moves(6, p, 6)[0]) for p in range(8)]


def test_identical_players_mirror_within_a_pair(ref, oracle):
    pl = (oracle.EVAL_HASH, None, 16)
    games, stats = ref.play_match(pl, pl, 8, 3, seed=9)
    for p in range(4):
        g0, g1 = games[2 * p], games[2 * p + 1]
        assert g0["moves"] == g1["moves"]
        assert g0["result_a"] == -g1["result_a"]
    assert sum(g["result_a"] for g in games) == 0
    assert stats["a_wins"][0] == stats["b_wins"][1] and stats["b_wins"][0] == stats["a_wins"][1]
    assert stats["draws"][0] == stats["draws"][1]
    assert stats["sims"][0] == stats["sims"][1] and stats["evals"][0] == stats["evals"][1]


def test_opening_index_is_one_f32_multiply(ref, oracle):
    """idx = min((int)(u * (float)n_legal), n_legal - 1) against a direct computation: u has 24
    significant bits and n_legal 3, so the float64 product is exact and its rounding
    to float32 is the one f32 multiply."""
    L = oracle.lib()
    us = [0.0, 1.0 - 2.0 ** -23, 0.5, 1.0 / 3.0, 2.0 ** -23] + [L.or_u01_f32(7, g, k) for g in range(40) for k in range(6)]
    for n_legal in range(1, 8):
        for u in us:
            u32 = np.float32(u)
            exp = min(int(np.float32(np.float64(u32) * n_legal)), n_legal - 1)
            vec = int(np.minimum((np.array([u32]) * np.float32(n_legal)).astype(np.int32), n_legal - 1)[0])
            assert ref.opening_index(u32, n_legal) == exp == vec
            assert 0 <= exp < n_legal
        assert ref.opening_index(0.0, n_legal) == 0
        assert ref.opening_index(1.0 - 2.0 ** -23, n_legal) == n_legal - 1
    # the opening itself: the idx-th legal column in ascending order, from the (seed, pair, k) draw
    for pair in range(6):
        moves, _ = ref.opening_moves(3, pair, 6)
        s = oracle.C4()
        for k, a in enumerate(moves):
            legal = s.valid_actions()
            assert a == legal[int(np.float32(L.or_u01_f32(3, pair, k)) * np.float32(len(legal)))]
            s = s.next_state(a)


def test_hand_checked_uniform_game(ref, oracle):
    """UNIFORM against UNIFORM at 2 simulations, no opening.  Every search starts from a
    root without children (a fresh tree, or the unvisited child the opponent's move
    re-rooted to): simulation 1 expands it, simulation 2 goes to the last of the equally
    scored children, so the mover plays the highest open column (the first-selection
    KAT: column 6).  Columns 6, 5, 4 fill up with the movers alternating, so row 0 is
    the first mover's in each; stone 19, column 3, makes four in row 0."""
    uni = (oracle.EVAL_UNIFORM, None, 2)
    games, stats = ref.play_match(uni, uni, 2, 0, seed=0)
    line = [6] * 6 + [5] * 6 + [4] * 6 + [3]
    assert games[0]["moves"] == games[1]["moves"] == line
    assert (games[0]["result_a"], games[1]["result_a"]) == (1, -1)
    assert stats["a_wins"] == [1.0, 0.0] and stats["b_wins"] == [0.0, 1.0] and stats["draws"] == [0.0, 0.0]
    # the first mover searched 10 times and the second 9 in each game; the winning
    # move's second simulation ends on the won position, which is not evaluated
    assert stats["sims"] == [2.0 * 19, 2.0 * 19]
    assert stats["evals"] == [2.0 * 19 - 1, 2.0 * 19 - 1]


def test_single_simulation_has_no_move(ref, oracle):
    """one simulation only expands the root: no child is visited, the device's SPAI_ERR_NAN"""
    one = (oracle.EVAL_HASH, None, 1)
    with pytest.raises(ref.MatchNaN):
        ref.play_match(one, (oracle.EVAL_UNIFORM, None, 1), 1, 0, seed=0)


@pytest.mark.parametrize("game_id", [0, 1])
def test_second_movers_tree_is_replaced_once_then_rerooted(ref, oracle, game_id):
    trace = []
    players = ((oracle.EVAL_HASH, None, 16), (oracle.EVAL_UNIFORM, None, 24))
    g = ref.play_game(game_id, players, 2, seed=4, trace=trace)
    assert len(trace) == len(g["moves"]) - 2 >= 5   # no game ends before its 7th stone
    first = game_id & 1   # plies are even after the 2-ply opening: the id's parity moves first
    assert [s["mover"] for s in trace] == [(first + k) & 1 for k in range(len(trace))]
    assert trace[0]["replaced"]                       # the second mover's tree had no children yet
    assert not any(s["replaced"] for s in trace[1:])  # from then on both trees are re-rooted
    for s in trace[1:]:
        assert s["root_visits_after"] == s["child_visits_before"]   # the new root keeps N (quirk Q4)
    assert any(s["root_visits_after"] > 0 for s in trace[1:])
