"""The yardstick of the chess match tests (tests/chess_match_ref.py oracle_match)
pinned on the CPU: what the GPU tests compare spai_chess_match_run against has
to be right by itself.  No GPU, no product code."""
import numpy as np
import pytest

import chess_match_ref as ref
from chess_match_ref import EVAL_HASH, EVAL_UNIFORM, MATE_IN_ONE, ONGOING, SHUFFLE, TIED, WON

STATE_DTYPE = np.dtype([("pieces", "<u8", 6), ("colors", "<u8", 2), ("side", "u1"), ("castle", "u1"),
                        ("ep", "u1"), ("status", "u1"), ("fifty", "<u2"), ("made", "<u2"), ("reps", "<u4"),
                        ("pad", "<u4")])


@pytest.fixture(scope="module")
def ch():
    import chessref
    chessref.lib()
    yield chessref
    chessref.arena_reset()


def start_of(ch, fen):
    return np.array([ref.abi_from_state(ch.ChessState(fen=fen).st, STATE_DTYPE)], STATE_DTYPE)


def test_opening_index_edges():
    below_one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    assert ref.opening_index(below_one, 20) == 19 and ref.opening_index(below_one, 218) == 217
    assert ref.opening_index(1.0, 20) == 19   # (no 23-bit uniform is 1.0: the min() is a guard)
    assert ref.opening_index(below_one, 1) == 0
    assert ref.opening_index(0.0, 1) == 0 and ref.opening_index(0.5, 1) == 0
    assert ref.opening_index(0.0, 20) == 0 and ref.opening_index(0.5, 20) == 10


def test_pick_last_max():
    assert ref.pick_last_max([0, 3, 1, 3, 0]) == 3
    assert ref.pick_last_max([0, 0, 0]) is None
    assert ref.pick_last_max([]) is None


def _replay(ch, g, start=None):
    s = ch.ChessState() if start is None else ref.state_from_abi(start)
    for m in g["moves"]:
        assert s.status == ONGOING
        assert int(m) in s.valid_actions()
        s = s.next_state(int(m))
    return s


def test_moves_legal_and_results_consistent(ch):
    a, b = (EVAL_HASH, None, 8), (EVAL_UNIFORM, None, 12)
    games, stats = ref.oracle_match(a, b, 3, game_id_base=3, opening_plies=3, max_plies=20, seed=5)
    assert [g["game"] for g in games] == [3, 4, 5]
    assert [g["a_moves_first"] for g in games] == [False, True, False]
    for g in games:
        end = _replay(ch, g)
        assert g["n_moves"] == len(g["moves"]) <= 20
        assert g["status"] == end.status
        assert g["adjudicated"] == (end.status == ONGOING) and (not g["adjudicated"] or g["n_moves"] == 20)
    # games 4 and 5 are one pair: the same opening
    assert list(games[1]["moves"][:3]) == list(games[2]["moves"][:3])
    assert sum(stats["a_wins"]) + sum(stats["draws"]) + sum(stats["b_wins"]) == 3
    searched = [g["n_moves"] - 3 for g in games]
    # A plays the even searched plies of the even ids, the odd ones of the odd ids
    a_plies = sum((n + (1 if g["a_moves_first"] else 0)) // 2 for n, g in zip(searched, games))
    assert stats["sims"] == [8.0 * a_plies, 12.0 * (sum(searched) - a_plies)]
    assert stats["plies"] == sum(g["n_moves"] for g in games)


def test_identical_players_mirror_and_rerun(ch):
    p = (EVAL_HASH, None, 16)
    kw = dict(opening_plies=2, max_plies=24, seed=9)
    games, stats = ref.oracle_match(p, p, 4, **kw)
    for k in (0, 2):
        assert np.array_equal(games[k]["moves"], games[k + 1]["moves"])
        assert games[k]["result_a"] == -games[k + 1]["result_a"]
        assert games[k]["a_moves_first"] and not games[k + 1]["a_moves_first"]
    again, stats2 = ref.oracle_match(p, p, 4, **kw)
    assert stats == stats2
    for g, h in zip(games, again):
        assert np.array_equal(g["moves"], h["moves"]) and {k: v for k, v in g.items() if k != "moves"} == \
            {k: v for k, v in h.items() if k != "moves"}


def test_follow_replaces_only_before_second_players_first_search(ch):
    trace = []
    games, _ = ref.oracle_match((EVAL_HASH, None, 24), (EVAL_UNIFORM, None, 8), 2, opening_plies=2, max_plies=14,
                                seed=1, trace=trace)
    for g in games:
        tr = [t for t in trace if t["game"] == g["game"]]
        assert len(tr) >= 6
        # the first follow (after searched ply 0, game ply opening + 1) replaces the tree, no later one does
        assert [t["replaced"] for t in tr] == [True] + [False] * (len(tr) - 1)
        assert tr[0]["ply"] == 3
        for t in tr[1:]:
            assert t["root_visits_after"] == t["child_visits_before"]


def test_start_mate_in_one_is_won_for_the_mover(ch):
    st = start_of(ch, MATE_IN_ONE)
    s = ref.state_from_abi(st[0])
    assert len(s.valid_actions()) == 1 and s.next_state(s.valid_actions()[0]).status == WON
    games, stats = ref.oracle_match((EVAL_UNIFORM, None, 8), (EVAL_UNIFORM, None, 8), 2, opening_plies=0,
                                    max_plies=16, seed=0, start=st)
    for g in games:
        assert g["n_moves"] == 1 and g["status"] == WON and not g["adjudicated"]
        assert ch.uci(int(g["moves"][0])) == "d8f7"
    # the mover of ply 1: A in game 0, B in game 1
    assert [g["result_a"] for g in games] == [1, -1]
    assert stats["a_wins"] == [1.0, 0.0] and stats["b_wins"] == [0.0, 1.0]


def test_start_shuffle_is_tied_by_repetition(ch):
    st = start_of(ch, SHUFFLE)
    games, stats = ref.oracle_match((EVAL_HASH, None, 8), (EVAL_UNIFORM, None, 12), 2, opening_plies=0,
                                    max_plies=64, seed=0, start=st)
    for g in games:
        assert [ch.uci(int(m)) for m in g["moves"]] == ["h1g1", "h8g8", "g1h1", "g8h8"] * 2
        assert g["status"] == TIED and g["result_a"] == 0 and not g["adjudicated"]
        end = _replay(ch, g, start=st[0])
        assert end.repetitions() == 3 and end.st.fifty == 8
    assert stats["draws"] == [1.0, 1.0] and stats["adjudicated"] == 0


def test_max_plies_adjudicates_ongoing(ch):
    games, stats = ref.oracle_match((EVAL_HASH, None, 8), (EVAL_HASH, None, 8), 2, opening_plies=2, max_plies=6,
                                    seed=2)
    for g in games:
        assert g["adjudicated"] and g["status"] == ONGOING and g["result_a"] == 0 and g["n_moves"] == 6
    assert stats["adjudicated"] == 2 and stats["draws"] == [1.0, 1.0]


def test_start_rules(ch):
    with pytest.raises(ValueError):
        ref.oracle_match((EVAL_HASH, None, 8), (EVAL_HASH, None, 8), 1, opening_plies=1,
                         start=start_of(ch, SHUFFLE))
    mated = ref.state_from_abi(start_of(ch, MATE_IN_ONE)[0])
    mated = mated.next_state(mated.valid_actions()[0])
    with pytest.raises(ValueError):
        ref.oracle_match((EVAL_HASH, None, 8), (EVAL_HASH, None, 8), 1, opening_plies=0,
                         start=np.array([ref.abi_from_state(mated.st, STATE_DTYPE)], STATE_DTYPE))
    with pytest.raises(ref.MatchNaN):
        ref.oracle_match((EVAL_HASH, None, 1), (EVAL_HASH, None, 8), 1, opening_plies=0)
