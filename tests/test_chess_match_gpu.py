"""spai_chess_match_run on the MI355X (ChessEngine.match) against the two
restatements of tests/chess_match_ref.py: the CPU oracle's play() loop for the
stub evaluators (bit-exact: moves, results, status, adjudication, sims, evals),
and the one-tree-per-call loop over the older device API for bf16 nets (moves and
results).  1-block nets, at most 8 games and 48 simulations."""
import ctypes as C

import numpy as np
import pytest

import chess_match_ref as ref
from chess_match_ref import EVAL_HASH, EVAL_NET, EVAL_UNIFORM, MATE_IN_ONE, ONGOING, SHUFFLE, TIED, WON

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NAN = -1, -5   # SPAI_ERR_INVALID, SPAI_ERR_NAN


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


def start_of(ch, sc, fen, n=1):
    return np.array([ref.abi_from_state(ch.ChessState(fen=fen).st, sc.STATE_DTYPE)] * n, sc.STATE_DTYPE)


def same_games(got, want, stats=None, want_stats=None):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g["moves"], w["moves"]), (g["game"], list(g["moves"]), list(w["moves"]))
        for k in ("game", "a_moves_first", "result_a", "status", "adjudicated", "n_moves"):
            assert g[k] == w[k], (g["game"], k, g[k], w[k])
    if stats is not None:
        for k in ("a_wins", "draws", "b_wins", "sims", "evals", "adjudicated", "plies"):
            assert stats[k] == want_stats[k], (k, stats[k], want_stats[k])


STUB_CASES = [
    # a, b, n_games, game_id_base, opening_plies, max_plies
    ((EVAL_HASH, None, 8), (EVAL_HASH, None, 12), 1, 0, 2, 24),
    ((EVAL_HASH, None, 8), (EVAL_HASH, None, 12), 5, 0, 0, 24),
    ((EVAL_HASH, None, 24), (EVAL_UNIFORM, None, 24), 8, 0, 2, 24),
    ((EVAL_HASH, None, 8), (EVAL_UNIFORM, None, 12), 5, 6, 3, 24),
    ((EVAL_UNIFORM, None, 12), (EVAL_HASH, None, 8), 8, 3, 3, 24),
    ((EVAL_HASH, None, 24), (EVAL_HASH, None, 24), 1, 7, 0, 24),
]


@pytest.mark.parametrize("a,b,n,base,opening,max_plies", STUB_CASES)
def test_stub_players_match_oracle(ch, sc, a, b, n, base, opening, max_plies):
    eng = sc.ChessEngine(num_searches=24, max_trees=2 * n, eval_kind=sc.EVAL_HASH, max_moves=256)
    games, stats = eng.match(a, b, n, game_id_base=base, opening_plies=opening, max_plies=max_plies, seed=11)
    want, want_stats = ref.oracle_match(a, b, n, game_id_base=base, opening_plies=opening, max_plies=max_plies,
                                        seed=11)
    same_games(games, want, stats, want_stats)
    assert stats["seconds"] > 0
    eng.close()


def test_stub_games_to_their_natural_end(ch, sc):
    """max_plies = 0: 6 games at 8 simulations until Won or Tied (the shape of the
    self-play parity test), through compaction and long histories"""
    p = (EVAL_HASH, None, 8)
    eng = sc.ChessEngine(num_searches=8, max_trees=12, eval_kind=sc.EVAL_HASH, max_moves=2048)
    games, stats = eng.match(p, p, 6, opening_plies=2, max_plies=0, seed=21)
    want, want_stats = ref.oracle_match(p, p, 6, opening_plies=2, max_plies=0, seed=21)
    same_games(games, want, stats, want_stats)
    assert all(g["status"] != ONGOING and not g["adjudicated"] for g in games)
    eng.close()


def test_start_positions_won_and_tied(ch, sc):
    eng = sc.ChessEngine(num_searches=12, max_trees=8, eval_kind=sc.EVAL_HASH, max_moves=256)
    u = (EVAL_UNIFORM, None, 8)
    st = start_of(ch, sc, MATE_IN_ONE)
    games, stats = eng.match(u, u, 2, opening_plies=0, max_plies=16, start=st)
    want, want_stats = ref.oracle_match(u, u, 2, opening_plies=0, max_plies=16, start=st)
    same_games(games, want, stats, want_stats)
    assert [(g["n_moves"], g["status"], g["result_a"]) for g in games] == [(1, WON, 1), (1, WON, -1)]
    # two pairs with different starts, an odd base: game 3 is pair 1 (start[0]), games 4, 5 pair 2 (start[1])
    a, b = (EVAL_HASH, None, 8), (EVAL_UNIFORM, None, 12)
    st = np.concatenate([start_of(ch, sc, MATE_IN_ONE), start_of(ch, sc, SHUFFLE)])
    games, stats = eng.match(a, b, 3, game_id_base=3, opening_plies=0, max_plies=64, start=st)
    want, want_stats = ref.oracle_match(a, b, 3, game_id_base=3, opening_plies=0, max_plies=64, start=st)
    same_games(games, want, stats, want_stats)
    assert [(g["n_moves"], g["status"], g["result_a"]) for g in games] == [(1, WON, -1), (8, TIED, 0), (8, TIED, 0)]
    eng.close()


def _nets(sc, eng, seeds, blocks=1):
    return [sc.ChessNet(eng, blocks, sc.init_params(blocks, s)) for s in seeds]


NET_CASES = ["net_vs_net", "net_vs_uniform", "same_net"]


@pytest.mark.parametrize("case", NET_CASES)
def test_net_players_match_device_loop(ch, sc, case):
    """bf16 nets: the match (many trees per forward, two streams) plays the games of
    the one-tree-per-call loop, i.e. the forward is invariant to its batch"""
    n, sims, max_plies = 4, 16, 16
    eng = sc.ChessEngine(num_searches=sims, max_trees=2 * n, eval_kind=sc.EVAL_UNIFORM, max_moves=256)
    pa, pb = sc.init_params(1, 3), sc.init_params(1, 4)
    na, nb = _nets(sc, eng, (3, 4))
    if case == "net_vs_net":
        a, b = (EVAL_NET, na, sims), (EVAL_NET, nb, sims)
        ra, rb = (EVAL_NET, pa, sims), (EVAL_NET, pb, sims)
    elif case == "net_vs_uniform":
        a, b = (EVAL_NET, na, sims), (EVAL_UNIFORM, None, sims)
        ra, rb = (EVAL_NET, pa, sims), (EVAL_UNIFORM, None, sims)
    else:
        a, b = (EVAL_NET, na, sims), (EVAL_NET, na, sims)
        ra, rb = (EVAL_NET, pa, sims), (EVAL_NET, pa, sims)
    games, stats = eng.match(a, b, n, opening_plies=2, max_plies=max_plies, seed=5)
    want, want_stats = ref.device_match(sc, ra, rb, n, opening_plies=2, max_plies=max_plies, seed=5, max_moves=256)
    same_games(games, want)
    assert stats["sims"] == want_stats["sims"]
    for g in games:   # and every move is legal
        s = ch.ChessState()
        for m in g["moves"]:
            assert int(m) in s.valid_actions()
            s = s.next_state(int(m))
    na.close()
    nb.close()
    eng.close()


def test_identical_net_players_mirror_and_repeat(ch, sc):
    n, sims = 4, 16
    eng = sc.ChessEngine(num_searches=sims, max_trees=2 * n, eval_kind=sc.EVAL_HASH, max_moves=256)
    net, = _nets(sc, eng, (7,))
    p = (EVAL_NET, net, sims)
    games, stats = eng.match(p, p, n, opening_plies=2, max_plies=16, seed=2)
    for k in (0, 2):
        assert np.array_equal(games[k]["moves"], games[k + 1]["moves"])
        assert games[k]["result_a"] == -games[k + 1]["result_a"]
    again, stats2 = eng.match(p, p, n, opening_plies=2, max_plies=16, seed=2)
    same_games(again, games, stats2, stats)
    net.close()
    eng.close()


@pytest.mark.parametrize("sa,sb", [(4, 40), (40, 4)])
def test_unequal_and_empty_chains(ch, sc, sa, sb):
    """n_games = 1: one chain is empty at every ply; 3 games: both run, 10x apart in length"""
    eng = sc.ChessEngine(num_searches=40, max_trees=6, eval_kind=sc.EVAL_NET, max_moves=256)
    a, b = (EVAL_HASH, None, sa), (EVAL_UNIFORM, None, sb)
    for n in (1, 3):
        games, stats = eng.match(a, b, n, game_id_base=1, opening_plies=2, max_plies=12, seed=4)
        want, want_stats = ref.oracle_match(a, b, n, game_id_base=1, opening_plies=2, max_plies=12, seed=4)
        same_games(games, want, stats, want_stats)
    eng.close()


def test_one_stream_schedule_plays_the_same_games(sc):
    """spai_chess_match_set_one_stream changes where the chains run, not what they compute"""
    n, sims = 4, 16
    eng = sc.ChessEngine(num_searches=sims, max_trees=2 * n, eval_kind=sc.EVAL_HASH, max_moves=256)
    na, nb = _nets(sc, eng, (3, 4))
    a, b = (EVAL_NET, na, sims), (EVAL_NET, nb, 12)
    games, stats = eng.match(a, b, n, game_id_base=1, opening_plies=2, max_plies=16, seed=6)
    eng.match_one_stream(True)
    one, stats1 = eng.match(a, b, n, game_id_base=1, opening_plies=2, max_plies=16, seed=6)
    eng.match_one_stream(False)
    two, stats2 = eng.match(a, b, n, game_id_base=1, opening_plies=2, max_plies=16, seed=6)
    same_games(one, games, stats1, stats)
    same_games(two, games, stats2, stats)
    na.close()
    nb.close()
    eng.close()


def test_one_search_has_no_move_to_play(sc):
    eng = sc.ChessEngine(num_searches=8, max_trees=4, eval_kind=sc.EVAL_HASH, max_moves=256)
    one, p = (EVAL_HASH, None, 1), (EVAL_HASH, None, 8)
    for a, b in ((one, p), (p, one)):
        with pytest.raises(sc.SpaiError) as ei:
            eng.match(a, b, 2, opening_plies=2, max_plies=8)
        assert ei.value.code == ERR_NAN
    games, _ = eng.match(p, p, 2, opening_plies=2, max_plies=8)   # the engine stays usable
    assert all(g["n_moves"] == 8 for g in games)
    eng.close()


def _raw_match(sc, eng, a, b, n_games, cfg, moves=None):
    pl = [sc.ChessMatchPlayer(int(k), int(s), net.h if net is not None else None) for k, net, s in (a, b)]
    return sc.lib().spai_chess_match_run(eng.h, C.byref(pl[0]), C.byref(pl[1]), n_games, 0, C.byref(cfg), None,
                                         moves, None)


def test_validation(ch, sc):
    eng = sc.ChessEngine(num_searches=8, max_trees=4, eval_kind=sc.EVAL_HASH, max_moves=256)
    other = sc.ChessEngine(num_searches=8, max_trees=4, eval_kind=sc.EVAL_HASH, max_moves=256)
    foreign, = _nets(sc, other, (1,))
    p = (EVAL_HASH, None, 8)

    def invalid(**kw):
        args = dict(a=p, b=p, n_games=2, opening_plies=2, max_plies=8)
        args.update(kw)
        with pytest.raises(sc.SpaiError) as ei:
            eng.match(args.pop("a"), args.pop("b"), args.pop("n_games"), **args)
        assert ei.value.code == ERR_INVALID, kw

    invalid(start=start_of(ch, sc, SHUFFLE), opening_plies=1)        # start together with an opening
    mated = ch.ChessState(fen=MATE_IN_ONE)
    mated = mated.next_state(mated.valid_actions()[0])
    invalid(start=np.array([ref.abi_from_state(mated.st, sc.STATE_DTYPE)], sc.STATE_DTYPE), opening_plies=0)
    kingless = start_of(ch, sc, SHUFFLE)
    kingless["pieces"][0, 5] &= kingless["colors"][0, 0]             # Black's king off the board
    kingless["colors"][0, 1] &= ~np.uint64(1 << 63)
    invalid(start=kingless, opening_plies=0)
    invalid(opening_plies=4)
    invalid(n_games=3)                                               # 6 trees > max_trees 4
    invalid(a=(EVAL_HASH, None, 0))
    invalid(b=(EVAL_HASH, None, 9))                                  # > cfg.num_searches
    invalid(a=(EVAL_NET, None, 8))
    invalid(b=(EVAL_NET, foreign, 8))
    cfg = sc.ChessMatchConfig()
    assert sc.lib().spai_chess_match_config_default(C.byref(cfg)) == 0
    assert (cfg.struct_size, cfg.opening_plies, cfg.max_plies, cfg.moves_stride, cfg.seed, cfg.start) == \
        (C.sizeof(sc.ChessMatchConfig), 2, 512, 0, 0, None)
    cfg.max_plies = 6
    cfg.struct_size -= 8                                             # a client built from another header
    assert _raw_match(sc, eng, p, p, 2, cfg) == ERR_INVALID
    cfg.struct_size += 8
    buf = np.full((3, 4), 0xFFFF, np.uint16)                         # [n_games][moves_stride] and a guard row
    assert _raw_match(sc, eng, p, p, 2, cfg, buf.ctypes.data_as(C.c_void_p)) == ERR_INVALID   # moves, stride 0
    cfg.moves_stride = 4                                             # shorter than the games: the first 4 codes
    assert _raw_match(sc, eng, p, p, 2, cfg, buf.ctypes.data_as(C.c_void_p)) == 0
    games, _ = eng.match(p, p, 2, opening_plies=2, max_plies=6)
    for g, row in zip(games, buf):
        assert g["n_moves"] == 6 and np.array_equal(row, g["moves"][:4])
    assert np.all(buf[2] == 0xFFFF)
    foreign.close()
    other.close()
    eng.close()


def _stub_self_play(eng):
    games, stats = eng.self_play(3)
    return [(g["game"], g["moves"].tobytes(), g["value"].tobytes(), g["policy"].tobytes()) for g in games], \
        {k: v for k, v in stats.items() if k != "seconds"}


def test_self_play_is_undisturbed(sc):
    """after a match of other evaluators, and after a failed match call, the engine's
    own self-play (its cfg.eval, net, temperature, timers) is a fresh engine's"""
    kw = dict(num_searches=8, max_trees=4, eval_kind=sc.EVAL_HASH, seed=3, max_moves=2048)
    fresh = sc.ChessEngine(**kw)
    fresh.set_timing(True)
    want = _stub_self_play(fresh)
    want_t = fresh.timing()
    eng = sc.ChessEngine(**kw)
    eng.set_timing(True)
    net, = _nets(sc, eng, (2,))
    eng.match((EVAL_NET, net, 8), (EVAL_UNIFORM, None, 6), 2, opening_plies=2, max_plies=10)
    assert not any(x.any() for x in eng.timing()[1:])       # nothing sampled by the match
    with pytest.raises(sc.SpaiError):
        eng.match((EVAL_HASH, None, 1), (EVAL_HASH, None, 8), 2)
    with pytest.raises(sc.SpaiError):
        eng.match((EVAL_HASH, None, 8), (EVAL_HASH, None, 8), 3)
    assert _stub_self_play(eng) == want
    got_t = eng.timing()
    assert np.array_equal(got_t[1], want_t[1]) and np.array_equal(got_t[2], want_t[2])   # launches, items
    net.close()
    for e in (fresh, eng):
        e.close()


def test_tree_children(sc):
    eng = sc.ChessEngine(num_searches=48, max_trees=3, eval_kind=sc.EVAL_HASH, max_moves=256)
    eng.trees_create(3)
    mv, vis = eng.tree_children(1)
    assert len(mv) == 0 and len(vis) == 0                   # a fresh tree: root not expanded
    _, _, svis, smv, nc = eng.search([1, 2], 48)
    for i, t in enumerate((1, 2)):
        mv, vis = eng.tree_children(t)
        assert len(mv) == nc[i] == 20
        assert np.array_equal(mv, smv[i, :nc[i]]) and np.array_equal(vis, svis[i, :nc[i]].astype(np.uint32))
        assert vis.sum() == 47
        mv2, vis2 = eng.tree_children(t)                    # reading changes nothing
        assert np.array_equal(mv, mv2) and np.array_equal(vis, vis2)
    assert len(eng.tree_children(0)[0]) == 0
    with pytest.raises(sc.SpaiError):
        eng.tree_children(3)
    eng.close()
