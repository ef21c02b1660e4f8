"""Compact chess self-play samples on the host (spai_chess_sample, ChessSamples,
spai_chess_samples_expand): no device is needed, libspai.so loads without one.

The yardstick runs none of the library's code: the planes are the CPU oracle's
orc_encoding of the position (which counts the repetitions from the state's own
history), the policy row is numpy float32 visits / visits.sum() scattered through
the oracle's policy_index.  Positions: the 24 of chess_search_ref.positions() (both
colours, roots that stand a second time, lost castling rights, promotions, en
passant), a position with 218 legal moves (the most any position has) and one with
a single legal move.  Visit counts are random and include zeros."""
import numpy as np
import pytest

import chessref as ch
from chess_compact_ref import make_samples, positions, reference, take


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    spai_chess.lib()
    return spai_chess


@pytest.fixture(scope="module")
def case(sc):
    states = positions()
    cs, moves, visits = make_samples(sc, states)
    return states, cs, moves, visits, reference(states, moves, visits)


def test_symbols_and_layout(sc):
    import spai
    for name in ("spai_chess_selfplay_compact", "spai_chess_samples_expand", "spai_chess_learner_train_batch_compact",
                 "spai_chess_learner_train_compact", "spai_chess_learner_batch"):
        assert spai.SYMBOLS.count(name) == 1 and hasattr(sc.lib(), name), name
    assert sc.SAMPLE_DTYPE.itemsize == 96 and sc.SAMPLE_DTYPE.fields["value"][1] == 80


def test_positions_cover_the_extremes(case):
    states, _, moves, visits, _ = case
    assert len(moves[24]) == 218 and len({ch.policy_index(0, int(m)) for m in moves[24]}) == 218
    assert len(moves[25]) == 1 and states[25].side == 1
    assert {s.side for s in states} == {0, 1}
    assert sum(s.repetitions() == 2 for s in states) >= 7
    assert any((v == 0).any() for v in visits)
    for s, mv in zip(states, moves):   # a legal move list never maps two moves to one index
        assert len({ch.policy_index(s.side, int(m)) for m in mv}) == len(mv)


def test_expand_equals_oracle_and_numpy(case):
    states, cs, _, _, (enc, pol) = case
    e, p, v = cs.expand()
    assert e.dtype == p.dtype == v.dtype == np.float32
    assert np.array_equal(e.view(np.uint32), enc.view(np.uint32))
    assert np.array_equal(p.view(np.uint32), pol.view(np.uint32))   # the zeros are +0.0 too
    assert np.array_equal(v, cs.samples["value"])
    assert len(cs) == 26 and cs.nbytes == 26 * 96 + 6 * len(cs.child_moves)
    assert cs.nbytes * 40 < e.nbytes + p.nbytes + v.nbytes


def test_expand_of_a_repeated_set_is_tiled(case):
    _, cs, _, _, (enc, pol) = case
    r = cs.with_repeat(3)
    e, p, v = r.expand()
    assert len(r) == 78 and r.n == 26 and r.nbytes == cs.nbytes
    assert np.array_equal(e, np.tile(enc, (3, 1))) and np.array_equal(p, np.tile(pol, (3, 1)))
    assert np.array_equal(v, np.tile(cs.samples["value"], 3)) and np.array_equal(r.game, np.tile(cs.game, 3))


def _one(sc, cs, i, **change):
    """sample i alone, with fields of its state or record changed"""
    s = cs.samples[i:i + 1].copy()
    f, k = int(s["first"][0]), int(s["n_children"][0])
    mv, vis = cs.child_moves[f:f + k].copy(), cs.child_visits[f:f + k].copy()
    s["first"] = 0
    for name, val in change.items():
        if name == "drop":
            mv, vis = np.delete(mv, val), np.delete(vis, val)
            s["n_children"] = k - 1
        else:
            s["state"][name] = val
    return sc.ChessSamples(s, mv, vis)


def test_reference_reacts_to_errors(sc, case):
    """the yardstick tells a wrong expansion from a right one: a swapped side, a repetition
    plane forced to 1 and a dropped child each leave its rows"""
    states, cs, _, visits, (enc, pol) = case
    for i in (0, 1, 2, 12, 24):
        e, p, _ = _one(sc, cs, i).expand()
        assert np.array_equal(e[0], enc[i]) and np.array_equal(p[0], pol[i])
        e, p, _ = _one(sc, cs, i, side=1 - states[i].side).expand()
        assert not np.array_equal(p[0], pol[i])
        assert i in (0, 2) or not np.array_equal(e[0], enc[i])   # 0, 2: the start position, its own mirror image
        k = int(np.flatnonzero(visits[i])[0])
        e, p, _ = _one(sc, cs, i, drop=k).expand()
        assert np.array_equal(e[0], enc[i]) and not np.array_equal(p[0], pol[i])
    rep2 = [i for i, s in enumerate(states) if s.repetitions() == 2]
    for i in rep2:
        e, p, _ = _one(sc, cs, i, reps=1).expand()
        assert not np.array_equal(e[0], enc[i]) and np.array_equal(p[0], pol[i])
        assert np.array_equal(np.flatnonzero(e[0] != enc[i]), np.arange(16 * 64, 17 * 64))


def _pair(sc, cs):
    """samples 3 and 4 as a set of two: index 1 is the one the cases below break"""
    a, b = _one(sc, cs, 3), _one(sc, cs, 4)
    return sc.ChessSamples.concat([sc.ChessSamples(a.samples, a.child_moves, a.child_visits, [0]),
                                   sc.ChessSamples(b.samples, b.child_moves, b.child_visits, [1])])


def _rejected(sc, cs, *words):
    with pytest.raises(sc.SpaiError) as ei:
        cs.expand()
    assert ei.value.code == -1, ei.value
    msg = str(ei.value)
    for w in ("sample 1",) + words:
        assert w in msg, (w, msg)


def test_validation_rules(sc, case):
    _, cs, _, _, _ = case
    good = _pair(sc, cs)
    good.expand()
    f = int(good.samples["first"][1])

    def broken():
        return sc.ChessSamples(good.samples.copy(), good.child_moves.copy(), good.child_visits.copy())

    for n in (0, 257):
        b = broken()
        b.samples["n_children"][1] = n
        _rejected(sc, b, "n_children")
    b = broken()
    b.samples["first"][1] = len(b.child_moves) - int(b.samples["n_children"][1]) + 1
    _rejected(sc, b, "first", "n_children_total")
    b = broken()
    b.samples["first"][1] = 0xFFFFFFFF
    _rejected(sc, b, "first")
    b = broken()                                 # no white king
    st = b.samples["state"][1]
    king = st["pieces"][5] & st["colors"][0]
    b.samples["state"]["pieces"][1][5] &= ~king
    b.samples["state"]["colors"][1][0] &= ~king
    _rejected(sc, b, "king")
    b = broken()                                 # a second black king on an empty square
    occ = int(st["colors"][0] | st["colors"][1])
    sq = next(s for s in range(64) if not (occ >> s) & 1)
    b.samples["state"]["pieces"][1][5] |= np.uint64(1 << sq)
    b.samples["state"]["colors"][1][1] |= np.uint64(1 << sq)
    _rejected(sc, b, "king")
    b = broken()
    b.samples["state"]["side"][1] = 2
    _rejected(sc, b, "side")
    b = broken()                                 # h7a8 promoting to a rook: channel fd + 1 = -6
    b.child_moves[f] = ch.move(ch.sq("h7"), ch.sq("a8"), ch.ROOK)
    assert ch.policy_index(0, int(b.child_moves[f])) < 0
    _rejected(sc, b, "child_moves", "policy index")
    b = broken()
    b.child_moves[f + 1] = b.child_moves[f]
    _rejected(sc, b, "child_moves", "shares")
    b = broken()
    b.child_visits[f:] = 0
    _rejected(sc, b, "child_visits", "sum")
    b = broken()
    b.child_visits[f:] = 0
    b.child_visits[f] = 1 << 24
    _rejected(sc, b, "child_visits", "sum")
    b = broken()                                 # the largest sum that passes
    b.child_visits[f:] = 0
    b.child_visits[f], b.child_visits[f + 1] = (1 << 24) - 2, 1
    _, p, _ = b.expand()
    tot = np.float32((1 << 24) - 1)
    assert sorted(p[1][p[1] != 0]) == [np.float32(1) / tot, np.float32((1 << 24) - 2) / tot]


def test_concat_round_trips(sc, case):
    _, cs, _, _, (enc, pol) = case
    games = [sc.ChessSamples.concat([_with_game(sc, _one(sc, cs, i), cs.game[i])
                                     for i in range(len(cs)) if cs.game[i] == g]) for g in range(13)]
    assert all(q.n == 2 and list(q.samples["first"]) == [0, int(q.samples["n_children"][0])] for q in games)
    order = np.random.default_rng(5).permutation(13)
    back = sc.ChessSamples.concat([games[g] for g in order])
    assert np.array_equal(back.samples, cs.samples) and np.array_equal(back.game, cs.game)
    assert np.array_equal(back.child_moves, cs.child_moves) and np.array_equal(back.child_visits, cs.child_visits)
    e, p, _ = back.expand()
    assert np.array_equal(e, enc) and np.array_equal(p, pol)
    assert len(sc.ChessSamples.concat([])) == 0
    idx = [25, 3, 3, 24, 0]
    a, b = cs.take(idx), take(sc, cs, idx)
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.game, cs.game[idx])
    assert np.array_equal(a.child_moves, b.child_moves) and np.array_equal(a.child_visits, b.child_visits)
    assert np.array_equal(a.expand()[1], pol[idx])


def _with_game(sc, q, g):
    return sc.ChessSamples(q.samples, q.child_moves, q.child_visits, np.full(q.n, g))


def test_learn_loop_defaults_are_the_dense_route():
    """learn_loop's default hooks build what the loop built before it had hooks"""
    import spai_learn as SL
    rng = np.random.default_rng(1)
    games = [dict(game=g, enc=rng.random((n, 5), np.float32), policy=rng.random((n, 3), np.float32),
                  value=rng.random(n, np.float32)) for g, n in ((7, 2), (3, 4), (5, 1))]
    part = SL._gather(games)
    by_id = sorted(games, key=lambda g: g["game"])
    assert np.array_equal(part[0], np.concatenate([g["enc"] for g in by_id]))
    assert list(part[3]) == [3, 3, 3, 3, 5, 7, 7]
    args, seen = SL._join([part, part], 3)
    for k in range(3):
        assert np.array_equal(args[k], np.concatenate([part[k], part[k]] * 3)) and args[k] is seen[k]
    assert np.array_equal(seen[3], np.tile(part[3], 6))
