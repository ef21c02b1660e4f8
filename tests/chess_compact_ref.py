"""Compact chess self-play samples for the tests: the positions, a ChessSamples over
them with random visit counts, and the dense form they stand for, computed with
none of the library's code (tests/test_chess_compact_samples_cpu.py says how)."""
import numpy as np

import chess_search_ref as SR
import chessref as ch
from chess_match_ref import abi_from_state

FEN_218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
FEN_ONE = "k7/8/1K6/8/8/8/8/7R b - - 0 1"


def positions():
    """the 26 ChessStates, all ongoing"""
    out = [s for _, _, s in SR.positions()]
    out += [ch.ChessState(fen=FEN_218, made=0, fifty=0), ch.ChessState(fen=FEN_ONE, made=0, fifty=0)]
    assert len(out) == 26 and all(s.status == 0 for s in out)
    return out


def make_samples(sc, states, seed=0):
    """a ChessSamples over `states` with random visit counts (about a quarter of them 0, never
    all), values in {-1, 0, 1} and game ids 0, 0, 1, 1, ...; and what it was made of"""
    rng = np.random.default_rng(seed)
    smp = np.zeros(len(states), sc.SAMPLE_DTYPE)
    moves, visits = [], []
    for i, s in enumerate(states):
        mv = s.valid_actions()
        vis = rng.integers(0, 40, len(mv)) * (rng.random(len(mv)) > 0.25)
        vis[rng.integers(len(mv))] = rng.integers(1, 40)
        st = abi_from_state(s.st, sc.STATE_DTYPE)
        st["reps"] = s.repetitions()
        smp[i]["state"] = st
        smp[i]["value"] = rng.choice([-1.0, 0.0, 1.0])
        smp[i]["move"] = mv[int(rng.integers(len(mv)))]
        smp[i]["n_children"] = len(mv)
        smp[i]["first"] = sum(len(m) for m in moves)
        moves.append(np.array(mv, np.uint16))
        visits.append(vis.astype(np.uint32))
    cs = sc.ChessSamples(smp, np.concatenate(moves), np.concatenate(visits), np.arange(len(states)) // 2)
    return cs, moves, visits


def reference(states, moves, visits):
    """(enc, policy) by the oracle and numpy alone"""
    enc = np.stack([s.encoding().reshape(-1) for s in states])
    pol = np.zeros((len(states), ch.POLICY), np.float32)
    for i, s in enumerate(states):
        v = visits[i].astype(np.float32)
        p = v / v.sum(dtype=np.float32)
        for m, x in zip(moves[i], p):
            pol[i, ch.policy_index(s.side, int(m))] = x
    return enc, pol


def take(sc, cs, idx):
    """the samples idx of cs, in that order, as a set of their own (game id = position in idx)"""
    smp = cs.samples[np.asarray(idx)].copy()
    mv = [cs.child_moves[int(f):int(f) + int(k)] for f, k in zip(smp["first"], smp["n_children"])]
    vis = [cs.child_visits[int(f):int(f) + int(k)] for f, k in zip(smp["first"], smp["n_children"])]
    nch = smp["n_children"].astype(np.int64)
    smp["first"] = np.cumsum(nch) - nch
    return sc.ChessSamples(smp, np.concatenate(mv), np.concatenate(vis), np.arange(len(smp)))
