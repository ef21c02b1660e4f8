"""CPU restatement of a Connect4 match between two evaluators (spai_match_run,
include/spai.h "match"), from the oracle's primitives alone: or_tree_with_root,
or_search on tree handles with an eval kind and net per call, or_tree_use_subtree,
or_tree_node_info, or_c4_next_state and or_u01_f32.  One game at a time, one
search call per move: play() of main.rs:54-135 with a second evaluator where the
human sits.

A player is (eval_kind, oracle.Net or None, num_searches); in the net's place a
callable (user, n, states, priors, values) evaluates that player's leaves instead
(oracle.search_c4's eval_fn), whatever the eval kind.
"""
import ctypes as C

import numpy as np

import oracle as orc


class MatchNaN(RuntimeError):
    """NaN UCB, or no visited root child to play (the device's SPAI_ERR_NAN)"""


def opening_index(u, n_legal):
    """idx = min((int)(u * (float)n_legal), n_legal - 1), the product one f32 multiply"""
    return min(int(np.float32(u) * np.float32(n_legal)), n_legal - 1)


def opening_moves(seed, pair, plies):
    """the opening of a pair of games: ply k plays the idx-th legal column in
    ascending order, u the Philox uniform keyed (seed, pair, k)"""
    s = orc.C4()
    moves = []
    for k in range(plies):
        legal = s.valid_actions()
        a = legal[opening_index(orc.lib().or_u01_f32(seed, pair, k), len(legal))]
        moves.append(a)
        s = s.next_state(a)
    return moves, s


def root_info(tree):
    """(visits, children ids, their actions) of the tree's root (id 0)"""
    L = orc.lib()
    par, act, nch = C.c_int(), C.c_int(), C.c_int()
    pri, w = C.c_float(), C.c_float()
    vis = C.c_uint32()
    ch = (C.c_int * 9)()
    L.or_tree_node_info(tree, 0, C.byref(par), C.byref(act), C.byref(pri), C.byref(vis), C.byref(w), C.byref(nch), ch)
    kids = [int(ch[i]) for i in range(nch.value)]
    acts = []
    for k in kids:
        ka = C.c_int()
        L.or_tree_node_info(tree, k, C.byref(par), C.byref(ka), C.byref(pri), C.byref(C.c_uint32()), C.byref(w),
                            C.byref(C.c_int()), (C.c_int * 9)())
        acts.append(ka.value)
    return vis.value, kids, acts


def node_visits(tree, node):
    L = orc.lib()
    vis = C.c_uint32()
    L.or_tree_node_info(tree, node, C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_float()), C.byref(vis),
                        C.byref(C.c_float()), C.byref(C.c_int()), (C.c_int * 9)())
    return vis.value


def play_game(game_id, players, opening_plies, seed, c=2.0, trace=None):
    """One game.  players = (A, B); A moves first when game_id is even.  Returns a dict
    (game, a_moves_first, result_a, moves, sims [2], evals [2]).  trace: a list that
    receives one dict per move (mover, opponent tree replaced or re-rooted, and the
    opponent root's visits after against the child's before)."""
    L = orc.lib()
    moves, state = opening_moves(seed, game_id // 2, opening_plies)
    assert state.status == orc.ONGOING
    trees = [L.or_tree_with_root(orc.GAME_CONNECT4, C.byref(state.st)) for _ in players]
    sims, evals = [0, 0], [0, 0]
    result = 0
    try:
        while state.status == orc.ONGOING:
            p = (game_id ^ state.n) & 1          # A (0) moves at the plies of the id's parity
            kind, net, ns = players[p]
            fn = net if callable(net) else None
            rc, _pol, ids, vis, nc = orc.search_c4(None, ns, eval_kind=kind, net=None if fn else net, c=c,
                                                   trees=[trees[p]], eval_fn=fn)
            if rc < 0:
                raise MatchNaN("NaN UCB")
            sims[p] += ns
            evals[p] += rc
            n = int(nc[0])
            v = vis[0, :n]
            if n == 0 or not (v > 0).any():
                raise MatchNaN("no visited root child")
            idx = n - 1 - int(np.argmax(v[::-1]))          # the last maximum
            a = state.valid_actions()[idx]
            L.or_tree_use_subtree(trees[p], int(ids[0, idx]))
            state = state.next_state(a)
            moves.append(a)
            q = p ^ 1                                      # the opponent's tree follows the action
            _rv, kids, acts = root_info(trees[q])
            step = dict(mover=p, action=a, replaced=not kids)
            if kids:
                child = kids[acts.index(a)]
                step["child_visits_before"] = node_visits(trees[q], child)
                L.or_tree_use_subtree(trees[q], child)
                step["root_visits_after"] = root_info(trees[q])[0]
            else:
                L.or_tree_destroy(trees[q])
                trees[q] = L.or_tree_with_root(orc.GAME_CONNECT4, C.byref(state.st))
            if trace is not None:
                trace.append(step)
            if state.status == orc.WON:
                result = 1 if p == 0 else -1
    finally:
        for t in trees:
            L.or_tree_destroy(t)
    return dict(game=game_id, a_moves_first=game_id % 2 == 0, result_a=result, moves=moves, sims=sims, evals=evals)


def play_match(a, b, n_games, opening_plies, seed, game_id_base=0, c=2.0):
    """(games, stats) in Engine.match's shape (without seconds)"""
    games = [play_game(game_id_base + g, (a, b), opening_plies, seed, c) for g in range(n_games)]
    stats = {k: [0.0, 0.0] for k in ("a_wins", "draws", "b_wins", "sims", "evals")}
    for g in games:
        f = 0 if g["a_moves_first"] else 1
        stats["a_wins" if g["result_a"] > 0 else "b_wins" if g["result_a"] < 0 else "draws"][f] += 1
        for p in range(2):
            stats["sims"][p] += g["sims"][p]
            stats["evals"][p] += g["evals"][p]
    return [{k: g[k] for k in ("game", "a_moves_first", "result_a", "moves")} for g in games], stats
