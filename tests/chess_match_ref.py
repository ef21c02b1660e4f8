"""Two restatements of spai_chess_match_run (include/spai.h "chess match"), the
yardsticks of tests/test_chess_match_gpu.py.  Neither runs any code of the match.

oracle_match   play() (main.rs:54-135) over the CPU oracle's primitives
               (oracle/chessref.py): one game at a time, one search per move, the
               opponent's tree followed as main.rs:92 does it.  Bit-exact for the
               stub evaluators (HASH: the oracle's own; UNIFORM: a callback).
device_match   the same loop over the device API that predates the match: one
               ChessEngine per player, search([t]) then advance, one tree per
               call.  The yardstick for bf16 nets, where no CPU oracle is bit-exact.

Both return (games, stats) in ChessEngine.match's format.
"""
import ctypes as C

import numpy as np

import chessref
import oracle as _oracle

EVAL_NET, EVAL_UNIFORM, EVAL_HASH = 0, 1, 2
ONGOING, TIED, WON = 0, 1, 2
POLICY = chessref.POLICY

# start positions of the two fixed cases (verified in tests/test_chess_match_ref_cpu.py)
# the only legal move, Nd8xf7, is a smothered mate
MATE_IN_ONE = "3N2rk/5qpp/8/8/8/8/4P1P1/4RKR1 w - - 0 1"
# each side's only legal move shuffles its king between two squares (the shape of
# g1f3 g8f6 f3g1 f6g8 ...): the start position stands a third time after ply 8
SHUFFLE = "5b1k/4p1p1/4P1P1/8/8/4p1p1/4P1P1/5B1K w - - 0 1"


class MatchNaN(Exception):
    """a root without a visited child, or a NaN UCB: SPAI_ERR_NAN on the device"""


def opening_index(u, n_legal):
    """idx = min((int)(u * (float)n_legal), n_legal - 1), the product rounded to f32"""
    return min(int(np.float32(u) * np.float32(n_legal)), n_legal - 1)


def pick_last_max(visits):
    """the most-visited child, ties to the last; None when none was visited"""
    best, idx = 0, None
    for k, v in enumerate(visits):
        if v > 0 and v >= best:
            best, idx = v, k
    return idx


def state_from_abi(rec):
    """spai_chess_state record (spai_chess.STATE_DTYPE) -> ChessState with an empty table"""
    b = chessref.Board()
    for i in range(6):
        b.pieces[i] = int(rec["pieces"][i])
    b.color[0], b.color[1] = int(rec["colors"][0]), int(rec["colors"][1])
    b.side = int(rec["side"])
    b.castle[0], b.castle[1] = int(rec["castle"]) & 3, (int(rec["castle"]) >> 2) & 3
    b.ep = int(rec["ep"])
    s = chessref.ChessState()
    chessref.lib().orc_state_from_board(C.byref(s.st), C.byref(b), int(rec["made"]), int(rec["fifty"]))
    return s


def abi_from_state(st, dtype):
    """oracle State (ctypes) -> spai_chess_state record"""
    a = np.zeros(1, dtype)
    b = st.b
    a["pieces"] = [b.pieces[i] for i in range(6)]
    a["colors"] = [b.color[0], b.color[1]]
    a["side"] = b.side
    a["castle"] = b.castle[0] | (b.castle[1] << 2)
    a["ep"] = b.ep
    a["fifty"] = st.fifty
    a["made"] = st.made
    return a[0]


def _same_board(x, y):
    return (all(x.pieces[i] == y.pieces[i] for i in range(6)) and x.color[0] == y.color[0] and
            x.color[1] == y.color[1] and x.side == y.side and x.castle[0] == y.castle[0] and
            x.castle[1] == y.castle[1] and x.ep == y.ep)


def _uniform_eval(user, n, states, priors, values):
    """Model::predict of a net that answers ones and 0: mask_invalid(ones), value 0"""
    pri = np.ctypeslib.as_array(priors, (n * POLICY,))
    ones = np.ones(POLICY, np.float32)
    for k in range(n):
        pri[k * POLICY:(k + 1) * POLICY] = chessref.ChessState(st=states[k].contents).mask_invalid(ones)
        values[k] = 0.0


_UNIFORM = chessref.EVAL_FN(_uniform_eval)
_HASH = chessref.EVAL_FN()   # NULL: the oracle's hash stub


def _lib():
    L = chessref.lib()
    _oracle.lib()
    return L


def _root_stats(L, tree):
    """(child ids, visits, moves) of a tree's root: a search of 0 iterations"""
    arr = (C.c_void_p * 1)(tree)
    ids = np.zeros(chessref.MAX_MOVES, np.int32)
    vis = np.zeros(chessref.MAX_MOVES, np.float32)
    mv = np.zeros(chessref.MAX_MOVES, np.int32)
    nc = np.zeros(1, np.int32)
    ip = C.POINTER(C.c_int)
    rc = L.orc_search(arr, 1, 0, 2.0, _HASH, None, None, ids.ctypes.data_as(ip), chessref._f(vis),
                      mv.ctypes.data_as(ip), nc.ctypes.data_as(ip))
    assert rc == 0
    n = int(nc[0])
    return ids[:n], vis[:n], mv[:n]


def _search(L, tree, sims, kind, c):
    arr = (C.c_void_p * 1)(tree)
    ids = np.zeros(chessref.MAX_MOVES, np.int32)
    vis = np.zeros(chessref.MAX_MOVES, np.float32)
    mv = np.zeros(chessref.MAX_MOVES, np.int32)
    nc = np.zeros(1, np.int32)
    ip = C.POINTER(C.c_int)
    fn = {EVAL_HASH: _HASH, EVAL_UNIFORM: _UNIFORM}[kind]
    rc = L.orc_search(arr, 1, sims, c, fn, None, None, ids.ctypes.data_as(ip), chessref._f(vis),
                      mv.ctypes.data_as(ip), nc.ctypes.data_as(ip))
    if rc < 0:
        raise MatchNaN("NaN UCB")
    n = int(nc[0])
    return rc, ids[:n], vis[:n], mv[:n]


def opening_state(start_state, seed, pair, plies):
    """the position after the opening and the moves that lead to it"""
    s, moves = start_state, []
    for k in range(plies):
        legal = s.valid_actions()
        u = _oracle.lib().or_u01_f32(seed, pair, k)
        m = legal[opening_index(u, len(legal))]
        moves.append(m)
        s = s.next_state(m)
    return s, moves


def _finish(games, sims, evals):
    stats = dict(a_wins=[0.0, 0.0], draws=[0.0, 0.0], b_wins=[0.0, 0.0], sims=[float(x) for x in sims],
                 evals=[float(x) for x in evals], adjudicated=0.0, plies=0.0)
    for g in games:
        f = 0 if g["a_moves_first"] else 1
        stats["a_wins" if g["result_a"] > 0 else "b_wins" if g["result_a"] < 0 else "draws"][f] += 1
        stats["adjudicated"] += g["adjudicated"]
        stats["plies"] += g["n_moves"]
        g["moves"] = np.array(g["moves"], np.uint16)
    return games, stats


def oracle_match(a, b, n_games, game_id_base=0, opening_plies=2, max_plies=512, seed=0, start=None, c=2.0,
                 trace=None):
    """a, b: (eval_kind, None, num_searches) with eval_kind HASH or UNIFORM; start: STATE_DTYPE
    records, one per pair.  trace (a list) receives one dict per followed move: game, ply,
    replaced, child_visits_before, root_visits_after."""
    L = _lib()
    if start is not None and opening_plies:
        raise ValueError("start positions take no opening")
    players = (a, b)
    games, sims, evals = [], [0, 0], [0, 0]
    for g in range(n_games):
        gid = game_id_base + g
        pair = gid // 2
        s0 = chessref.ChessState() if start is None else state_from_abi(start[pair - game_id_base // 2])
        if s0.status != ONGOING:
            raise ValueError("start position is not Ongoing")
        cur, moves = opening_state(s0, seed, pair, opening_plies)
        trees = [L.orc_tree_with_root(C.byref(cur.st)) for _ in range(2)]
        G = dict(game=gid, a_moves_first=gid % 2 == 0, result_a=0, status=ONGOING, adjudicated=False)
        searched = 0
        while True:
            if max_plies and len(moves) >= max_plies:
                G["adjudicated"] = True
                break
            p = (gid + searched) & 1
            kind, _, n_s = players[p]
            ne, ids, vis, mv = _search(L, trees[p], n_s, kind, c)
            sims[p] += n_s
            evals[p] += ne
            k = pick_last_max(vis)
            if k is None:
                raise MatchNaN("no visited root child")
            move = int(mv[k])
            nxt = cur.next_state(move)
            L.orc_tree_use_subtree(trees[p], int(ids[k]))
            moves.append(move)
            searched += 1
            cur = nxt
            G["status"] = nxt.status
            if nxt.status != ONGOING:
                if nxt.status == WON:
                    G["result_a"] = 1 if p == 0 else -1
                break
            # the opponent's tree follows (main.rs:92): the first arena node whose state is the next state
            o = trees[p ^ 1]
            size = L.orc_tree_size(o)
            if size == 1:
                L.orc_tree_destroy(o)
                trees[p ^ 1] = L.orc_tree_with_root(C.byref(nxt.st))
                if trace is not None:
                    trace.append(dict(game=gid, ply=len(moves), replaced=True))
            else:
                root_made = L.orc_tree_node_state(o, 0).contents.made
                found = None
                for i in range(1, size):
                    st = L.orc_tree_node_state(o, i).contents
                    if st.made == root_made + 1 and _same_board(st.b, nxt.st.b):
                        found = i
                        break
                assert found is not None, "the opponent's tree does not hold the move"
                oids, ovis, omv = _root_stats(L, o)
                kk = list(oids).index(found)
                assert int(omv[kk]) == move and kk == k   # the same child index: both roots are the same position
                before = int(ovis[kk])
                L.orc_tree_use_subtree(o, found)
                _, avis, _ = _root_stats(L, o)
                after = 1 + int(avis.sum()) if len(avis) else 0
                if trace is not None:
                    trace.append(dict(game=gid, ply=len(moves), replaced=False, child_visits_before=before,
                                      root_visits_after=after))
        for t in trees:
            L.orc_tree_destroy(t)
        G["n_moves"] = len(moves)
        G["moves"] = moves
        games.append(G)
    return _finish(games, sims, evals)


def device_match(sc, a, b, n_games, game_id_base=0, opening_plies=2, max_plies=512, seed=0, start=None, blocks=1,
                 max_moves=2048):
    """a, b: (eval_kind, params or None, num_searches); a net player's engine gets a
    ChessNet of `blocks` blocks from params.  Game g is tree g and slot g of both engines."""
    _lib()
    players = (a, b)
    engs = []
    for kind, params, n_s in players:
        e = sc.ChessEngine(num_searches=n_s, max_trees=n_games, eval_kind=kind, max_moves=max_moves)
        if kind == EVAL_NET:
            e.set_net(sc.ChessNet(e, blocks, params))
        e.games_resize(n_games)
        e.trees_create(n_games)
        engs.append(e)
    pairs = [(game_id_base + g) // 2 for g in range(n_games)]
    if start is not None:
        assert opening_plies == 0
        st = np.array([start[pr - game_id_base // 2] for pr in pairs], sc.STATE_DTYPE)
        for e in engs:
            e.games_write(st)
    opening = [[] for _ in range(n_games)]
    for k in range(opening_plies):
        mv, cnt = engs[0].legal_moves(n_games)
        pick = np.array([mv[g, opening_index(_oracle.lib().or_u01_f32(seed, pairs[g], k), int(cnt[g]))]
                         for g in range(n_games)], np.uint16)
        for e in engs:
            e.apply(pick)
        for g in range(n_games):
            opening[g].append(int(pick[g]))
    for e in engs:
        for g in range(n_games):
            e.tree_reset(g, g)
    games, sims, evals = [], [0, 0], [0, 0]
    for g in range(n_games):
        gid = game_id_base + g
        moves = list(opening[g])
        G = dict(game=gid, a_moves_first=gid % 2 == 0, result_a=0, status=ONGOING, adjudicated=False)
        searched = 0
        while True:
            if max_plies and len(moves) >= max_plies:
                G["adjudicated"] = True
                break
            p = (gid + searched) & 1
            E, O = engs[p], engs[p ^ 1]
            n_s = players[p][2]
            _, _, vis, mv, nc = E.search([g], n_s)
            sims[p] += n_s
            k = pick_last_max(vis[0, :nc[0]])
            if k is None:
                raise MatchNaN("no visited root child")
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
            ra, rb = E.tree_root(g)[0], O.tree_root(g)[0]
            assert ra.tobytes() == rb.tobytes(), "the two trees disagree on the position after the move"
        G["n_moves"] = len(moves)
        G["moves"] = moves
        games.append(G)
    for e in engs:
        e.close()
    return _finish(games, sims, evals)
