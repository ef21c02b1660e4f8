"""Mcts::search, self-play and matches over the CPU Connect4 oracle with the net
given as a callback, the yardstick of tests/test_c4_search_net_gpu.py (and, with
the oracle's own fp32 net behind it, the subject of
tests/test_c4_search_ref_cpu.py).  It runs none of the device search's code:
or_search / or_self_play walk the oracle's trees and ask `predict` for every leaf.

Evaluator    the callback.  From the n or_c4_state the oracle hands over it takes
             the bitboards (bit col * 7 + row, the product's layout) and the move
             count, calls predict(states [(x, o, n, 0)]) -> (priors [m][7] float32,
             values [m] float32) once per callback over the positions not seen
             before, keeps the answers by (x, o, n) and writes their bytes back
             unchanged.  An Evaluator is itself the eval_fn of oracle.search_c4,
             oracle.self_play and a player of match_ref.
RefSearch    oracle trees rooted at given positions: search, use_subtree, and the
             root's N, W and its children's N, W, P through or_tree_node_info.
Fault        a wrapper around any predict: the errors of a search's net path that
             the yardstick must react to, and the ulp noise that only the node
             records show.
positions    the roots both tests search from.
"""
import ctypes as C
import zlib

import numpy as np

import oracle as orc

STATE_BYTES = C.sizeof(orc.C4State)
# bit of board[row][col] in the product's bitboards
_BITS = np.array([[1 << (col * 7 + row) for col in range(7)] for row in range(6)], np.uint64)


def state_keys(states, n):
    """the n or_c4_state behind the callback's pointers -> [(x, o, moves played)]"""
    raw = np.frombuffer(b"".join(C.string_at(states[i], STATE_BYTES) for i in range(n)), np.uint8)
    raw = raw.reshape(n, STATE_BYTES)
    board = raw[:, :42].reshape(n, 6, 7)
    x = np.where(board == orc.X, _BITS, np.uint64(0)).sum((1, 2), dtype=np.uint64)
    o = np.where(board == orc.O, _BITS, np.uint64(0)).sum((1, 2), dtype=np.uint64)
    return list(zip(x.tolist(), o.tolist(), raw[:, 43].tolist()))


def state_from_key(x, o, n):
    """oracle.C4 of the ongoing position (x, o, n)"""
    st = orc.C4State()
    orc.lib().or_c4_init(C.byref(st))
    for col in range(7):
        for row in range(6):
            b = 1 << (col * 7 + row)
            if x & b:
                st.board[row][col] = orc.X
            elif o & b:
                st.board[row][col] = orc.O
    st.num_actions_played = n
    st.current_player = orc.X if n % 2 == 0 else orc.O
    st.status = orc.ONGOING
    return orc.C4(st)


def key_of(s):
    """(x, o, n) of an oracle.C4"""
    x, o = s.bitboards()
    return x, o, s.n


def legal_columns(x, o):
    """the columns that are not full, ascending (the order of a node's children)"""
    occ = x | o
    return [c for c in range(7) if not (occ >> (c * 7 + 5)) & 1]


def oracle_predict(net):
    """predict(states) on an oracle.Net: or_predict, the fp32 Model::predict"""
    def predict(states):
        sts = [state_from_key(x, o, n) for x, o, n, _ in states]
        m = len(sts)
        arr = (C.c_void_p * m)(*[C.addressof(s.st) for s in sts])
        p, v = np.zeros((m, 7), np.float32), np.zeros(m, np.float32)
        orc.lib().or_predict(net.h, m, arr, orc._f(p), orc._f(v))
        return p, v
    return predict


class Evaluator:
    """the callback's state: predict, what it answered (shared between searches, so
    that a rerun costs no forward) and what it saw"""

    def __init__(self, predict):
        self.predict = predict
        self.index = {}                               # (x, o, n) -> row of P, V
        self.P = np.zeros((1024, 7), np.float32)
        self.V = np.zeros(1024, np.float32)
        self.calls = 0        # callbacks
        self.leaves = 0       # leaves handed over
        self.forwards = 0     # predict calls
        self.error = None

    def rows(self, keys):
        new = [k for k in dict.fromkeys(keys) if k not in self.index]
        if new:
            p, v = self.predict([(x, o, n, 0) for x, o, n in new])
            p, v = np.asarray(p), np.asarray(v)
            assert p.dtype == np.float32 and v.dtype == np.float32 and p.shape == (len(new), 7), (p.dtype, p.shape)
            self.forwards += 1
            base = len(self.index)
            while base + len(new) > len(self.V):
                self.P = np.concatenate([self.P, np.zeros_like(self.P)])
                self.V = np.concatenate([self.V, np.zeros_like(self.V)])
            self.P[base:base + len(new)] = p
            self.V[base:base + len(new)] = v
            for i, k in enumerate(new):
                self.index[k] = base + i
        return np.fromiter((self.index[k] for k in keys), np.int64, len(keys))

    def entry(self, key):
        """(priors [7], value) as predict answered for (x, o, n), evaluated now if new"""
        r = self.rows([tuple(key)])[0]
        return self.P[r].copy(), self.V[r].copy()

    def __call__(self, user, n, states, priors, values):
        try:
            r = self.rows(state_keys(states, n))
            np.ctypeslib.as_array(priors, (n, 7))[:] = self.P[r]
            np.ctypeslib.as_array(values, (n,))[:] = self.V[r]
            self.calls += 1
            self.leaves += n
        except Exception as ex:   # an exception cannot cross the C frame: keep it for check()
            self.error = self.error or ex
            np.ctypeslib.as_array(priors, (n, 7))[:] = 1.0 / 7
            np.ctypeslib.as_array(values, (n,))[:] = 0.0

    def check(self):
        if self.error is not None:
            raise self.error


class Fault:
    """predict with one injected error of the search's net path.  Slots are those of
    the wrapped predict's own call (the positions a callback had not seen before)."""
    NEG_VALUE = "value negated"
    NEXT_PRIORS = "priors of batch slot k+1 given to slot k"
    NEXT_VALUE = "value of batch slot k+1 given to slot k"
    SWAP_SIDES = "entry of the position with mine and theirs swapped"
    NO_RENORM = "priors not renormalised after masking"
    ULP_NOISE = "priors times 1 + k * 2^-23"
    GROSS = (NEG_VALUE, NEXT_PRIORS, NEXT_VALUE, SWAP_SIDES, NO_RENORM)

    def __init__(self, predict, kind, seed=0, amp=1):
        """ULP_NOISE: k an integer drawn uniformly from [-amp, amp] per (seed, position, column).
        NO_RENORM: predict's priors are renormalised and do not tell the mass the mask
        removed; the fault is modelled with the mass a flat softmax keeps, legal / 7, so it
        acts at the positions with a full column, as the real one does."""
        self.predict, self.kind, self.seed, self.amp = predict, kind, seed, amp
        self.changed = set()   # positions (x, o, n) whose legal priors or value got other bits

    def __call__(self, states):
        states = [tuple(int(v) for v in s) for s in states]
        if self.kind == self.SWAP_SIDES:
            p, v = self.predict([(o, x, n, st) for x, o, n, st in states])
            p, v = np.array(p), np.array(v)
            self.changed.update(s[:3] for s in states)
            return p, v
        p0, v0 = self.predict(states)
        p, v = np.array(p0), np.array(v0)
        if self.kind == self.NEG_VALUE:
            v = -v
        elif self.kind == self.NEXT_PRIORS:
            p = np.roll(p, -1, axis=0)
        elif self.kind == self.NEXT_VALUE:
            v = np.roll(v, -1)
        elif self.kind == self.NO_RENORM:
            legal = np.array([len(legal_columns(x, o)) for x, o, _, _ in states], np.float32)
            p = p * (legal / np.float32(7))[:, None]
        elif self.kind == self.ULP_NOISE:
            for i, (x, o, n, _) in enumerate(states):
                rng = np.random.default_rng([self.seed, zlib.crc32(np.array([x, o, n], np.uint64).tobytes())])
                k = rng.integers(-self.amp, self.amp + 1, 7)
                p[i] = (p[i].astype(np.float64) * (1.0 + k * 2.0 ** -23)).astype(np.float32)
        else:
            raise ValueError(self.kind)
        for i, s in enumerate(states):
            cols = legal_columns(s[0], s[1])
            if p[i, cols].tobytes() != np.asarray(p0)[i, cols].tobytes() or v[i].tobytes() != np.asarray(v0)[i].tobytes():
                self.changed.add(s[:3])
        return p.astype(np.float32), v.astype(np.float32)


class RefSearch:
    """oracle trees rooted at `roots` (oracle.C4), searched with `ev` (Evaluator).  The
    trees live until close(), so advance() + search() is use_subtree + a further search."""

    def __init__(self, roots, ev, c=2.0):
        self.L = orc.lib()
        self.ev, self.c = ev, c
        self.n = len(roots)
        self.trees = [self.L.or_tree_with_root(orc.GAME_CONNECT4, C.byref(s.st)) for s in roots]
        self.last = None

    def close(self):
        for t in self.trees:
            self.L.or_tree_destroy(t)
        self.trees = []

    def search(self, sims):
        """-> dict(policy [n][7], ids [n][7], visits [n][7], nc [n], evals)"""
        rc, pol, ids, vis, nc = orc.search_c4(None, sims, eval_kind=orc.EVAL_NET, c=self.c, trees=self.trees,
                                              eval_fn=self.ev)
        self.ev.check()
        if rc < 0:
            raise FloatingPointError("or_search: NaN UCB")
        self.last = dict(policy=pol, ids=ids, visits=vis, nc=nc, evals=rc)
        return self.last

    def advance(self, t, k):
        """Tree::use_subtree(root child k) of tree t, after a search()"""
        assert 0 <= k < self.last["nc"][t]
        self.L.or_tree_use_subtree(self.trees[t], int(self.last["ids"][t, k]))

    def _info(self, t, node):
        act, nch = C.c_int(), C.c_int()
        pri, w = C.c_float(), C.c_float()
        vis = C.c_uint32()
        ch = (C.c_int * 9)()
        rc = self.L.or_tree_node_info(self.trees[t], node, None, C.byref(act), C.byref(pri), C.byref(vis), C.byref(w),
                                      C.byref(nch), ch)
        assert rc == 0, (t, node)
        return act.value, pri.value, vis.value, w.value, [int(ch[i]) for i in range(nch.value)]

    def root(self, t):
        """(N, W) of tree t's root, W a float32"""
        _, _, vis, w, _ = self._info(t, 0)
        return vis, np.float32(w)

    def root_state(self, t):
        return orc.C4(orc.C4State.from_buffer_copy(C.string_at(self.L.or_tree_node_state(self.trees[t], 0), STATE_BYTES)))

    def children(self, t):
        """tree t's root children in action order -> (actions [k], N uint32 [k], W float32 [k], P float32 [k])"""
        kids = self._info(t, 0)[4]
        rec = [self._info(t, k)[:4] for k in kids]
        return (np.array([r[0] for r in rec], np.int64), np.array([r[2] for r in rec], np.uint32),
                np.array([r[3] for r in rec], np.float32), np.array([r[1] for r in rec], np.float32))

    def records(self):
        return [self.children(t) for t in range(self.n)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def most_visited_last(visits, n):
    """index of the most visited of the first n children, the last one on ties"""
    v = np.asarray(visits[:n])
    return int(n - 1 - np.argmax(v[::-1]))


def wins_in_one(s):
    return any(s.next_state(a).status == orc.WON for a in s.valid_actions())


def has_full_column(s):
    return len(s.valid_actions()) < 7


def positions(n, seed, duplicates=0):
    """n ongoing roots (oracle.C4) after 0..20 random legal plies each, the empty board
    among them; every third playout prefers a few columns, so that columns fill up.
    n - duplicates of them are distinct, and of those at least an eighth (one at least)
    have a full column and as many stand one move before a win of the side to move, so
    that terminal children and terminal leaves occur in their searches; `duplicates`
    further roots repeat earlier ones, so that trees share leaves.  The order is
    shuffled: kinds and copies spread over the batch."""
    rng = np.random.default_rng(seed)
    distinct = n - duplicates
    assert distinct >= 3 and duplicates >= 0
    q = max(1, distinct // 8)
    need = {"full": q, "win": q}
    out, seen, tries = [], set(), 0
    while len(out) < distinct:
        plies = 0 if tries == 0 else int(rng.integers(0, 21))
        w = rng.dirichlet([0.3] * 7) + 1e-3 if tries % 3 == 2 else np.ones(7)
        tries += 1
        s = orc.C4()
        for _ in range(plies):
            va = s.valid_actions()
            pw = w[va] / w[va].sum()
            nx = s.next_state(int(rng.choice(va, p=pw)))
            if nx.status != orc.ONGOING:
                break
            s = nx
        k = key_of(s)
        if k in seen:
            continue
        kinds = [kind for kind, f in (("full", has_full_column), ("win", wins_in_one)) if need[kind] > 0 and f(s)]
        if not kinds and len(out) >= distinct - sum(need.values()):
            continue   # the places left are kept for the kinds still missing
        for kind in kinds:
            need[kind] -= 1
        seen.add(k)
        out.append(s)
    out = [out[i] for i in rng.permutation(distinct)]
    out += [out[int(i)] for i in rng.integers(0, distinct, duplicates)]
    return [out[i] for i in rng.permutation(n)]
