"""The CPU yardstick of the chess search's root noise: Mcts::search over the oracle's
trees (orc_search) with the hash evaluator given as a callback, which mixes a given
noise vector into the priors of the root states.  It runs none of the device code.

The callback per leaf: orc_hash_eval_raw -> orc_mask_invalid (what orc_search's
built-in hash evaluator does), then, if the leaf is the root of tree t and eta[t] is
given, at the legal moves' policy indices in move-generation order
    P_j <- mix(P_j, eta[t][j], eps)
mix() is spai.h's float32 definition: a = (1 - eps) * P, b = eps * eta, a + b, the
factor 1 - eps rounded once and every operation rounded on its own.

A root is evaluated only while it has no children, so this covers fresh roots; a
root that kept its subtree is checked on the device side against get_ucb() below,
mcts.rs:94-99 restated in numpy float32.
"""
import ctypes as C

import numpy as np

import chessref as ch

POLICY = ch.POLICY

# positions with 218 legal moves (the most of any position) and with one
FEN_218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
FEN_ONE = "k7/8/8/8/8/7q/8/7K w - - 0 1"


def mix(prior, eta, eps):
    p, e = np.asarray(prior, np.float32), np.asarray(eta, np.float32)
    eps = np.float32(eps)
    om = np.float32(1.0) - eps
    a = om * p
    b = eps * e
    return (a + b).astype(np.float32)


def get_ucb(parent_n, n, w, prior, c=2.0):
    """get_ucb of every child (mcts.rs:91-100) in the reference's operation order, float32"""
    n32 = np.asarray(n).astype(np.float32)
    w32, p32 = np.asarray(w, np.float32), np.asarray(prior, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(np.asarray(n) == 0, np.float32(0.0), ((-w32 / n32) + np.float32(1.0)) / np.float32(2.0))
    u = np.float32(c) * p32
    u = u * np.sqrt(np.float32(parent_n))
    u = u / (np.float32(1.0) + n32)
    return (q.astype(np.float32) + u).astype(np.float32)


def last_argmax(x):
    """the last of equal maxima (Iterator::max_by, mcts.rs:110-113)"""
    x = np.asarray(x)
    return int(len(x) - 1 - np.argmax(x[::-1]))


class NoisedHashSearch:
    """oracle trees rooted at `states` (chessref.ChessState), searched with the hash
    evaluator as a callback; eta: per tree a float32 vector over the root's legal moves
    (or None), mixed in with weight eps when the tree's root is evaluated"""

    def __init__(self, states, eta=None, eps=0.0, c=2.0):
        self.L = ch.lib()
        self.states, self.c, self.eps = states, c, eps
        self.n = len(states)
        self.eta = list(eta) if eta is not None else [None] * self.n
        self.trees = [self.L.orc_tree_with_root(C.byref(s.st)) for s in states]
        self.arr = (C.c_void_p * self.n)(*self.trees)
        self.mixed = []          # trees whose root the callback mixed, in order
        self.error = None
        self._cb = ch.EVAL_FN(self._evaluate)

    def close(self):
        for t in self.trees:
            self.L.orc_tree_destroy(t)
        self.trees = []

    def _evaluate(self, user, n, states, priors, values):
        try:
            self._evaluate_checked(n, states, priors, values)
        except Exception as ex:   # an exception cannot cross the C frame: keep it for search()
            self.error = ex
            np.ctypeslib.as_array(priors, (n * POLICY,))[:] = 1.0 / POLICY
            np.ctypeslib.as_array(values, (n,))[:] = 0.0

    def _evaluate_checked(self, n, states, priors, values):
        L = self.L
        fp = C.POINTER(C.c_float)
        roots = {C.addressof(L.orc_tree_node_state(t, 0).contents): i for i, t in enumerate(self.trees)}
        pri = np.ctypeslib.as_array(priors, (n * POLICY,)).reshape(n, POLICY)
        val = np.ctypeslib.as_array(values, (n,))
        raw = np.zeros(POLICY, np.float32)
        out = np.zeros(POLICY, np.float32)
        for i in range(n):
            st = states[i]
            v = C.c_float()
            L.orc_hash_eval_raw(st, raw.ctypes.data_as(fp), C.byref(v))
            if L.orc_mask_invalid(st, raw.ctypes.data_as(fp), POLICY, out.ctypes.data_as(fp)) != 0:
                raise ValueError("orc_mask_invalid")
            t = roots.get(C.addressof(st.contents))
            if t is not None and self.eta[t] is not None:
                b = st.contents.b
                idx = [ch.policy_index(int(b.side), m) for m in ch.legal_moves(b)]
                eta = np.asarray(self.eta[t], np.float32)
                assert len(eta) == len(idx), (t, len(eta), len(idx))
                out[idx] = mix(out[idx], eta, self.eps)
                self.mixed.append(t)
            pri[i] = out
            val[i] = v.value

    def search(self, sims):
        """-> dict(nc [n], moves [n][256], visits [n][256], ids [n][256], policy [n][4672], evals)"""
        n = self.n
        pol = np.zeros((n, POLICY), np.float32)
        ids = np.zeros((n, ch.MAX_MOVES), np.int32)
        vis = np.zeros((n, ch.MAX_MOVES), np.float32)
        mv = np.zeros((n, ch.MAX_MOVES), np.int32)
        nc = np.zeros(n, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        rc = self.L.orc_search(self.arr, n, sims, self.c, self._cb, None, fp(pol), ip(ids), fp(vis), ip(mv), ip(nc))
        if self.error is not None:
            raise self.error
        if rc < 0:
            raise FloatingPointError("orc_search: NaN UCB")
        return dict(nc=nc, moves=mv, visits=vis, ids=ids, policy=pol, evals=rc)


def noised_hash_search(states, sims, eta=None, eps=0.0, c=2.0):
    rs = NoisedHashSearch(states, eta, eps, c)
    try:
        res = rs.search(sims)
        res["mixed"] = sorted(rs.mixed)
        return res
    finally:
        rs.close()


def extra_states():
    """the 218-move and the one-move position as ChessStates (empty history)"""
    return [ch.ChessState(fen=FEN_218, made=0, fifty=0), ch.ChessState(fen=FEN_ONE, made=0, fifty=0)]
