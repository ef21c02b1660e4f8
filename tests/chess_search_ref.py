"""Mcts::search over the CPU chess oracle with a net evaluator given as a
callback, the yardstick of tests/test_chess_search_net_gpu.py (and, with a
float64 net, the subject of tests/test_chess_search_ref_cpu.py).  It runs none of
the device search's code: orc_search walks the oracle's trees and asks
`forward` for every leaf.

Model::predict (model/mod.rs:36-98) per leaf, restated here:
  encoding   orc_encoding of the leaf's State (19 planes from the side to move)
  forward    forward(x [n][19][8][8] float32) -> logits [n][4672], value [n]; one
             call per callback over the encodings not seen before, cached by the
             encoding's bytes
  priors     softmax in float64, cast to float32, orc_mask_invalid
  value      float32

positions()  the 24 root positions both tests use.
Fault        the errors of a search's net path that the reference must react to.
ulp noise    every softmax entry times 1 + k * 2^-23, k an integer drawn
             uniformly from [-amp, amp] per (seed, encoding, entry): what a
             last-bits difference between two evaluators' priors can do.
"""
import ctypes as C
import random
import zlib

import numpy as np

import chessref as ch

POLICY = ch.POLICY
N_POSITIONS = 24

# the FENS of tests/test_chess_gpu.py (promotions, an en-passant capture on offer, both sides with rights)
FENS = [
    "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1",
    "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1",
    "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8",
    "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1",
    "4k3/8/8/3pP3/8/8/P7/4K3 w - d6 0 1",
]

LINES = [
    "",                               # the start position
    "e2e4",                           # black to move, en-passant square set
    "g1f3 g8f6 f3g1 f6g8",            # the root has occurred before: repetitions 2, fifty 4
    "e2e4 e7e5 e1e2",                 # white has lost both rights, black to move
    "h2h4 a7a5 h1h3",                 # white's king-side rook has moved: one right lost on one side
    # further roots that stand a second time (the repetition plane is 2 only at such positions,
    # so a search reacts to an error in it only from them), of both colours
    "e2e4 e7e5 g1f3 b8c6 f3g1 c6b8",
    "d2d4 g8f6 b1c3 f6g8 c3b1",
    "d2d4 d7d5 b1a3 b8a6 a3b1 a6b8",
    "c2c4 c7c5 g1f3 g8f6 f3g1 f6g8",
    "g2g3 e7e6 f1g2 f8e7 g2f1 e7f8",
    "b2b3 b7b6 c1b2 c8b7 b2c1 b7c8",
]


def _mv(s):
    return ch.move(ch.sq(s[:2]), ch.sq(s[2:4]))


def positions():
    """[(moves or None, fen or None, ChessState)] x 24: LINES played from the start
    position (the state carries the history), FENS with an empty history, then
    random playouts of 1 to 59 plies (random.Random(17)) that are still ongoing"""
    out = []
    for line in LINES:
        s, seq = ch.ChessState(), [_mv(m) for m in line.split()]
        for m in seq:
            s = s.next_state(m)
        out.append((seq, None, s))
    for f in FENS:
        out.append((None, f, ch.ChessState(fen=f, made=0, fifty=0)))
    rng = random.Random(17)
    while len(out) < N_POSITIONS:
        s, seq = ch.ChessState(), []
        for _ in range(rng.randrange(1, 60)):
            mv = s.valid_actions()
            if not mv or s.status:
                break
            m = rng.choice(mv)
            seq.append(m)
            s = s.next_state(m)
        if not s.status and s.valid_actions():
            out.append((seq, None, s))
    return out


def softmax64(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max())
    return e / e.sum()


def ulps(a, b):
    """|a - b| in units of float32 ulp(b), elementwise, for positive normal b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float32)
    return np.abs(a - b.astype(np.float64)) / np.spacing(b).astype(np.float64)


class Fault:
    """one injected error of the search's net path (None: no fault)"""
    SWAP_CASTLING = "castling planes: mine <-> theirs"
    REPS_ONE = "repetition plane forced to 1"
    MADE_ZERO = "made plane zeroed"
    WHITE_INDEX = "priors gathered with policy_index(0, move) for black"
    NEG_VALUE = "value negated"
    ALL = (SWAP_CASTLING, REPS_ONE, MADE_ZERO, WHITE_INDEX, NEG_VALUE)


class Evaluator:
    """the callback's state: forward, its cache and what it saw (shared between
    searches so that a rerun costs no forward)"""

    def __init__(self, forward):
        self.forward = forward
        self.cache = {}       # (fault-transformed) encoding bytes -> (softmax float64 [4672], value float32)
        self.forwards = 0     # forward calls
        self.misses = 0       # encodings evaluated

    def lookup(self, encs):
        keys = [e.tobytes() for e in encs]
        new = {}
        for k, e in zip(keys, encs):
            if k not in self.cache and k not in new:
                new[k] = e
        if new:
            lg, v = self.forward(np.stack(list(new.values())).astype(np.float32))
            self.forwards += 1
            self.misses += len(new)
            for i, k in enumerate(new):
                self.cache[k] = (softmax64(lg[i]), np.float32(v[i]))
        return keys, [self.cache[k] for k in keys]


class RefSearch:
    """n oracle trees rooted at `states` (ChessState), searched with `ev`
    (Evaluator).  The trees live until close(), so advance() + search() is
    use_subtree + a further search, as self-play does it."""

    def __init__(self, states, ev, c=2.0, fault=None, noise=None):
        """noise = (seed, amp): the ulp noise of the module docstring"""
        self.L = ch.lib()
        self.ev, self.c, self.fault, self.noise = ev, c, fault, noise
        self.n = len(states)
        self.states = states                      # keeps the roots' tables referenced
        self.trees = [self.L.orc_tree_with_root(C.byref(s.st)) for s in states]
        self.arr = (C.c_void_p * self.n)(*self.trees)
        self.sides = set()
        self.path_rep2 = 0                        # non-root leaves with orc_num_repetitions == 2
        self.seen = set()                         # distinct (true) encodings
        self.evals = 0
        self.batches = []                         # leaves per callback (one per search iteration with a leaf)
        self._cb = ch.EVAL_FN(self._evaluate)
        self.error = None

    def close(self):
        for t in self.trees:
            self.L.orc_tree_destroy(t)
        self.trees = []

    # ---- the callback
    def _encode(self, st):
        e = np.zeros((19, 8, 8), np.float32)
        self.L.orc_encoding(st, e.ctypes.data_as(C.POINTER(C.c_float)))
        return e

    def _evaluate(self, user, n, states, priors, values):
        try:
            self._evaluate_checked(n, states, priors, values)
        except Exception as ex:   # an exception cannot cross the C frame: keep it for search()
            self.error = ex
            np.ctypeslib.as_array(priors, (n * POLICY,))[:] = 1.0 / POLICY
            np.ctypeslib.as_array(values, (n,))[:] = 0.0

    def _evaluate_checked(self, n, states, priors, values):
        L = self.L
        roots = {C.addressof(L.orc_tree_node_state(t, 0).contents) for t in self.trees}
        encs = []
        for i in range(n):
            st = states[i]
            e = self._encode(st)
            self.seen.add(e.tobytes())
            self.sides.add(int(st.contents.b.side))
            if C.addressof(st.contents) not in roots and L.orc_num_repetitions(st) == 2:
                self.path_rep2 += 1
            if self.fault == Fault.SWAP_CASTLING:
                e[[12, 13, 14, 15]] = e[[14, 15, 12, 13]]
            elif self.fault == Fault.REPS_ONE:
                e[16] = 1.0
            elif self.fault == Fault.MADE_ZERO:
                e[18] = 0.0
            encs.append(e)
        keys, res = self.ev.lookup(encs)
        self.evals += n
        self.batches.append(n)
        pri = np.ctypeslib.as_array(priors, (n * POLICY,)).reshape(n, POLICY)
        val = np.ctypeslib.as_array(values, (n,))
        for i in range(n):
            sm, v = res[i]
            if self.noise is not None:
                seed, amp = self.noise
                k = np.random.default_rng([seed, zlib.crc32(keys[i])]).integers(-amp, amp + 1, POLICY)
                sm = sm * (1.0 + k * 2.0 ** -23)
            sm32 = np.ascontiguousarray(sm, np.float32)
            if self.fault == Fault.WHITE_INDEX and states[i].contents.b.side == ch.BLACK:
                mv = ch.legal_moves(states[i].contents.b)
                m = np.zeros(POLICY, np.float32)
                for a in mv:
                    m[ch.policy_index(ch.BLACK, a)] = sm32[ch.policy_index(ch.WHITE, a)]
                pri[i] = m / m.sum(dtype=np.float32)
            else:
                out = np.zeros(POLICY, np.float32)
                if L.orc_mask_invalid(states[i], sm32.ctypes.data_as(C.POINTER(C.c_float)), POLICY,
                                      out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
                    raise ValueError("orc_mask_invalid")
                pri[i] = out
            val[i] = -v if self.fault == Fault.NEG_VALUE else v

    # ---- Mcts::search / use_subtree
    def search(self, sims):
        """-> dict(nc [n], moves [n][256], visits [n][256], ids [n][256], policy [n][4672], evals,
        batches: the leaves evaluated in each iteration that had any)"""
        n = self.n
        pol = np.zeros((n, POLICY), np.float32)
        ids = np.zeros((n, ch.MAX_MOVES), np.int32)
        vis = np.zeros((n, ch.MAX_MOVES), np.float32)
        mv = np.zeros((n, ch.MAX_MOVES), np.int32)
        nc = np.zeros(n, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        before, calls = self.evals, len(self.batches)
        rc = self.L.orc_search(self.arr, n, sims, self.c, self._cb, None, fp(pol), ip(ids), fp(vis), ip(mv), ip(nc))
        if self.error is not None:
            raise self.error
        if rc < 0:
            raise FloatingPointError("orc_search: NaN UCB")
        assert rc == self.evals - before, (rc, self.evals - before)
        self.last = dict(nc=nc, moves=mv, visits=vis, ids=ids, policy=pol, evals=rc,
                         batches=self.batches[calls:])
        return self.last

    def advance(self, picks):
        """Tree::use_subtree(child picks[t]) of every tree, after a search()"""
        for t, k in enumerate(picks):
            assert 0 <= k < self.last["nc"][t]
            self.L.orc_tree_use_subtree(self.trees[t], int(self.last["ids"][t, k]))

    def root(self, t):
        return self.L.orc_tree_node_state(self.trees[t], 0)


def most_visited_last(visits, n):
    """index of the most visited of the first n children, the last one on ties"""
    v = np.asarray(visits[:n])
    return int(n - 1 - np.argmax(v[::-1]))


def visit_table(res):
    """the visit counts of a search() result as one comparable tuple per tree"""
    return [tuple(res["visits"][t, :res["nc"][t]].astype(np.int64)) for t in range(len(res["nc"]))]
