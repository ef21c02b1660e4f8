"""The CPU yardsticks of the Connect4 search's root noise.  Neither runs any of the
device code.

(a) NoisedSearch: the oracle's Mcts::search (or_search) over its own trees with the
    hash evaluator given as a callback -- or_hash_eval_raw, then or_c4_mask_invalid,
    what the oracle's built-in hash evaluator does -- which, when the leaf it is asked
    about is the root of tree t (the address of or_tree_node_state(t, 0)) and eta[t] is
    given, mixes eta[t] into the priors of the root's legal columns, ascending:
        P_j <- mix(P_j, eta[t][j], eps)
    A root is evaluated only while it has no children, so (a) covers fresh roots.

(b) PyTree / py_search / py_self_play: mcts.rs:196-332 restated in Python on float32
    numpy scalars: select by get_ucb with the last maximum, expand in ascending
    legal-column order, back up with the sign flip, use_subtree keeping the new root's
    N and W; and SelfPlayWorker::self_play on it (or_u01_f32, or_weighted_index, the
    values signed per mover).  It can mix an eta into a root that already has children,
    which (a) cannot, and it can mix late (after the first selection at the root), the
    error a misplaced launch would make.

mix, get_ucb and last_argmax are chess_noise_ref's: one definition serves both games.
"""
import ctypes as C

import numpy as np

import c4_search_ref as R
import oracle as orc
from chess_noise_ref import get_ucb, last_argmax, mix

F32 = np.float32


# ---------------------------------------------------------------- the hash evaluator
def hash_eval(state):
    """(priors [7] float32, value float32) of the hash evaluator for an oracle.C4"""
    x, o = state.bitboards()
    raw = np.zeros(7, F32)
    v = C.c_float()
    orc.lib().or_hash_eval_raw(x, o, int(state.n), 7, orc._f(raw), C.byref(v))
    return state.mask_invalid(raw), F32(v.value)


def hash_predict(states):
    """c4_search_ref's predict signature over the hash evaluator: [(x, o, n, _)] -> (P [m][7], V [m])"""
    out = [hash_eval(R.state_from_key(x, o, n)) for x, o, n, _ in states]
    return np.array([p for p, _ in out], F32).reshape(len(out), 7), np.array([v for _, v in out], F32)


# ---------------------------------------------------------------- (a)
class NoisedSearch:
    """oracle trees rooted at `roots` (oracle.C4); eta: per tree a float32 vector over the
    root's legal columns (or None), mixed in with weight eps when that root is evaluated"""

    def __init__(self, roots, eta=None, eps=0.0, c=2.0):
        self.L = orc.lib()
        self.c, self.eps = c, eps
        self.n = len(roots)
        self.eta = list(eta) if eta is not None else [None] * self.n
        self.trees = [self.L.or_tree_with_root(orc.GAME_CONNECT4, C.byref(s.st)) for s in roots]
        self.mixed = []      # trees whose root the callback mixed, in order
        self.error = None
        self.ref = R.RefSearch.__new__(R.RefSearch)   # its record readers, over these trees
        self.ref.L, self.ref.trees, self.ref.n = self.L, self.trees, self.n

    def close(self):
        for t in self.trees:
            self.L.or_tree_destroy(t)
        self.trees = []
        self.ref.trees = []

    def _evaluate(self, user, n, states, priors, values):
        try:
            roots = {int(self.L.or_tree_node_state(t, 0)): i for i, t in enumerate(self.trees)}
            pri = np.ctypeslib.as_array(priors, (n, 7))
            val = np.ctypeslib.as_array(values, (n,))
            for i, (x, o, m) in enumerate(R.state_keys(states, n)):
                s = R.state_from_key(x, o, m)
                p, v = hash_eval(s)
                t = roots.get(int(states[i]))
                if t is not None and self.eta[t] is not None:
                    cols = s.valid_actions()
                    eta = np.asarray(self.eta[t], F32)
                    assert len(eta) == len(cols), (t, len(eta), len(cols))
                    p[cols] = mix(p[cols], eta, self.eps)
                    self.mixed.append(t)
                pri[i] = p
                val[i] = v
        except Exception as ex:   # an exception cannot cross the C frame: keep it for search()
            self.error = self.error or ex
            np.ctypeslib.as_array(priors, (n, 7))[:] = 1.0 / 7
            np.ctypeslib.as_array(values, (n,))[:] = 0.0

    def search(self, sims):
        """-> dict(policy [n][7], ids [n][7], visits [n][7], nc [n], evals)"""
        rc, pol, ids, vis, nc = orc.search_c4(None, sims, eval_kind=orc.EVAL_NET, c=self.c, trees=self.trees,
                                              eval_fn=self._evaluate)
        if self.error is not None:
            raise self.error
        if rc < 0:
            raise FloatingPointError("or_search: NaN UCB")
        return dict(policy=pol, ids=ids, visits=vis, nc=nc, evals=rc)

    def root(self, t):
        return self.ref.root(t)

    def children(self, t):
        return self.ref.children(t)


def noised_search(roots, sims, eta=None, eps=0.0, c=2.0):
    """one search of fresh trees -> the search's dict plus mixed, roots [(N, W)] and records"""
    rs = NoisedSearch(roots, eta, eps, c)
    try:
        res = rs.search(sims)
        res["mixed"] = sorted(rs.mixed)
        res["roots"] = [rs.root(t) for t in range(rs.n)]
        res["records"] = [rs.children(t) for t in range(rs.n)]
        return res
    finally:
        rs.close()


# ---------------------------------------------------------------- (b)
class _Node:
    __slots__ = ("state", "action", "prior", "n", "w", "children", "parent")

    def __init__(self, state, action, prior, parent):
        self.state, self.action, self.prior, self.parent = state, action, F32(prior), parent
        self.n, self.w, self.children = 0, F32(0.0), []


class PyTree:
    """Tree (mcts.rs:20-60) with Mcts::search's per-tree steps; evaluate(state) -> (priors [7], value)"""

    def __init__(self, root=None, evaluate=hash_eval, c=2.0):
        self.root = _Node(root if root is not None else orc.C4(), -1, 0.0, None)
        self.evaluate, self.c = evaluate, c
        self.evals = 0

    # mcts.rs:102-114
    def _select(self, node):
        ch = node.children
        u = get_ucb(node.n, np.array([k.n for k in ch], np.uint32), np.array([k.w for k in ch], F32),
                    np.array([k.prior for k in ch], F32), self.c)
        if np.isnan(u).any():
            raise FloatingPointError("NaN UCB")
        return ch[last_argmax(u)]

    # mcts.rs:145-159
    @staticmethod
    def _backprop(node, value):
        sign = F32(1.0)
        while node is not None:
            node.n += 1
            node.w = F32(node.w + F32(sign * F32(value)))
            sign = F32(-sign)
            node = node.parent

    def mix_root(self, eta, eps):
        """P_j <- mix(P_j, eta_j, eps) over the root's children in stored order"""
        ch = self.root.children
        assert len(ch) == len(eta), (len(ch), len(eta))
        new = mix(np.array([k.prior for k in ch], F32), eta, eps)
        for k, p in zip(ch, new):
            k.prior = F32(p)

    def search(self, sims, eta=None, eps=0.0, late=False):
        """Mcts::search's iterations for this tree (mcts.rs:214-285).  eta: mixed into the root
        children's priors once -- on entry where the root has children, else right behind the
        root's expansion (before the first selection at it); late: after the first selection at
        the root instead (the error of a mix enqueued too late)."""
        pending = eta is not None
        if pending and self.root.children and not late:
            self.mix_root(eta, eps)
            pending = False
        for _ in range(sims):
            node = self.root
            selected_at_root = bool(node.children)
            while node.children:
                node = self._select(node)
            v, term = node.state.value_terminated()
            if term:
                self._backprop(node, F32(v))
            else:
                p, v = self.evaluate(node.state)
                self.evals += 1
                for a in node.state.valid_actions():            # ascending (mcts.rs:116-143)
                    node.children.append(_Node(node.state.next_state(a), a, p[a], node))
                self._backprop(node, v)
                if pending and node is self.root and not late:
                    self.mix_root(eta, eps)
                    pending = False
            if pending and late and selected_at_root:
                self.mix_root(eta, eps)
                pending = False

    def use_subtree(self, k):
        """Tree::use_subtree(root child k): the child keeps its N, W and subtree"""
        self.root = self.root.children[k]
        self.root.parent = None

    def root_record(self):
        return self.root.n, F32(self.root.w)

    def children(self):
        """-> (actions [k], N uint32 [k], W float32 [k], P float32 [k]), c4_search_ref.RefSearch.children's form"""
        ch = self.root.children
        return (np.array([k.action for k in ch], np.int64), np.array([k.n for k in ch], np.uint32),
                np.array([k.w for k in ch], F32), np.array([k.prior for k in ch], F32))

    def visits(self):
        return np.array([k.n for k in self.root.children], F32)

    def policy(self):
        """the root visit policy (mcts.rs:310-331): visits by action, over their sequential float32 sum"""
        pol = np.zeros(7, F32)
        for k in self.root.children:
            pol[k.action] = F32(k.n)
        s = F32(0.0)
        for a in range(7):
            s = F32(s + pol[a])
        with np.errstate(invalid="ignore"):     # one simulation: no child visited, 0 / 0 as in the reference
            return (pol / s).astype(F32)


def n_root_children(tree):
    """how many children the root has, or will have once expanded"""
    return len(tree.root.children) or len(tree.root.state.valid_actions())


def py_search(roots, sims, eta=None, eps=0.0, late=False, c=2.0):
    """fresh PyTrees over `roots`, searched once -> the trees"""
    trees = [PyTree(s, c=c) for s in roots]
    for t, tr in enumerate(trees):
        tr.search(sims, None if eta is None else eta[t], eps, late)
    return trees


def py_self_play(n_games, sims, seed, eta_fn=None, eps=0.0, temperature=1.25, game_id_base=0, c=2.0,
                 evaluate=hash_eval):
    """SelfPlayWorker::self_play (learner_concurrent.rs:169-242) on PyTree.  eta_fn(game id, move
    number, n children) -> the root noise of that search (None: no noise).  -> {game id:
    dict(enc [m][126], policy [m][7], value [m], moves [m])}"""
    L = orc.lib()
    trees = {g: PyTree(evaluate=evaluate, c=c) for g in range(n_games)}
    hist = {g: [] for g in range(n_games)}
    out = {}
    move_no = 0
    while trees:
        for g in sorted(trees):
            tr = trees[g]
            eta = None if eta_fn is None else eta_fn(game_id_base + g, move_no, n_root_children(tr))
            tr.search(sims, eta, eps)
        for g in sorted(trees, reverse=True):
            tr = trees[g]
            vis = np.ascontiguousarray(tr.visits())
            u = L.or_u01_f32(seed, game_id_base + g, move_no)
            idx = L.or_weighted_index(orc._f(vis), len(vis), temperature, u)
            assert idx >= 0, (g, move_no)
            child = tr.root.children[idx]
            hist[g].append((tr.root.state, tr.policy(), child.action))
            v, term = child.state.value_terminated()
            if not term:
                tr.use_subtree(idx)
                continue
            cur = child.state.current_player
            out[game_id_base + g] = dict(
                enc=np.array([s.encoding().reshape(126) for s, _, _ in hist[g]], F32),
                policy=np.array([p for _, p, _ in hist[g]], F32),
                value=np.array([v if s.current_player == cur else -v for s, _, _ in hist[g]], F32),
                moves=np.array([a for _, _, a in hist[g]], np.int32))
            del trees[g]
        move_no += 1
    return out
