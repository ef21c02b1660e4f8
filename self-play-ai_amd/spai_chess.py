"""ctypes binding of the chess section of libspai.so (include/spai.h).

Mirrors the reference's chess surface (joshua16266261/self-play-ai):
  State (game/chess.rs)            -> ChessEngine.games_* / legal_moves / apply / status / encode / mask_invalid
  Policy::get_channel / get_action -> move_index / index_move
  Net (model/chess.rs)             -> ChessNet.forward
  Tree + Mcts::search (mcts.rs)    -> ChessEngine.trees_create / search / use_subtree
  SelfPlayWorker::self_play        -> ChessEngine.self_play
  play() (main.rs:54-135)          -> ChessEngine.match
  Model::train (model/mod.rs)      -> ChessLearner.train_batch / train
  (compact self-play samples)      -> ChessSamples, self_play(samples="compact"), learn(samples="compact")
  Learner::learn (learner.rs)      -> learn
Every call goes through the HIP library; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

import spai
from spai import EVAL_HASH, EVAL_NET, EVAL_UNIFORM, GAME_CHESS, Config, SelfPlayStats, SpaiError  # noqa: F401
from spai_learn import DeviceLearner, _iter_seed, _samples, learn_loop  # noqa: F401

POLICY, ENC, MAX_MOVES = 4672, 1216, 256

STATE_DTYPE = np.dtype([("pieces", "<u8", 6), ("colors", "<u8", 2), ("side", "u1"), ("castle", "u1"),
                        ("ep", "u1"), ("status", "u1"), ("fifty", "<u2"), ("made", "<u2"), ("reps", "<u4"),
                        ("pad", "<u4")])
assert STATE_DTYPE.itemsize == 80

SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                   C.POINTER(C.c_float), C.POINTER(C.c_uint16))

# spai_chess_sample and its sink
SAMPLE_DTYPE = np.dtype([("state", STATE_DTYPE), ("value", "<f4"), ("move", "<u2"), ("n_children", "<u2"),
                         ("first", "<u4"), ("pad", "<u4")])
assert SAMPLE_DTYPE.itemsize == 96
COMPACT_SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint16),
                           C.POINTER(C.c_uint32), C.c_uint32)


class ChessMatchPlayer(C.Structure):
    _fields_ = [("eval", C.c_int32), ("num_searches", C.c_uint32), ("net", C.c_void_p)]


class ChessMatchConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("opening_plies", C.c_uint32), ("max_plies", C.c_uint32),
                ("moves_stride", C.c_uint32), ("seed", C.c_uint64), ("start", C.c_void_p)]


class ChessMatchGame(C.Structure):
    _fields_ = [("game_id", C.c_uint64), ("a_moves_first", C.c_int8), ("result_a", C.c_int8),
                ("status", C.c_uint8), ("adjudicated", C.c_uint8), ("n_moves", C.c_uint32)]


class ChessMatchStats(C.Structure):
    _fields_ = [(k, C.c_double * 2) for k in ("a_wins", "draws", "b_wins", "sims", "evals")] + \
               [(k, C.c_double) for k in ("adjudicated", "plies", "seconds")]


_ready = False


def lib():
    global _ready
    L = spai.lib()
    if not _ready:
        vp, u32, u64, i32, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER
        L.spai_chess_config_default.argtypes = [P(Config)]
        L.spai_chess_create.argtypes = [P(Config), i32, P(vp)]
        L.spai_chess_destroy.argtypes = [vp]
        L.spai_chess_sync.argtypes = [vp]
        L.spai_chess_games_resize.argtypes = [vp, u32]
        L.spai_chess_games_write.argtypes = [vp, u32, u32, vp]
        L.spai_chess_games_read.argtypes = [vp, u32, u32, vp]
        L.spai_chess_legal_moves.argtypes = [vp, u32, u32, vp, vp]
        L.spai_chess_apply.argtypes = [vp, u32, u32, vp, vp]
        L.spai_chess_status.argtypes = [vp, u32, u32, vp, vp, vp, vp]
        L.spai_chess_encode.argtypes = [vp, u32, u32, vp]
        L.spai_chess_mask_invalid.argtypes = [vp, u32, u32, vp, u32, vp]
        L.spai_chess_move_index.argtypes = [i32, C.c_uint16, P(C.c_int32)]
        L.spai_chess_index_move.argtypes = [i32, C.c_int32, P(C.c_uint16)]
        L.spai_chess_net_num_params.argtypes = [i32, P(C.c_size_t)]
        L.spai_chess_net_init_params.argtypes = [i32, u64, vp]
        L.spai_chess_net_create.argtypes = [vp, i32, vp, C.c_size_t, P(vp)]
        L.spai_chess_net_create_dtype.argtypes = [vp, i32, vp, C.c_size_t, i32, P(vp)]
        L.spai_chess_net_dtype.argtypes = [vp, P(i32)]
        L.spai_chess_net_destroy.argtypes = [vp]
        L.spai_chess_net_forward.argtypes = [vp, u32, vp, vp, vp]
        L.spai_chess_predict.argtypes = [vp, u32, u32, vp, vp]
        L.spai_chess_rules_bench.argtypes = [vp, u32, u32, u32, vp]
        L.spai_chess_perft.argtypes = [vp, u32, C.c_int, vp]
        L.spai_chess_tree_reset.argtypes = [vp, u32, u32]
        L.spai_chess_set_net.argtypes = [vp, vp]
        L.spai_chess_trees_create.argtypes = [vp, u32]
        L.spai_chess_search.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp]
        L.spai_chess_tree_use_subtree.argtypes = [vp, u32, u32]
        L.spai_chess_tree_root.argtypes = [vp, u32, vp, vp, vp]
        L.spai_chess_trees_advance.argtypes = [vp, u32, vp, vp, vp, vp]
        L.spai_chess_selfplay_run.argtypes = [vp, u32, u64, SINK, vp, P(SelfPlayStats)]
        L.spai_chess_selfplay_stream.argtypes = [vp, u32, u32, u64, SINK, vp, P(SelfPlayStats)]
        L.spai_chess_set_timing.argtypes = [vp, i32]
        L.spai_chess_timing.argtypes = [vp, vp, vp, vp]
        L.spai_chess_net_set_params.argtypes = [vp, vp, C.c_size_t]
        L.spai_chess_net_set_params_from_learner.argtypes = [vp, vp]
        L.spai_chess_net_image.argtypes = [vp, vp, C.c_size_t, P(C.c_size_t)]
        L.spai_chess_match_config_default.argtypes = [P(ChessMatchConfig)]
        L.spai_chess_match_run.argtypes = [vp, P(ChessMatchPlayer), P(ChessMatchPlayer), u32, u64,
                                           P(ChessMatchConfig), P(ChessMatchGame), vp, P(ChessMatchStats)]
        L.spai_chess_tree_children.argtypes = [vp, u32, vp, vp, P(u32)]
        L.spai_chess_tree_child_stats.argtypes = [vp, u32, vp, vp, vp, vp, P(u32)]
        L.spai_chess_match_set_one_stream.argtypes = [vp, i32]
        L.spai_chess_learner_create.argtypes = [vp, i32, vp, C.c_size_t, P(spai.AdamConfig), P(vp)]
        L.spai_chess_learner_destroy.argtypes = [vp]
        L.spai_chess_learner_train_batch.argtypes = [vp, u32, vp, vp, vp, vp]
        L.spai_chess_learner_train.argtypes = [vp, u32, vp, vp, vp, u32, u32, u64, vp]
        L.spai_chess_learner_params.argtypes = [vp, vp, C.c_size_t]
        L.spai_chess_learner_grads.argtypes = [vp, vp, C.c_size_t]
        L.spai_chess_learner_activation.argtypes = [vp, i32, vp, C.c_size_t]
        L.spai_chess_learner_last_batch.argtypes = [vp, P(u32)]
        L.spai_chess_learner_set_compute.argtypes = [vp, i32]
        L.spai_chess_learner_get_compute.argtypes = [vp, P(i32)]
        L.spai_chess_learner_set_capture.argtypes = [vp, i32]
        L.spai_chess_learner_gradient.argtypes = [vp, i32, vp, C.c_size_t]
        L.spai_chess_learner_logits.argtypes = [vp, vp, C.c_size_t]
        L.spai_chess_selfplay_compact.argtypes = [vp, u32, u32, u64, COMPACT_SINK, vp, P(SelfPlayStats)]
        L.spai_chess_samples_expand.argtypes = [u32, vp, vp, vp, u32, vp, vp, vp]
        L.spai_chess_learner_train_batch_compact.argtypes = [vp, u32, vp, vp, vp, u32, vp]
        L.spai_chess_learner_train_compact.argtypes = [vp, u32, vp, vp, vp, u32, u32, u32, u32, u64, vp]
        L.spai_chess_learner_batch.argtypes = [vp, vp, vp, vp, u32]
        L.spai_chess_set_root_noise.argtypes = [vp, C.c_float, C.c_float]
        L.spai_chess_get_root_noise.argtypes = [vp, P(C.c_float), P(C.c_float)]
        L.spai_chess_root_noise.argtypes = [vp, u32, vp, vp, vp, C.c_float, vp]
        L.spai_chess_search_keyed.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        _ready = True
    return L


def _check(rc):
    if rc != 0:
        raise SpaiError(rc, lib().spai_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def move_index(side, mv):
    """Policy::get_prob / set_prob index (get_channel, chess.rs:311-393)"""
    out = C.c_int32()
    _check(lib().spai_chess_move_index(side, mv, C.byref(out)))
    return out.value


def index_move(side, index):
    """Policy::get_action (chess.rs:395-493), knight-underpromotion bug kept"""
    out = C.c_uint16()
    _check(lib().spai_chess_index_move(side, index, C.byref(out)))
    return out.value


def num_params(blocks):
    n = C.c_size_t()
    _check(lib().spai_chess_net_num_params(blocks, C.byref(n)))
    return n.value


def init_params(blocks, seed=0):
    p = np.zeros(num_params(blocks), np.float32)
    _check(lib().spai_chess_net_init_params(blocks, seed, _p(p)))
    return p


def states_from(boards):
    """oracle-style boards (pieces[6], color[2], side, castle[2], ep) -> STATE_DTYPE array"""
    a = np.zeros(len(boards), STATE_DTYPE)
    for i, b in enumerate(boards):
        a[i]["pieces"] = b["pieces"]
        a[i]["colors"] = b["colors"]
        a[i]["side"] = b["side"]
        a[i]["castle"] = b["castle"]
        a[i]["ep"] = b["ep"]
        a[i]["fifty"] = b.get("fifty", 0)
        a[i]["made"] = b.get("made", 0)
    return a


class ChessSamples:
    """Compact self-play samples (spai_chess_sample): per sample the searched position,
    the value and the move played (`samples`, SAMPLE_DTYPE), and the root children of
    all of them CSR-style, child_moves (uint16 move codes, MoveGen order) and
    child_visits (uint32 N), sample i owning [first, first + n_children) of both.
    `game` holds each sample's game id.  About 100 bytes plus 6 per legal move instead
    of the 23,556 of the dense form, which expand() builds on the host and
    ChessLearner.train_batch / train build on the device.

    repeat: the set stands for its samples repeated that many times (virtual sample
    j is sample j % n), as learn's clone_self_play repeats a batch of games; len(),
    game and expand() are those of the repeated set, the arrays are stored once."""

    def __init__(self, samples, child_moves, child_visits, game=None, repeat=1):
        self.samples = np.ascontiguousarray(samples, SAMPLE_DTYPE).reshape(-1)
        self.child_moves = np.ascontiguousarray(child_moves, np.uint16).reshape(-1)
        self.child_visits = np.ascontiguousarray(child_visits, np.uint32).reshape(-1)
        if len(self.child_moves) != len(self.child_visits):
            raise ValueError("child_moves and child_visits differ in length")
        self._game = (np.zeros(len(self.samples), np.int64) if game is None
                      else np.ascontiguousarray(game, np.int64).reshape(-1))
        if len(self._game) != len(self.samples):
            raise ValueError("one game id per sample")
        if int(repeat) < 1:
            raise ValueError("repeat must be >= 1")
        self.repeat = int(repeat)

    @property
    def n(self):
        """stored samples (len() counts the repeats)"""
        return len(self.samples)

    def __len__(self):
        return self.n * self.repeat

    @property
    def game(self):
        return np.tile(self._game, self.repeat)

    @property
    def nbytes(self):
        """bytes of the stored sample records and children"""
        return self.samples.nbytes + self.child_moves.nbytes + self.child_visits.nbytes

    def with_repeat(self, repeat):
        """the same arrays (not copied) standing for `repeat` repetitions"""
        return ChessSamples(self.samples, self.child_moves, self.child_visits, self._game, repeat)

    @staticmethod
    def concat(parts):
        """one set of the parts' stored samples in ascending game id (a stable sort: a
        game's samples keep their move order), children packed in that order and `first`
        rebuilt; repeat 1"""
        parts = list(parts)
        if not parts:
            return ChessSamples(np.zeros(0, SAMPLE_DTYPE), [], [])
        smp = np.concatenate([q.samples for q in parts])
        game = np.concatenate([q._game for q in parts])
        base = np.cumsum([0] + [len(q.child_moves) for q in parts[:-1]])
        first = np.concatenate([q.samples["first"].astype(np.int64) + b for q, b in zip(parts, base)])
        smp["first"] = first
        whole = ChessSamples(smp, np.concatenate([q.child_moves for q in parts]),
                             np.concatenate([q.child_visits for q in parts]), game)
        return whole.take(np.argsort(game, kind="stable"))

    def take(self, idx):
        """the stored samples idx, in that order, as a set of their own: their children
        packed in that order and `first` rebuilt; repeat 1"""
        idx = np.asarray(idx, np.int64).reshape(-1)
        smp = self.samples[idx].copy()
        nch = smp["n_children"].astype(np.int64)
        new_first = np.cumsum(nch) - nch
        # entry k of sample i moves from first[i] + k to new_first[i] + k
        src = np.repeat(smp["first"].astype(np.int64) - new_first, nch) + np.arange(int(nch.sum()))
        smp["first"] = new_first
        return ChessSamples(smp, self.child_moves[src], self.child_visits[src], self._game[idx])

    def expand(self):
        """the dense form (enc [len][1216], policy [len][4672], value [len]) through
        spai_chess_samples_expand: what self-play's dense sink hands over, bit for bit"""
        n = self.n
        enc = np.zeros((n, ENC), np.float32)
        pol = np.zeros((n, POLICY), np.float32)
        val = np.zeros(n, np.float32)
        _check(lib().spai_chess_samples_expand(n, _p(self.samples), _p(self.child_moves), _p(self.child_visits),
                                               len(self.child_moves), _p(enc), _p(pol), _p(val)))
        if self.repeat > 1:
            enc, pol, val = np.tile(enc, (self.repeat, 1)), np.tile(pol, (self.repeat, 1)), np.tile(val, self.repeat)
        return enc, pol, val


class ChessEngine:
    def __init__(self, num_searches=400, max_trees=1024, eval_kind=EVAL_NET, device=0, c=2.0, temperature=1.25,
                 seed=0, max_moves=None, root_noise=None):
        """root_noise: None (the default: the reference's noise-free search) or (alpha,
        eps), the Dirichlet root noise of self-play and keyed searches (set_root_noise)"""
        cfg = Config()
        _check(lib().spai_chess_config_default(C.byref(cfg)))
        cfg.c, cfg.num_searches, cfg.temperature = c, num_searches, temperature
        cfg.max_trees, cfg.eval, cfg.seed = max_trees, eval_kind, seed
        if max_moves is not None:
            cfg.max_moves = max_moves
        self.cfg = cfg
        h = C.c_void_p()
        _check(lib().spai_chess_create(C.byref(cfg), device, C.byref(h)))
        self.h = h
        self.net = None
        if root_noise is not None:
            try:
                self.set_root_noise(*root_noise)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            if self.net is not None:
                self.net.close()
                self.net = None
            lib().spai_chess_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- rules
    def games_resize(self, n):
        _check(lib().spai_chess_games_resize(self.h, n))

    def games_write(self, states, first=0):
        a = np.ascontiguousarray(states, STATE_DTYPE)
        _check(lib().spai_chess_games_write(self.h, first, len(a), _p(a)))

    def games_read(self, n, first=0):
        a = np.zeros(n, STATE_DTYPE)
        _check(lib().spai_chess_games_read(self.h, first, n, _p(a)))
        return a

    def legal_moves(self, n, first=0):
        mv = np.zeros((n, MAX_MOVES), np.uint16)
        cnt = np.zeros(n, np.uint32)
        _check(lib().spai_chess_legal_moves(self.h, first, n, _p(mv), _p(cnt)))
        return mv, cnt

    def apply(self, moves, first=0, check=True):
        m = np.ascontiguousarray(moves, np.uint16)
        rc = np.zeros(len(m), np.int32)
        r = lib().spai_chess_apply(self.h, first, len(m), _p(m), _p(rc))
        if check:
            _check(r)
        return rc

    def status(self, n, first=0):
        st = np.zeros(n, np.uint8)
        reps = np.zeros(n, np.uint32)
        v = np.zeros(n, np.float32)
        term = np.zeros(n, np.uint8)
        _check(lib().spai_chess_status(self.h, first, n, _p(st), _p(reps), _p(v), _p(term)))
        return st, reps, v, term

    def rules_bench(self, n, first=0, iters=10):
        """device ms per launch: [legal moves + status, encoding] over slots [first, first+n)"""
        ms = np.zeros(2, np.float64)
        _check(lib().spai_chess_rules_bench(self.h, first, n, iters, _p(ms)))
        return ms

    def perft(self, depth, slot=0):
        """[perft(1), ..., perft(depth)] of slot `slot`'s position, on the device"""
        out = np.zeros(depth, np.uint64)
        _check(lib().spai_chess_perft(self.h, slot, depth, _p(out)))
        return [int(v) for v in out]

    def encode(self, n, first=0):
        out = np.zeros((n, 19, 8, 8), np.float32)
        _check(lib().spai_chess_encode(self.h, first, n, _p(out)))
        return out

    def mask_invalid(self, policy, first=0):
        p = np.ascontiguousarray(policy, np.float32)
        p2 = p.reshape(p.shape[0], -1)
        out = np.zeros((p2.shape[0], POLICY), np.float32)
        _check(lib().spai_chess_mask_invalid(self.h, first, p2.shape[0], _p(p2), p2.shape[1], _p(out)))
        return out

    # ---- net / search
    def set_net(self, net):
        _check(lib().spai_chess_set_net(self.h, net.h if net else None))
        self.net = net

    def trees_create(self, n):
        _check(lib().spai_chess_trees_create(self.h, n))

    def set_root_noise(self, alpha, eps):
        """Dirichlet(alpha) root noise of weight eps in self-play and in keyed searches
        (search(noise_keys=...)); eps = 0 (the default of a new engine) turns it off, and
        the search is then the reference's.  Plain searches and matches never use it.
        alpha in [0.01, 100], eps in [0, 1]."""
        _check(lib().spai_chess_set_root_noise(self.h, float(alpha), float(eps)))

    def root_noise(self):
        """(alpha, eps) as set; eps 0.0 = off"""
        a, e = C.c_float(), C.c_float()
        _check(lib().spai_chess_get_root_noise(self.h, C.byref(a), C.byref(e)))
        return a.value, e.value

    def root_noise_draws(self, game_ids, move_nos, n_children, alpha=None):
        """the Dirichlet draws the search makes for these keys, by its own device
        function: float32 [len][MAX_MOVES], row i zero from n_children[i] on.
        alpha None: the engine's"""
        g = np.ascontiguousarray(game_ids, np.uint64).reshape(-1)
        m = np.ascontiguousarray(move_nos, np.uint32).reshape(-1)
        k = np.ascontiguousarray(n_children, np.uint32).reshape(-1)
        if not len(g) == len(m) == len(k):
            raise ValueError("one game id, move number and child count per draw")
        a = self.root_noise()[0] if alpha is None else float(alpha)
        eta = np.zeros((len(g), MAX_MOVES), np.float32)
        _check(lib().spai_chess_root_noise(self.h, len(g), _p(g), _p(m), _p(k), a, _p(eta)))
        return eta

    def search(self, trees, num_searches=None, noise_keys=None):
        """Mcts::search over the listed trees.  noise_keys=(game_ids, move_nos), one pair
        per tree: the keyed call (spai_chess_search_keyed), which mixes the engine's root
        noise into each root under that key; without it, or with eps = 0, the plain search"""
        idx = np.ascontiguousarray(trees, np.uint32)
        n = len(idx)
        pol = np.zeros((n, POLICY), np.float32)
        ids = np.zeros((n, MAX_MOVES), np.uint32)
        vis = np.zeros((n, MAX_MOVES), np.float32)
        mv = np.zeros((n, MAX_MOVES), np.uint16)
        nc = np.zeros(n, np.uint32)
        ns = self.cfg.num_searches if num_searches is None else num_searches
        if noise_keys is None:
            _check(lib().spai_chess_search(self.h, n, _p(idx), ns, _p(pol), _p(ids), _p(vis), _p(mv), _p(nc)))
        else:
            g = np.ascontiguousarray(noise_keys[0], np.uint64).reshape(-1)
            m = np.ascontiguousarray(noise_keys[1], np.uint32).reshape(-1)
            if not len(g) == len(m) == n:
                raise ValueError("noise_keys: one game id and one move number per tree")
            _check(lib().spai_chess_search_keyed(self.h, n, _p(idx), _p(g), _p(m), ns, _p(pol), _p(ids), _p(vis),
                                                 _p(mv), _p(nc)))
        return pol, ids, vis, mv, nc

    def tree_reset(self, tree, slot):
        """Tree::with_root_state(state of game slot `slot`)"""
        _check(lib().spai_chess_tree_reset(self.h, tree, slot))

    def use_subtree(self, tree, child_index):
        _check(lib().spai_chess_tree_use_subtree(self.h, tree, child_index))

    def advance(self, trees, child_index):
        t = np.ascontiguousarray(trees, np.uint32)
        k = np.ascontiguousarray(child_index, np.uint32)
        st = np.zeros(len(t), np.uint8)
        reps = np.zeros(len(t), np.uint32)
        _check(lib().spai_chess_trees_advance(self.h, len(t), _p(t), _p(k), _p(st), _p(reps)))
        return st, reps

    def tree_root(self, tree):
        st = np.zeros(1, STATE_DTYPE)
        n = C.c_uint32()
        w = C.c_float()
        _check(lib().spai_chess_tree_root(self.h, tree, _p(st), C.byref(n), C.byref(w)))
        return st[0], n.value, w.value

    def tree_children(self, tree):
        """root children of a tree without searching it: (moves uint16 [n], visits uint32 [n]);
        n = 0 while the root is not expanded"""
        mv = np.zeros(MAX_MOVES, np.uint16)
        vis = np.zeros(MAX_MOVES, np.uint32)
        n = C.c_uint32()
        _check(lib().spai_chess_tree_children(self.h, tree, _p(mv), _p(vis), C.byref(n)))
        return mv[:n.value].copy(), vis[:n.value].copy()

    def tree_child_stats(self, tree):
        """root children of a tree in stored (MoveGen) order, each exactly as its node record
        holds it: (moves uint16 [n], visits uint32 [n], value_sums float32 [n], priors float32 [n]);
        n = 0 while the root is not expanded.  Read-only: no search, the tree is unchanged"""
        mv = np.zeros(MAX_MOVES, np.uint16)
        vis = np.zeros(MAX_MOVES, np.uint32)
        w = np.zeros(MAX_MOVES, np.float32)
        pr = np.zeros(MAX_MOVES, np.float32)
        n = C.c_uint32()
        _check(lib().spai_chess_tree_child_stats(self.h, tree, _p(mv), _p(vis), _p(w), _p(pr), C.byref(n)))
        k = n.value
        return mv[:k].copy(), vis[:k].copy(), w[:k].copy(), pr[:k].copy()

    def match(self, a, b, n_games, game_id_base=0, opening_plies=2, max_plies=512, seed=0, start=None,
              keep_moves=True):
        """play() (main.rs:54-135) between two players over n_games chess games
        (spai_chess_match_run).  A player is (eval_kind, ChessNet or None, num_searches).
        Game i has id game_id_base + i; A plays the first searched ply of the even ids,
        and both games of a pair (id // 2) share their start: start[pair - game_id_base
        // 2] (a STATE_DTYPE array, opening_plies must be 0) or the start position plus
        opening_plies drawn plies.  A game still Ongoing at max_plies plies (0: no limit)
        is adjudicated a draw.  Returns (games, stats): per game a dict (game,
        a_moves_first, result_a = +1 A won / 0 draw / -1 B won, status, adjudicated,
        n_moves, moves np.uint16 or None), and the counts split by who moved first
        ([0]: A), per-player sims and evals, adjudicated, plies, seconds."""
        cfg = ChessMatchConfig()
        _check(lib().spai_chess_match_config_default(C.byref(cfg)))
        cfg.opening_plies, cfg.max_plies, cfg.seed = opening_plies, max_plies, seed
        st_arr = None
        if start is not None:
            st_arr = np.ascontiguousarray(start, STATE_DTYPE)
            n_pairs = (game_id_base + max(n_games, 1) - 1) // 2 - game_id_base // 2 + 1
            if len(st_arr) < n_pairs:
                raise ValueError(f"start holds {len(st_arr)} positions, the match has {n_pairs} pairs")
            cfg.start = st_arr.ctypes.data
        mv = None
        if keep_moves:
            # longest game: the ply limit, else the engine's history bound plus the opening
            stride = max_plies if max_plies else self.cfg.max_moves + 4
            stride = max(int(stride), int(opening_plies), 1)
            cfg.moves_stride = stride
            mv = np.zeros((max(n_games, 1), stride), np.uint16)
        pl = [ChessMatchPlayer(int(kind), int(sims), net.h if net is not None else None) for kind, net, sims in (a, b)]
        out = (ChessMatchGame * max(n_games, 1))()
        st = ChessMatchStats()
        _check(lib().spai_chess_match_run(self.h, C.byref(pl[0]), C.byref(pl[1]), n_games, game_id_base,
                                          C.byref(cfg), out, _p(mv) if mv is not None else None, C.byref(st)))
        games = [dict(game=int(g.game_id), a_moves_first=bool(g.a_moves_first), result_a=int(g.result_a),
                      status=int(g.status), adjudicated=bool(g.adjudicated), n_moves=int(g.n_moves),
                      moves=mv[i, :min(g.n_moves, mv.shape[1])].copy() if mv is not None else None)
                 for i, g in enumerate(out[:n_games])]
        stats = {k: [float(v) for v in getattr(st, k)] for k in ("a_wins", "draws", "b_wins", "sims", "evals")}
        for k in ("adjudicated", "plies", "seconds"):
            stats[k] = float(getattr(st, k))
        return games, stats

    def match_one_stream(self, on=True):
        """measurement only: both chains of later matches on the engine's stream (default: two streams)"""
        _check(lib().spai_chess_match_set_one_stream(self.h, 1 if on else 0))

    def self_play(self, n_games, game_id_base=0, keep=True, keep_policy=True, window=None, samples="dense"):
        """SelfPlayWorker::self_play over n_games games; window: play them through
        that many tree slots (spai_chess_selfplay_stream), games in finishing order.
        samples="compact" (spai_chess_selfplay_compact): the same games, each game's
        dict holding game, n and samples, a ChessSamples, instead of the dense enc /
        policy / value / moves arrays (which its expand() and samples["move"] give back)"""
        if samples not in ("dense", "compact"):
            raise ValueError(f'samples must be "dense" or "compact", got {samples!r}')
        games = []
        if samples == "compact":
            def csink(user, gid, n, smp, mv, vis, total):
                if keep:
                    a = np.frombuffer(C.string_at(smp, n * SAMPLE_DTYPE.itemsize), SAMPLE_DTYPE).copy()
                    games.append(dict(game=gid, n=n, samples=ChessSamples(
                        a, np.ctypeslib.as_array(mv, (total,)).copy(), np.ctypeslib.as_array(vis, (total,)).copy(),
                        np.full(n, gid, np.int64))))

            ccb = COMPACT_SINK(csink)
            st = SelfPlayStats()
            _check(lib().spai_chess_selfplay_compact(self.h, n_games, 0 if window is None else int(window),
                                                     game_id_base, ccb, None, C.byref(st)))
            return games, {k: getattr(st, k) for k, _ in SelfPlayStats._fields_}

        def sink(user, gid, n, enc, pol, val, moves):
            if keep:
                g = dict(game=gid, n=n,
                         enc=np.ctypeslib.as_array(enc, (n, ENC)).copy(),
                         value=np.ctypeslib.as_array(val, (n,)).copy(),
                         moves=np.ctypeslib.as_array(moves, (n,)).copy())
                if keep_policy:
                    g["policy"] = np.ctypeslib.as_array(pol, (n, POLICY)).copy()
                games.append(g)

        cb = SINK(sink)
        st = SelfPlayStats()
        if window is None:
            _check(lib().spai_chess_selfplay_run(self.h, n_games, game_id_base, cb, None, C.byref(st)))
        else:
            _check(lib().spai_chess_selfplay_stream(self.h, n_games, int(window), game_id_base, cb, None, C.byref(st)))
        return games, {k: getattr(st, k) for k, _ in SelfPlayStats._fields_}

    def set_timing(self, on=True):
        _check(lib().spai_chess_set_timing(self.h, 1 if on else 0))

    def timing(self):
        ms = np.zeros(3)
        launches = np.zeros(3)
        items = np.zeros(3)
        _check(lib().spai_chess_timing(self.h, _p(ms), _p(launches), _p(items)))
        return ms, launches, items


class ChessNet:
    """dtype "bf16" (the default: the MFMA throughput path) or "f32": the reference's own
    fp32 arithmetic on unrounded input planes, every output summed in one fixed order
    (spai.h), bit-exact against tests/chess_f32_ref.py and about 50 times slower
    (profiles/chess_net_f32).  Either kind serves forward, predict, search, self-play and match."""
    DTYPES = {"bf16": 0, "f32": 1}   # spai_dtype

    def __init__(self, eng, blocks, params, dtype="bf16"):
        if dtype not in self.DTYPES:
            raise ValueError(f"dtype {dtype!r}: 'bf16' or 'f32'")
        p = np.ascontiguousarray(params, np.float32)
        h = C.c_void_p()
        if dtype == "bf16":
            _check(lib().spai_chess_net_create(eng.h, blocks, _p(p), p.size, C.byref(h)))
        else:
            _check(lib().spai_chess_net_create_dtype(eng.h, blocks, _p(p), p.size, self.DTYPES[dtype], C.byref(h)))
        self.h = h
        self.eng = eng
        self.blocks = blocks
        d = C.c_int()
        _check(lib().spai_chess_net_dtype(h, C.byref(d)))
        self.dtype = {v: k for k, v in self.DTYPES.items()}[d.value]

    def close(self):
        if getattr(self, "h", None):
            lib().spai_chess_net_destroy(self.h)
            self.h = None

    def forward(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 19 * 64)
        n = x.shape[0]
        lg = np.zeros((n, POLICY), np.float32)
        v = np.zeros(n, np.float32)
        _check(lib().spai_chess_net_forward(self.h, n, _p(x), _p(lg), _p(v)))
        return lg, v

    def predict(self, n, first=0):
        """Model::predict over the engine's game slots [first, first+n)"""
        pr = np.zeros((n, POLICY), np.float32)
        v = np.zeros(n, np.float32)
        _check(lib().spai_chess_predict(self.h, first, n, _p(pr), _p(v)))
        return pr, v

    def set_params(self, params_or_learner):
        """weight refresh in place, folded and packed by HIP kernels: every packed word
        (image()), and so forward afterwards, is bit-identical to a fresh ChessNet of the
        same parameters.  The source is a float32 array (spai_chess_net_set_params), or a
        ChessLearner, whose device parameters are read in place with no host copy and no
        host synchronisation (spai_chess_net_set_params_from_learner); the net then holds
        a snapshot of them."""
        if isinstance(params_or_learner, ChessLearner):
            _check(lib().spai_chess_net_set_params_from_learner(self.h, params_or_learner.h))
        else:
            p = np.ascontiguousarray(params_or_learner, np.float32)
            _check(lib().spai_chess_net_set_params(self.h, _p(p), p.size))

    def image(self):
        """the net's packed weight buffers as a uint8 array, in spai_chess_net_image's order"""
        n = C.c_size_t()
        _check(lib().spai_chess_net_image(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        _check(lib().spai_chess_net_image(self.h, _p(out), out.size, C.byref(n)))
        return out


class ChessLearner(DeviceLearner):
    """Device train step of the chess net (model/chess.rs under
    model/mod.rs:128-141) on the engine's device and stream: train-mode forward,
    policy NLL + value MSE, backward, one Adam step.  Mirrors spai_ttt.TTTLearner.
    compute: "f32" (the default, exact fp32) or "bf16" (the conv GEMMs' operands
    rounded to bf16, fp32 sums; everything else fp32: spai.h)."""
    LIB, PREFIX, ENC, POLICY = staticmethod(lib), "spai_chess_learner", ENC, POLICY
    COMPUTE = {"f32": 1, "bf16": 0}   # spai_dtype

    def __init__(self, engine, blocks, params, compute="f32", **adam):
        super().__init__(engine, blocks, params, **adam)
        if compute != "f32":
            self.set_compute(compute)

    def train_batch(self, states, policies=None, values=None):
        """one train step on dense arrays, or on a ChessSamples (given alone), whose dense
        form a HIP kernel writes on the device from the uploaded records: the same bits"""
        if not isinstance(states, ChessSamples):
            return super().train_batch(states, policies, values)
        cs = states
        if policies is not None or values is not None:
            raise ValueError("a ChessSamples is given alone")
        if cs.repeat != 1:
            raise ValueError("train_batch takes the samples as they are (repeat 1); train() repeats them")
        loss = np.zeros(3, np.float32)
        self._call("train_batch_compact", self.h, cs.n, _p(cs.samples), _p(cs.child_moves), _p(cs.child_visits),
                   len(cs.child_moves), _p(loss))
        return loss

    def train(self, states, policies=None, values=None, epochs=1, batch=32, seed=0):
        """Model::train on dense arrays, or on a ChessSamples (given alone): over its
        len() = n * repeat virtual samples, bit-identical to train(*samples.expand()),
        with neither the dense arrays nor the repeats ever built on the host"""
        if not isinstance(states, ChessSamples):
            return super().train(states, policies, values, epochs=epochs, batch=batch, seed=seed)
        cs = states
        if policies is not None or values is not None:
            raise ValueError("a ChessSamples is given alone")
        loss = np.zeros(3, np.float32)
        self._call("train_compact", self.h, cs.n, _p(cs.samples), _p(cs.child_moves), _p(cs.child_visits),
                   len(cs.child_moves), cs.repeat, epochs, batch, seed, _p(loss))
        return loss

    def batch(self):
        """the last train step's batch as the step read it on the device, whichever route
        brought it there: (enc [B][1216], policy [B][4672], value [B])"""
        B = self.last_batch()
        enc = np.zeros((B, ENC), np.float32)
        pol = np.zeros((B, POLICY), np.float32)
        val = np.zeros(B, np.float32)
        self._call("batch", self.h, _p(enc), _p(pol), _p(val), B)
        return enc, pol, val

    def set_compute(self, compute):
        """between steps: parameters, Adam moments and step count are kept"""
        if compute not in self.COMPUTE:
            raise ValueError(f"compute {compute!r}: 'f32' or 'bf16'")
        self._call("set_compute", self.h, self.COMPUTE[compute])

    def compute(self):
        d = C.c_int32()
        self._call("get_compute", self.h, C.byref(d))
        return {v: k for k, v in self.COMPUTE.items()}[d.value]

    def set_capture(self, on):
        """keep the gradients a step otherwise overwrites (for gradient()); changes no result"""
        self._call("set_capture", self.h, int(bool(on)))

    def gradient(self, layer):
        """of the last (captured) train step: layers 0 .. 2*blocks the gradient of that
        trunk conv's pre-BN output, 2*blocks+1 the masked gradient of the first policy
        conv, [B][256][8][8]; 2*blocks+2 the logits' gradient, [B][4672]"""
        nt, B = 2 * self.blocks + 1, self.last_batch()
        out = np.zeros((B, 256, 8, 8) if layer <= nt else (B, POLICY), np.float32)
        self._call("gradient", self.h, layer, _p(out), out.size)
        return out

    def logits(self):
        """the last train step's logits [B][4672]"""
        out = np.zeros((self.last_batch(), POLICY), np.float32)
        self._call("logits", self.h, _p(out), out.size)
        return out

    def activation(self, layer):
        """the last train step's post-ReLU activations: layers 0 .. 2*blocks the trunk
        convs and 2*blocks+1 the first policy conv, [B][256][8][8]; 2*blocks+2 the value
        conv, [B][64]; 2*blocks+3 the first value linear, [B][256]"""
        nt, B = 2 * self.blocks + 1, self.last_batch()
        shape = (B, 256, 8, 8) if layer <= nt else (B, 64) if layer == nt + 1 else (B, 256)
        out = np.zeros(shape, np.float32)
        _check(lib().spai_chess_learner_activation(self.h, layer, _p(out), out.size))
        return out


def learn(num_learn_iters=10, num_self_play_iters=500, num_parallel_self_play_games=100, batch_size=32, num_epochs=4,
          num_searches=600, temperature=1.25, c=2.0, blocks=10, seed=0, checkpoint_dir=".", clone_self_play=True,
          params=None, device=0, on_train_set=None, window=None, max_moves=None, compute="f32", refresh="device",
          on_phase=None, samples="dense", root_noise=None):
    """Learner::learn (learner.rs:98-196) for chess, with mcts.rs:46-59's defaults:
    per iteration i, self-play with the current weights on one ChessEngine (the net
    refreshed in place), Model::train on the samples, checkpoint i.safetensors.

    clone_self_play (the reference's behaviour, learner.rs:127-137: the self-play
    state is cloned into every self-play iteration, so all of them play the same
    games): one batch of num_parallel_self_play_games games, its samples repeated
    num_self_play_iters times.  False: num_self_play_iters distinct batches.  Game
    ids (the sampling streams) are disjoint across batches and learn iterations.
    window: play each batch through that many tree slots (ChessEngine.self_play).
    on_train_set(i, states, policies, values, game_ids) sees every training set.
    compute: the train step's compute type, "f32" or "bf16" (ChessLearner).
    refresh: how the learner's weights reach the self-play net -- "device":
    ChessNet.set_params(learner), folded and packed by HIP kernels from the learner's
    device parameters; "host": ChessNet.set_params(learner.params()), the same kernels
    behind a host round trip.  Both give the same bits.  on_phase(i, name, seconds)
    receives the host time of each phase (learn_loop).
    samples: "dense" (the default), or "compact": self-play hands over ChessSamples
    and the learner expands them on the device, so the loop never builds a dense
    array; clone_self_play then trains with repeat=num_self_play_iters instead of
    tiling, and on_train_set(i, samples, None, None, game_ids) receives the
    ChessSamples.  Both give the same checkpoints, byte for byte.
    root_noise: None (the default: the reference's noise-free search) or (alpha, eps),
    Dirichlet noise at every self-play root (ChessEngine.set_root_noise).
    Returns per-iteration records: samples, loss [total, policy, value] of the last
    step, games, checkpoint."""
    G = num_parallel_self_play_games
    if compute not in ChessLearner.COMPUTE:
        raise ValueError(f"compute {compute!r}: 'f32' or 'bf16'")
    if refresh not in ("device", "host"):
        raise ValueError(f'refresh must be "device" or "host", got {refresh!r}')
    if samples not in ("dense", "compact"):
        raise ValueError(f'samples must be "dense" or "compact", got {samples!r}')
    hooks = {}
    if samples == "compact":
        def join(parts, repeat):
            cs = ChessSamples.concat(parts).with_repeat(repeat)
            return (cs,), (cs, None, None, cs.game)

        hooks = dict(gather=lambda games: ChessSamples.concat(g["samples"] for g in games), join=join)
    return learn_loop(
        lambda: ChessEngine(num_searches=num_searches, max_trees=G if window is None else int(window),
                            eval_kind=EVAL_NET, device=device, c=c, temperature=temperature, seed=seed,
                            max_moves=max_moves, root_noise=root_noise),
        lambda eng, P: ChessNet(eng, blocks, P), lambda eng, P: ChessLearner(eng, blocks, P, compute=compute),
        init_params(blocks, seed) if params is None else params, blocks, 256, GAME_CHESS, num_learn_iters,
        num_self_play_iters, G, batch_size, num_epochs, seed, checkpoint_dir, clone_self_play, on_train_set,
        self_play_kw=dict(window=window, samples=samples),
        refresh=(lambda net, L: net.set_params(L)) if refresh == "device" else None, on_phase=on_phase, **hooks)
