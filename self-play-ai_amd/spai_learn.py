"""What the TicTacToe and chess bindings share on the learner side: the ctypes
wrapper of a device learner (spai_<game>_learner_* in include/spai.h) and the
Learner::learn loop.  spai_ttt and spai_chess subclass and call these; spai.learn
(Connect4) runs the loop on spai.Engine / Net / Learner."""
import ctypes as C
import os
import time

import numpy as np

import spai
from spai import SpaiError


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceLearner:
    """Device train step of a game's net on the engine's device and stream:
    train-mode forward, policy NLL + value MSE, backward, one Adam step.  Mirrors
    spai.Learner.  A subclass sets LIB (the module's lib accessor), PREFIX (the C
    function-name prefix), ENC and POLICY (floats per state and per policy row)."""
    LIB = PREFIX = ENC = POLICY = None

    def _call(self, name, *args):
        """PREFIX_name(*args), an error code raised as SpaiError"""
        L = type(self).LIB()
        rc = getattr(L, f"{self.PREFIX}_{name}")(*args)
        if rc != 0:
            raise SpaiError(rc, L.spai_last_error().decode())

    def __init__(self, engine, blocks, params, **adam):
        cfg = spai.AdamConfig()
        type(self).LIB().spai_adam_config_default(C.byref(cfg))   # fails only on NULL
        for k, v in adam.items():
            setattr(cfg, k, float(v))
        p = np.ascontiguousarray(params, np.float32)
        self.n, self.blocks = p.size, blocks
        self.eng = engine   # the learner runs on the engine's stream: keep it alive
        h = C.c_void_p()
        self._call("create", engine.h, blocks, _p(p), p.size, C.byref(cfg), C.byref(h))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(type(self).LIB(), f"{self.PREFIX}_destroy")(self.h)
            self.h = None

    @classmethod
    def _batch(cls, states, policies, values):
        x = np.ascontiguousarray(states, np.float32).reshape(-1, cls.ENC)
        pi = np.ascontiguousarray(policies, np.float32).reshape(-1, cls.POLICY)
        z = np.ascontiguousarray(values, np.float32).reshape(-1)
        assert len(x) == len(pi) == len(z)
        return x, pi, z

    def train_batch(self, states, policies, values):
        x, pi, z = self._batch(states, policies, values)
        loss = np.zeros(3, np.float32)
        self._call("train_batch", self.h, len(z), _p(x), _p(pi), _p(z), _p(loss))
        return loss   # total, policy, value

    def train(self, states, policies, values, epochs=1, batch=32, seed=0):
        """Model::train (model/mod.rs:100-149): fresh Adam, one permutation, epochs x batches"""
        x, pi, z = self._batch(states, policies, values)
        loss = np.zeros(3, np.float32)
        self._call("train", self.h, len(z), _p(x), _p(pi), _p(z), epochs, batch, seed, _p(loss))
        return loss

    def last_batch(self):
        """the batch size of the latest train step (after train(): the last minibatch's)"""
        n = C.c_uint32()
        self._call("last_batch", self.h, C.byref(n))
        return n.value

    def params(self):
        out = np.zeros(self.n, np.float32)
        self._call("params", self.h, _p(out), self.n)
        return out

    def grads(self):
        out = np.zeros(self.n, np.float32)
        self._call("grads", self.h, _p(out), self.n)
        return out


def _samples(games):
    """self-play games (ascending game id) -> states [n][ENC], policies [n][POLICY], values [n]"""
    games = sorted(games, key=lambda g: g["game"])
    return (np.concatenate([g["enc"] for g in games]), np.concatenate([g["policy"] for g in games]),
            np.concatenate([g["value"] for g in games]))


def _gather(games):
    """learn_loop's default gather: one self-play batch -> (states, policies, values, game ids)"""
    games = sorted(games, key=lambda g: g["game"])
    return _samples(games) + (np.concatenate([np.full(len(g["value"]), g["game"], np.int64) for g in games]),)


def _join(parts, repeat):
    """learn_loop's default join: the batches' dense arrays concatenated, `repeat` times over"""
    s, p, v, g = (np.concatenate([q[k] for q in parts * repeat]) for k in range(4))
    return (s, p, v), (s, p, v, g)


def _iter_seed(seed, i):
    """the training permutation's seed of learn iteration i"""
    return (int(seed) * 0x9E3779B97F4A7C15 + i + 1) & 0xFFFFFFFFFFFFFFFF


def learn_loop(make_engine, make_net, make_learner, params, blocks, hidden, game, num_learn_iters,
               num_self_play_iters, num_parallel_self_play_games, batch_size, num_epochs, seed, checkpoint_dir,
               clone_self_play, on_train_set, self_play_kw=None, refresh=None, on_phase=None, gather=_gather,
               join=_join):
    """Learner::learn (learner.rs:98-196), the body of spai_ttt.learn, spai_chess.learn and
    spai.learn (their docstrings say what it does): make_engine() -> the self-play engine,
    make_net(eng, P) and make_learner(eng, P) on it, self_play_kw the keyword
    arguments of every eng.self_play call, hidden and game what save_params records.
    refresh(net, L) brings the learner's weights into the self-play net before every
    iteration but the first (default: net.set_params(L.params())); on_phase(i, name,
    seconds) receives the host time of iteration i's "refresh", of each of its "self_play"
    batches and of its "train".
    How the samples travel: gather(games) -> one self-play batch's part, and
    join(parts, repeat) -> (the arguments of L.train, the arguments of on_train_set
    after i), repeat being num_self_play_iters under clone_self_play and 1 otherwise;
    the last on_train_set argument holds one game id per training sample.  The
    defaults are dense arrays, concatenated and tiled (spai_chess.learn's compact
    samples replace both)."""
    if refresh is None:
        def refresh(net, L):
            net.set_params(L.params())

    def phase(i, name, t0):
        if on_phase is not None:
            on_phase(i, name, time.perf_counter() - t0)
    P = np.ascontiguousarray(params, np.float32)
    G = num_parallel_self_play_games
    eng = make_engine()
    net = make_net(eng, P)
    eng.set_net(net)
    L = make_learner(eng, P)
    os.makedirs(checkpoint_dir, exist_ok=True)
    out = []
    try:
        for i in range(num_learn_iters):
            if i:
                t0 = time.perf_counter()
                refresh(net, L)
                phase(i, "refresh", t0)
            batches = 1 if clone_self_play else num_self_play_iters
            parts, n_games = [], 0
            for b in range(batches):
                base = (i * num_self_play_iters + b) * G
                t0 = time.perf_counter()
                games, _ = eng.self_play(G, game_id_base=base, **(self_play_kw or {}))
                phase(i, "self_play", t0)
                n_games += len(games)
                parts.append(gather(games))
            train_args, seen = join(parts, num_self_play_iters if clone_self_play else 1)
            if on_train_set is not None:
                on_train_set(i, *seen)
            t0 = time.perf_counter()
            loss = L.train(*train_args, epochs=num_epochs, batch=batch_size, seed=_iter_seed(seed, i))
            phase(i, "train", t0)
            path = os.path.join(checkpoint_dir, f"{i}.safetensors")
            spai.save_params(path, L.params(), blocks, hidden, game=game)   # spai_params_save_safetensors
            out.append(dict(iteration=i, samples=int(len(seen[-1])), loss=[float(x) for x in loss], games=n_games,
                            checkpoint=path))
    finally:
        L.close()
        eng.close()
    return out
