"""The CPU side of the chess search's Dirichlet root noise: the yardsticks that
tests/test_chess_root_noise_gpu.py holds the device against are themselves checked
here, and the feature's surface exists.

  dirichlet_stats.check_draws   passes numpy's Dirichlet draws (cast to float32) on
      the whole grid for 5 seeds; fails draws of the wrong alpha, draws of a Gamma
      sampler that forgets the U^(1/alpha) boost of alpha < 1, and rows off by 1e-3
  chess_noise_ref               the hash evaluator as a callback is the oracle's
      built-in one with eps = 0, bit for bit, and a synthetic eta moves the search
"""
import os

import numpy as np
import pytest

import chess_noise_ref as NR
import chess_search_ref as R
import dirichlet_stats as DS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["spai_chess_set_root_noise", "spai_chess_get_root_noise", "spai_chess_root_noise",
               "spai_chess_search_keyed"]


@pytest.fixture(scope="module", autouse=True)
def feature():
    """the library, its Python binding and the headers carry the feature these yardsticks serve"""
    import spai
    import spai_chess as sc
    L = sc.lib()
    for name in NEW_SYMBOLS:
        assert spai.SYMBOLS.count(name) == 1 and hasattr(L, name), name
    return sc


def test_surface(feature):
    sc = feature
    with open(os.path.join(REPO, "include", "spai.h")) as f:
        header = f.read()
    with open(os.path.join(REPO, "rust", "src", "spai_sys.rs")) as f:
        rust = f.read()
    for name in NEW_SYMBOLS:
        assert header.count("int %s(" % name) == 1, name
        assert rust.count("pub fn %s(" % name) == 1, name
    assert "#define SPAI_VERSION_MINOR 5" in header
    assert sc.lib().spai_version().startswith(b"spai 0.5")
    for method in ("set_root_noise", "root_noise", "root_noise_draws"):
        assert hasattr(sc.ChessEngine, method), method
    import inspect
    assert inspect.signature(sc.ChessEngine.__init__).parameters["root_noise"].default is None
    assert inspect.signature(sc.ChessEngine.search).parameters["noise_keys"].default is None
    assert inspect.signature(sc.learn).parameters["root_noise"].default is None
    with open(os.path.join(REPO, "self-play-ai_amd", "Makefile")) as f:
        assert "csrc/dirichlet.h" in f.read()


# ---- the statistical helper
@pytest.mark.parametrize("n,alpha", DS.GRID)
def test_check_draws_passes_numpy(n, alpha):
    for seed in range(5):
        eta = np.random.default_rng([seed, n]).dirichlet([alpha] * n, DS.N_DRAWS).astype(np.float32)
        m = DS.check_draws(eta, alpha)
        print(n, alpha, seed, {k: m[k] for k in ("sum_err", "z_max", "var_ratio", "ks_p")})


@pytest.mark.parametrize("n,alpha", DS.GRID)
def test_check_draws_fails_wrong_alpha(n, alpha):
    eta = np.random.default_rng([11, n]).dirichlet([0.8 * alpha] * n, DS.N_DRAWS).astype(np.float32)
    with pytest.raises(AssertionError):
        DS.check_draws(eta, alpha)


@pytest.mark.parametrize("n,alpha", [g for g in DS.GRID if g[1] < 1.0])
def test_check_draws_fails_forgotten_boost(n, alpha):
    """Gamma(alpha) for alpha < 1 is Gamma(alpha + 1) times U^(1/alpha); without the factor
    the normalised draws are Dirichlet(alpha + 1)"""
    g = np.random.default_rng([12, n]).gamma(alpha + 1.0, size=(DS.N_DRAWS, n))
    eta = (g / g.sum(1, keepdims=True)).astype(np.float32)
    with pytest.raises(AssertionError):
        DS.check_draws(eta, alpha)


@pytest.mark.parametrize("n,alpha", DS.GRID)
def test_check_draws_fails_scaled_rows(n, alpha):
    eta = np.random.default_rng([13, n]).dirichlet([alpha] * n, DS.N_DRAWS).astype(np.float32)
    DS.check_draws(eta, alpha)
    with pytest.raises(AssertionError):
        DS.check_draws((eta * np.float32(1.001)).astype(np.float32), alpha)


def test_check_draws_single_child():
    assert DS.check_draws(np.ones((50, 1), np.float32), 0.3)["sum_err"] == 0.0
    with pytest.raises(AssertionError):
        DS.check_draws(np.full((50, 1), 0.999, np.float32), 0.3)


# ---- the mix and the reference's UCB
def test_mix_is_float32_per_operation():
    p = np.float32([0.1, 0.7, 1.0 / 3.0])
    e = np.float32([0.5, 0.25, 0.0])
    eps = np.float32(0.25)
    om = np.float32(1.0) - eps
    want = [np.float32(np.float32(om * p[i]) + np.float32(eps * e[i])) for i in range(3)]
    got = NR.mix(p, e, 0.25)
    assert got.dtype == np.float32 and got.tobytes() == np.float32(want).tobytes()
    assert NR.mix(p, e, 0.0).tobytes() == p.tobytes()      # eps = 0 is the identity, bit for bit
    assert NR.mix(p, e, 1.0).tobytes() == e.tobytes()


def test_get_ucb_order_and_last_argmax():
    n = np.array([0, 3, 1], np.uint32)
    w = np.float32([0.0, -1.5, 0.25])
    p = np.float32([0.2, 0.5, 0.3])
    u = NR.get_ucb(4, n, w, p, c=2.0)
    want = []
    for k in range(3):
        q = np.float32(0.0) if n[k] == 0 else (np.float32(-w[k] / np.float32(n[k])) + np.float32(1)) / np.float32(2)
        x = np.float32(2.0) * p[k]
        x = np.float32(x * np.sqrt(np.float32(4)))
        x = np.float32(x / (np.float32(1) + np.float32(n[k])))
        want.append(np.float32(q + x))
    assert u.tobytes() == np.float32(want).tobytes()
    assert NR.last_argmax([1.0, 3.0, 3.0, 2.0]) == 2


# ---- the hash evaluator as a callback
@pytest.fixture(scope="module")
def positions():
    import chessref as ch
    ch.lib()
    states = [s for _, _, s in R.positions()]
    yield ch, states
    ch.arena_reset()


def test_callback_with_eps_zero_is_the_builtin_hash_search(positions):
    ch, states = positions
    sims = 48
    rc, pol, ids, vis, mv, nc = ch.search(len(states), sims, states=states)
    assert rc >= 0
    eta = [np.full(len(s.valid_actions()), 1.0 / len(s.valid_actions()), np.float32) for s in states]
    for res in (NR.noised_hash_search(states, sims), NR.noised_hash_search(states, sims, eta=eta, eps=0.0)):
        assert res["evals"] == rc
        assert np.array_equal(res["nc"], nc) and np.array_equal(res["moves"], mv)
        assert np.array_equal(res["visits"], vis) and np.array_equal(res["ids"], ids)
        assert res["policy"].tobytes() == pol.tobytes()
    assert res["mixed"] == list(range(len(states)))   # every root went through the mix, once


def test_callback_with_synthetic_eta_moves_the_search(positions):
    ch, states = positions
    sims = 48
    plain = R.visit_table(NR.noised_hash_search(states, sims))
    eta = []
    for s in states:   # all the noise on the last legal move
        e = np.zeros(len(s.valid_actions()), np.float32)
        e[-1] = 1.0
        eta.append(e)
    noised = NR.noised_hash_search(states, sims, eta=eta, eps=0.5)
    table = R.visit_table(noised)
    moved = [t for t in range(len(states)) if table[t] != plain[t]]
    print(f"visit tables moved by the synthetic eta: {len(moved)} of {len(states)}")
    assert moved
    # the last move's prior is >= 0.5 and every other one's < 0.5: the first selection at the root takes it
    assert all(tb[-1] >= 1 for tb in table)
    assert all(sum(tb) == sims - 1 for tb in table)
    # only the roots are mixed: with eta on trees 0 and 5 alone, the others search as without
    some = [e if t in (0, 5) else None for t, e in enumerate(eta)]
    part = NR.noised_hash_search(states, sims, eta=some, eps=0.5)
    assert part["mixed"] == [0, 5]
    tp = R.visit_table(part)
    assert all(tp[t] == (table[t] if t in (0, 5) else plain[t]) for t in range(len(states)))


def test_extra_positions(positions):
    """the 218-move position and the one-move position are what the GPU test takes them for"""
    ch, _ = positions
    big, one = NR.extra_states()
    assert len(big.valid_actions()) == 218 and big.status == 0
    assert len(one.valid_actions()) == 1 and one.status == 0
