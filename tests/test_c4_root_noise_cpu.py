"""The CPU side of the Connect4 search's Dirichlet root noise: the yardsticks of
tests/test_c4_root_noise_gpu.py (tests/c4_noise_ref.py) are themselves pinned here,
and the feature's surface exists.  None of this runs device code.

  (b) PyTree, noise off, under the hash evaluator, to the bit:
        against c4_search_ref.RefSearch's records (N, W, P of root and children) on
        positions(12, SEED), across two advance steps, and against oracle.self_play
        on 4 games at 16 simulations
  (a) NoisedSearch against (b) with noise on, for fresh roots
  the yardstick reacts: eta applied to the wrong tree, eta rolled by one child, and
        the mix applied after the first selection instead of before each change some
        visit count at 32 simulations on these positions (SEED chosen here so they do)
"""
import inspect
import os

import numpy as np
import pytest

import c4_noise_ref as NR
import c4_search_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["spai_set_root_noise", "spai_get_root_noise", "spai_root_noise", "spai_search_keyed"]
# SEED (of the positions and of the synthetic eta): the first of 1..399 at which the late mix
# changes a visit count at 32 simulations.  It rarely does: the first selection visits another
# child, but by 32 simulations both orders have usually visited the same nodes (21 of the 399
# seeds react, each in one tree), which is why the GPU test's launch regimes run at 8 simulations
SEED, NPOS, SIMS, EPS, ALPHA = 16, 12, 32, 0.25, 0.3


@pytest.fixture(scope="module")
def pos(oracle):
    p = R.positions(NPOS, SEED)
    assert any(s.n == 0 for s in p) and any(R.has_full_column(s) for s in p) and any(R.wins_in_one(s) for s in p)
    return p


@pytest.fixture(scope="module")
def eta(pos):
    rng = np.random.default_rng(SEED)
    return [rng.dirichlet([ALPHA] * len(s.valid_actions())).astype(np.float32) for s in pos]


def test_surface():
    import spai
    L = spai.lib()
    for name in NEW_SYMBOLS:
        assert spai.SYMBOLS.count(name) == 1 and hasattr(L, name), name
    with open(os.path.join(REPO, "include", "spai.h")) as f:
        header = f.read()
    with open(os.path.join(REPO, "rust", "src", "spai_sys.rs")) as f:
        rust = f.read()
    for name in NEW_SYMBOLS:
        assert header.count("int %s(" % name) == 1, name
        assert rust.count("pub fn %s(" % name) == 1, name
    for method in ("set_root_noise", "get_root_noise", "root_noise_draws"):
        assert hasattr(spai.Engine, method), method
    assert inspect.signature(spai.Engine.__init__).parameters["root_noise"].default is None
    assert inspect.signature(spai.Engine.search).parameters["noise_keys"].default is None
    assert inspect.signature(spai.learn).parameters["root_noise"].default is None


def _same_records(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert R.same_bits(g, w), (what, i, g, w)


# ---- (b), noise off, against the oracle
def test_py_search_is_the_oracles_search(pos):
    ev = R.Evaluator(NR.hash_predict)
    rs = R.RefSearch(pos, ev)
    trees = [NR.PyTree(s) for s in pos]
    try:
        for step in range(3):                       # a search, then two advance steps
            r = rs.search(SIMS)
            for t, tr in enumerate(trees):
                tr.search(SIMS)
                k = int(r["nc"][t])
                assert len(tr.root.children) == k, (step, t)
                n_root, w_root = rs.root(t)
                assert tr.root_record()[0] == n_root and R.same_bits(tr.root_record()[1], w_root), (step, t)
                _same_records(tr.children(), rs.children(t), (step, t))
                assert R.same_bits(tr.visits(), r["visits"][t, :k]) and R.same_bits(tr.policy(), r["policy"][t]), (step, t)
            assert sum(tr.evals for tr in trees) == ev.leaves
            for t, tr in enumerate(trees):           # advance where the game goes on
                k = R.most_visited_last(r["visits"][t], int(r["nc"][t]))
                if tr.root.children[k].state.status == 0:
                    rs.advance(t, k)
                    tr.use_subtree(k)
    finally:
        rs.close()


def test_py_self_play_is_the_oracles_self_play(oracle):
    n, sims, seed = 4, 16, 7
    ref = oracle.self_play(oracle.GAME_CONNECT4, n, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42)
    got = NR.py_self_play(n, sims, seed)
    assert sorted(got) == list(range(n))
    for g in range(n):
        rows = np.flatnonzero(ref["game"] == g)
        assert np.array_equal(ref["ply"][rows], np.arange(len(rows))), g
        for k in ("enc", "policy", "value"):
            assert R.same_bits(got[g][k], ref[k][rows]), (g, k)
        assert R.same_bits(got[g]["moves"], ref["moves"][g, :ref["n_moves"][g]]), g
    based = NR.py_self_play(2, sims, seed, game_id_base=5)
    ref5 = oracle.self_play(oracle.GAME_CONNECT4, 2, sims, seed, eval_kind=oracle.EVAL_HASH, max_plies=42,
                            game_id_base=5)
    for g in range(2):
        assert R.same_bits(based[5 + g]["moves"], ref5["moves"][g, :ref5["n_moves"][g]]), g


# ---- (a) against (b), noise on, fresh roots
def _visit_table(trees):
    return [tuple(int(v) for v in tr.visits()) for tr in trees]


def test_noised_callback_is_py_search(pos, eta):
    plain = NR.noised_search(pos, SIMS)
    assert plain["mixed"] == []
    _same_records([tr.visits() for tr in NR.py_search(pos, SIMS)],
                  [plain["visits"][t, :plain["nc"][t]] for t in range(NPOS)], "eps 0")
    a = NR.noised_search(pos, SIMS, eta=eta, eps=EPS)
    b = NR.py_search(pos, SIMS, eta=eta, eps=EPS)
    assert a["mixed"] == list(range(NPOS))          # every root went through the mix, once
    for t, tr in enumerate(b):
        k = int(a["nc"][t])
        _same_records(tr.children(), a["records"][t], t)
        assert tr.root_record()[0] == a["roots"][t][0] and R.same_bits(tr.root_record()[1], a["roots"][t][1]), t
        assert R.same_bits(tr.visits(), a["visits"][t, :k]) and R.same_bits(tr.policy(), a["policy"][t]), t
    # the priors are the mix of the plain ones, and nothing else of the first expansion moved
    for t in range(NPOS):
        assert R.same_bits(a["records"][t][3], NR.mix(plain["records"][t][3], eta[t], EPS)), t
    moved = [t for t in range(NPOS) if _visit_table(b)[t] != tuple(int(v) for v in plain["visits"][t, :plain["nc"][t]])]
    print(f"trees whose visit counts the noise moved: {len(moved)} of {NPOS}")
    assert moved
    # two trees on one position carry different eta
    two = [pos[0], pos[0]]
    e2 = [eta[0], np.roll(eta[0], 1)]
    a2, b2 = NR.noised_search(two, SIMS, eta=e2, eps=EPS), NR.py_search(two, SIMS, eta=e2, eps=EPS)
    for t in range(2):
        _same_records(b2[t].children(), a2["records"][t], ("twins", t))
    assert not R.same_bits(a2["records"][0][3], a2["records"][1][3])


def test_reused_root_mix(pos, eta):
    """(b) mixes a root that kept its subtree: on entry, once per call, nothing else written"""
    tr = NR.PyTree(pos[0])
    tr.search(SIMS)
    tr.use_subtree(last := NR.last_argmax(tr.visits()))
    before = tr.children()
    n0 = tr.root_record()
    e = np.random.default_rng(5).dirichlet([ALPHA] * len(before[0])).astype(np.float32)
    tr.search(0, eta=e, eps=EPS)
    after = tr.children()
    assert R.same_bits(after[3], NR.mix(before[3], e, EPS)) and tr.root_record()[0] == n0[0]
    _same_records(after[:3], before[:3], last)
    tr.search(0, eta=e, eps=EPS)                    # a second call without a move mixes again
    assert R.same_bits(tr.children()[3], NR.mix(NR.mix(before[3], e, EPS), e, EPS))


# ---- the yardstick reacts
def test_yardstick_reacts(pos, eta):
    good = _visit_table(NR.py_search(pos, SIMS, eta=eta, eps=EPS))
    by_n = {}
    for t, s in enumerate(pos):
        by_n.setdefault(len(s.valid_actions()), []).append(t)
    # eta applied to the wrong tree: trees with equally many children swap their vectors
    wrong = list(eta)
    for ts in by_n.values():
        for i, t in enumerate(ts):
            wrong[t] = eta[ts[(i + 1) % len(ts)]]
    faults = dict(wrong_tree=dict(eta=wrong), rolled=dict(eta=[np.roll(e, 1) for e in eta]),
                  late=dict(eta=eta, late=True))
    for name, kw in faults.items():
        bad = _visit_table(NR.py_search(pos, SIMS, eps=EPS, **kw))
        moved = [t for t in range(NPOS) if bad[t] != good[t]]
        print(f"{name}: visit counts changed in {len(moved)} of {NPOS} trees: {moved}")
        assert moved, name
