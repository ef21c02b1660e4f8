"""The Connect4 net-search yardstick (tests/c4_search_ref.py) on the CPU, with the
oracle's own fp32 Model::predict (or_predict) as the forward behind the callback.

The harness is pinned: through the callback, the memo and the byte write-back the
oracle gives the visit counts, policies and self-play stream of
tests/golden/mcts_f32net.npz, which its built-in EVAL_NET path wrote
(gen_f32net_golden.py).  The searches are per tree, so every third root of the
fixture is searched (16 of 48 at the fixture's 64 simulations; or_predict takes
6 ms per position of the 2 x 64 net); the self-play stream is compared whole.

The yardstick reacts to what it exists for.  Shapes: the smallest deep search of
tests/test_c4_search_net_gpu.py, 100 roots of positions(100, 1, duplicates=10) at
its fewest simulations, 24 (the fewer the simulations, the fewer trees a fault
moves).  The forward is a 1-block x 16-channel net (0.4 ms per position) from the
shared init stream.  Every gross fault must move the root visit counts of at
least a quarter of the trees, and the root children's P or W bits of at least as
many; NO_RENORM acts only where a column is full, so its quarter is taken of the
trees whose root has one.  Noise of one float32 ulp on the priors must show in
the root children's P bits of every tree whose root entry it changed; how many
visit counts it moves is printed, not bounded: that figure is why the GPU test
compares P and W and not the visit counts alone."""
import os

import numpy as np
import pytest

import c4_search_ref as R
from conftest import GOLDEN

N, DUPLICATES, SIMS = 100, 10, 24


@pytest.fixture(scope="module")
def golden(oracle):
    z = np.load(os.path.join(GOLDEN, "mcts_f32net.npz"))
    blocks, seed = int(z["blocks"]), int(z["seed"])
    net = oracle.Net(oracle.GAME_CONNECT4, blocks, 64, oracle.init_params(oracle.GAME_CONNECT4, blocks, 64, seed))
    return z, R.Evaluator(R.oracle_predict(net))


def test_callback_search_equals_fixture(golden):
    z, ev = golden
    pick = np.arange(0, len(z["roots"]), 3)
    roots = [R.state_from_key(int(x), int(o), int(m)) for x, o, m in z["roots"][pick]]
    rs = R.RefSearch(roots, ev)
    r = rs.search(int(z["sims"]))
    assert R.same_bits(r["visits"], z["visits"][pick])
    assert R.same_bits(r["policy"], z["policy"][pick])
    assert R.same_bits(r["nc"], z["n_children"][pick])
    # the records agree with what the search call returns, and with the memo
    for t in range(rs.n):
        acts, vis, w, pri = rs.children(t)
        k = int(r["nc"][t])
        assert list(acts) == roots[t].valid_actions() and len(acts) == k
        assert R.same_bits(vis.astype(np.float32), r["visits"][t, :k])
        n_root, w_root = rs.root(t)
        assert n_root == int(z["sims"]) and vis.sum() == n_root - 1
        p, v = ev.entry(R.key_of(roots[t]))
        assert R.same_bits(pri, p[acts])
    assert ev.leaves == r["evals"] and ev.calls == int(z["sims"]) and ev.forwards <= ev.calls
    assert len(ev.index) < ev.leaves   # trees share positions: the memo served some
    rs.close()


def test_callback_self_play_equals_fixture(golden, oracle):
    z, ev = golden
    sp = oracle.self_play(oracle.GAME_CONNECT4, int(z["sp_games"]), int(z["sp_sims"]), int(z["sp_seed"]),
                          eval_kind=oracle.EVAL_NET, eval_fn=ev, max_plies=42)
    ev.check()
    for k in ("enc", "policy", "value", "game"):
        assert R.same_bits(sp[k], z["sp_" + k]), k
    assert R.same_bits(sp["moves"], z["sp_moves"]) and R.same_bits(sp["n_moves"], z["sp_n_moves"])


def test_state_keys_round_trip(oracle):
    pos = R.positions(40, 3)
    arr = (oracle.C.c_void_p * len(pos))(*[oracle.C.addressof(s.st) for s in pos])
    keys = R.state_keys(arr, len(pos))
    assert keys == [R.key_of(s) for s in pos]
    for s, (x, o, n) in zip(pos, keys):
        back = R.state_from_key(x, o, n)
        assert bytes(back.st) == bytes(s.st)
        assert R.legal_columns(x, o) == s.valid_actions()


@pytest.mark.parametrize("n,dup", [(100, 10), (100, 0), (160, 0), (700, 70)])
def test_positions_deliver(oracle, n, dup):
    pos = R.positions(n, 1, duplicates=dup)
    keys = [R.key_of(s) for s in pos]
    assert len(pos) == n and all(s.status == oracle.ONGOING for s in pos)
    assert len(set(keys)) == n - dup
    assert {s.n % 2 for s in pos} == {0, 1}
    assert (0, 0, 0) in keys and max(s.n for s in pos) <= 20
    full = sum(R.has_full_column(s) for s in pos)
    win = sum(R.wins_in_one(s) for s in pos)
    # a terminal within two plies: the side to move can win at once, or can move so that the other side can
    two = sum(R.wins_in_one(s) or any(R.wins_in_one(s.next_state(a)) for a in s.valid_actions()
                                      if s.next_state(a).status == oracle.ONGOING) for s in pos)
    print(f"positions({n}, 1, {dup}): {full} with a full column, {win} one move from a win, "
          f"{two} with a terminal within two plies")
    q = max(1, (n - dup) // 8)
    assert full >= q and win >= q and two >= win
    if dup:   # the copies do not all stand next to their originals
        first = {}
        gaps = [i - first.setdefault(k, i) for i, k in enumerate(keys)]
        assert max(gaps) > 1
    assert [R.key_of(s) for s in R.positions(n, 1, duplicates=dup)] == keys   # reproducible
    assert [R.key_of(s) for s in R.positions(n, 2, duplicates=dup)] != keys


@pytest.fixture(scope="module")
def deep(oracle):
    """the base run and a runner for the faulty ones"""
    net = oracle.Net(oracle.GAME_CONNECT4, 1, 16, oracle.init_params(oracle.GAME_CONNECT4, 1, 16, 5))
    predict = R.oracle_predict(net)
    roots = R.positions(N, 1, duplicates=DUPLICATES)

    def run(pred):
        ev = R.Evaluator(pred)
        rs = R.RefSearch(roots, ev)
        try:
            r = rs.search(SIMS)
            return r, rs.records(), ev
        finally:
            rs.close()

    base = run(predict)
    return dict(roots=roots, predict=predict, run=run, base=base)


def _moved(a, b):
    """trees whose visit counts differ, trees whose children's P or W bits differ"""
    (ra, reca, _), (rb, recb, _) = a, b
    vis = [t for t in range(len(reca)) if not R.same_bits(ra["visits"][t], rb["visits"][t])]
    rec = [t for t in range(len(reca)) if not (R.same_bits(reca[t][2], recb[t][2]) and R.same_bits(reca[t][3], recb[t][3]))]
    return vis, rec


def test_deep_search_is_reproducible(deep):
    again = deep["run"](deep["predict"])
    assert _moved(again, deep["base"]) == ([], [])
    r, rec, ev = deep["base"]
    assert all(int(v.sum()) == SIMS - 1 for _, v, _, _ in rec)
    assert r["evals"] < N * SIMS          # terminal leaves occurred
    assert len(ev.index) < ev.leaves      # shared leaves


@pytest.mark.parametrize("kind", R.Fault.GROSS)
def test_gross_fault_moves_visits_and_records(deep, kind):
    fault = R.Fault(deep["predict"], kind)
    got = deep["run"](fault)
    vis, rec = _moved(got, deep["base"])
    among = list(range(N))
    if kind == R.Fault.NO_RENORM:
        among = [t for t, s in enumerate(deep["roots"]) if R.has_full_column(s)]
    vis_in, rec_in = [t for t in vis if t in among], [t for t in rec if t in among]
    print(f"{kind}: visit counts moved in {len(vis)} of {N} trees ({len(vis) / N:.0%}), P or W bits in {len(rec)} "
          f"({len(rec) / N:.0%}); among the {len(among)} trees it is measured on: {len(vis_in)} and {len(rec_in)}")
    assert 4 * len(vis_in) >= len(among), (kind, len(vis_in), len(among))
    assert len(rec_in) >= len(vis_in), (kind, len(rec_in), len(vis_in))


@pytest.mark.parametrize("seed", [1, 2])
def test_ulp_noise_shows_in_the_records(deep, seed):
    fault = R.Fault(deep["predict"], R.Fault.ULP_NOISE, seed=seed, amp=1)
    got = deep["run"](fault)
    vis, rec = _moved(got, deep["base"])
    noised = [t for t, s in enumerate(deep["roots"]) if R.key_of(s) in fault.changed]
    p_moved = [t for t in range(N) if not R.same_bits(got[1][t][3], deep["base"][1][t][3])]
    print(f"one ulp of noise (seed {seed}): root entry changed in {len(noised)} of {N} trees, root-child P bits in "
          f"{len(p_moved)}, P or W bits in {len(rec)}, visit counts in {len(vis)}")
    assert len(noised) >= N // 2
    assert set(noised) <= set(p_moved), sorted(set(noised) - set(p_moved))
