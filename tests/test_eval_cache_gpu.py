"""The Connect4 search's evaluation cache (search.hip): a device table from the
full leaf position to the net's priors and value.  A hit hands the search the
very bytes a forward wrote for that position, so nothing a search or a
self-play call returns may depend on the cache being on, on its size, or on
what it holds: every test here compares against the same run with capacity 0,
bit for bit.

Shapes: a 2-block x 64 net; 128 tree slots, the fewest that run as two search
chains (64 trees each); 32 iterations per move.  With so few iterations every
call after a game's first would run in tail mode (one chain), so each schedule
is played both under the default tail policy and with tail mode off
(SPAI_TAIL_*=0, read per search call), which keeps the two concurrent chains.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCKS, SIMS, SLOTS, SEED = 2, 32, 128, 11
NO_TAIL = {"SPAI_TAIL_LEAVES": "0", "SPAI_TAIL_TREE_EVALS": "0"}
# schedule -> (games, window)
SCHEDULES = {"lockstep": (SLOTS, None), "streamed": (2 * SLOTS, SLOTS)}
STAT_KEYS = ("sims", "evals", "games", "positions")


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def _engine(spai, capacity, net_seed=1, sims=SIMS, slots=SLOTS):
    e = spai.Engine(num_searches=sims, max_trees=slots, eval_kind=spai.EVAL_NET, seed=SEED)
    if capacity is not None:
        e.set_eval_cache(capacity)
    e.set_net(spai.Net(e, BLOCKS, spai.init_params(BLOCKS, 64, seed=net_seed)))
    return e


def _play(spai, capacity, schedule, env=None, net_seed=1, timing=False):
    """one self-play call on a fresh engine -> (games by id, stats, cache stats, timing)"""
    games_n, window = SCHEDULES[schedule]
    env = env or {}
    os.environ.update(env)
    try:
        e = _engine(spai, capacity, net_seed)
        if timing:
            e.set_timing(True, stride=1)   # every forward launch of every chain
        games, stats = e.self_play(games_n, window=window)
        cs = e.eval_cache_stats()
        tm = e.timing() if timing else None
        e.close()
    finally:
        for k in env:
            del os.environ[k]
    return {g["game"]: g for g in games}, stats, cs, tm


_REF = {}


def _reference(spai, schedule):
    """the schedule's games with the cache off, played once for all the tests"""
    if schedule not in _REF:
        games, stats, cs, _ = _play(spai, 0, schedule)
        assert cs["capacity"] == 0 and cs["lookups"] == 0 and cs["hits"] == 0 and cs["inserts"] == 0
        _REF[schedule] = (games, stats)
    return _REF[schedule]


def _assert_same_games(got, ref):
    assert sorted(got) == sorted(ref)
    for gid, g in got.items():
        r = ref[gid]
        for k in ("moves", "policy", "value", "enc"):
            np.testing.assert_array_equal(g[k], r[k], err_msg="game %d, %s" % (gid, k))


@pytest.mark.parametrize("tail", ["tail-default", "tail-off"])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_self_play_cache_on_equals_off(spai, schedule, tail):
    """default capacity against capacity 0: the same games bit for bit, the same
    sims / evals / games / positions; the cache did serve leaves; and, with tail mode
    off and every forward launch timed, the leaves those launches ran (the per-launch
    counters the device keeps) plus the hits are exactly the evals (which come from
    the per-tree leaf counts): hits + forwarded == evals, and the timing items are
    the forwarded leaves, not the served ones."""
    ref_games, ref_stats = _reference(spai, schedule)
    no_tail = tail == "tail-off"
    games, stats, cs, tm = _play(spai, None, schedule, env=NO_TAIL if no_tail else None, timing=no_tail)
    _assert_same_games(games, ref_games)
    for k in STAT_KEYS:
        assert stats[k] == ref_stats[k], (k, stats[k], ref_stats[k])
    assert cs["capacity"] == 16384 * SLOTS   # the default: 16384 entries per tree slot
    assert cs["lookups"] == stats["evals"]
    forwarded = stats["evals"] - cs["hits"]
    print("evals %.0f hits %.0f (%.3f) inserts %.0f dropped %.0f clears %.0f" %
          (stats["evals"], cs["hits"], cs["hits"] / stats["evals"], cs["inserts"], cs["dropped"], cs["clears"]))
    assert cs["hits"] > 0 and forwarded > 0
    # every insert is a forwarded leaf's; duplicates inside a batch insert once
    assert 0 < cs["inserts"] <= forwarded
    if tm is not None:
        items = tm["evaluate"]["items"]
        print("forward launches %.0f ran %.0f leaves; evals - hits = %.0f" %
              (tm["evaluate"]["launches"], items, forwarded))
        assert tm["evaluate"]["launches"] > 0
        assert items == stats["evals"] - cs["hits"]


def _search_twice(spai, capacity, n=8, sims=64):
    """two search calls over n trees from the empty board, the roots moved on in between"""
    e = _engine(spai, capacity, sims=sims, slots=n)
    e.trees_create(n)
    out = []
    pol, ids, vis, nc = e.search(np.arange(n))
    out.append((pol, ids, vis, nc))
    for t in range(n):
        e.use_subtree(t, ids[t, t % int(nc[t])])
    out.append(e.search(np.arange(n)))
    cs = e.eval_cache_stats()
    e.close()
    return out, cs


def test_search_cache_on_equals_off(spai):
    """spai_search over a few trees: root policies, child ids, visit counts and child
    counts are those of the cache-off search, and trees that share positions hit"""
    on, cs = _search_twice(spai, None)
    off, cs_off = _search_twice(spai, 0)
    assert cs_off["hits"] == 0 and cs["hits"] > 0
    for a, b in zip(on, off):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def _search_two_trees(spai, capacity):
    """tree 0 searched for 6 iterations, then tree 1 for 32, both from the empty board"""
    e = _engine(spai, capacity, slots=2)
    e.trees_create(2)
    out = [e.search(np.array([0]), 6), e.search(np.array([1]), 32)]
    cs = e.eval_cache_stats()
    e.close()
    return out, cs


def test_one_bucket_full_key_compare(spai):
    """the smallest table, one bucket of 8 entries: every position maps to it, so a
    hit can only come from the full key compare, and most inserts are dropped.
    Self-play through it equals cache-off.  That it serves leaves at all is shown
    where it must, whatever the timing of the chains: tree 0's 6 iterations leave at
    most 6 entries (no clear: not above 3/4 of 8), the empty board among them, and
    tree 1 then starts with the same leaves, so at least its first one hits."""
    ref_games, ref_stats = _reference(spai, "lockstep")
    games, stats, cs, _ = _play(spai, 1, "lockstep", env=NO_TAIL)
    assert cs["capacity"] == 8
    _assert_same_games(games, ref_games)
    for k in STAT_KEYS:
        assert stats[k] == ref_stats[k], (k, stats[k], ref_stats[k])
    assert cs["dropped"] > 0
    print("self-play through one bucket: hits %.0f inserts %.0f dropped %.0f clears %.0f" %
          (cs["hits"], cs["inserts"], cs["dropped"], cs["clears"]))
    on, cs2 = _search_two_trees(spai, 1)
    off, _ = _search_two_trees(spai, 0)
    print("two trees through one bucket: hits %.0f inserts %.0f dropped %.0f" % (cs2["hits"], cs2["inserts"], cs2["dropped"]))
    assert cs2["capacity"] == 8 and cs2["hits"] > 0 and cs2["dropped"] > 0
    for a, b in zip(on, off):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_weight_change_clears(spai):
    """set_net with other weights: the next games are those of a fresh engine with
    the new weights, not the first net's, and the table was emptied"""
    games_n = SLOTS
    e = _engine(spai, None, net_seed=1)
    a = {g["game"]: g for g in e.self_play(games_n)[0]}
    c0 = e.eval_cache_stats()
    assert c0["inserts"] > 0
    e.set_net(spai.Net(e, BLOCKS, spai.init_params(BLOCKS, 64, seed=2)))
    b = {g["game"]: g for g in e.self_play(games_n)[0]}
    c1 = e.eval_cache_stats()
    e.close()
    assert c1["clears"] > c0["clears"]
    fresh, _, _, _ = _play(spai, None, "lockstep", net_seed=2)
    _assert_same_games(b, fresh)
    assert any(len(a[g]["moves"]) != len(b[g]["moves"]) or not np.array_equal(a[g]["moves"], b[g]["moves"])
               or not np.array_equal(a[g]["policy"], b[g]["policy"]) for g in a), "net B played net A's games"


def test_refill_during_stream(spai):
    """a table of 4096 entries against some thousand new positions per move: the fill
    threshold trips between the search calls of the streamed run (one clear is the
    table's creation), and the games do not change"""
    ref_games, ref_stats = _reference(spai, "streamed")
    games, stats, cs, _ = _play(spai, 4096, "streamed", env=NO_TAIL)
    assert cs["capacity"] == 4096
    print("clears %.0f inserts %.0f dropped %.0f hits %.0f" % (cs["clears"], cs["inserts"], cs["dropped"], cs["hits"]))
    assert cs["clears"] - 1 > 0
    assert cs["inserts"] > cs["capacity"]   # more than one table's worth went in
    _assert_same_games(games, ref_games)
    for k in STAT_KEYS:
        assert stats[k] == ref_stats[k], (k, stats[k], ref_stats[k])
