"""Thinning of the Connect4 search's evaluation cache (search.hip, "thinning"): past
its fill threshold the table is not emptied; the entries a lookup ever hit and the
newest stay, at the same generation, and the others are zeroed, which leaves holes
in their buckets.  What stays is a performance matter; what a search or a self-play
call returns must not depend on it, so every test compares against the same calls
with the cache off, bit for bit.  spai_eval_cache_thin drives a thinning directly.

Net: 2 blocks x 64, random init, bf16.  Tail mode is off where single trees are
searched one call at a time, so that every call is one chain of plain iterations.
"""
import os

import numpy as np
import pytest

import c4_search_ref as R

pytestmark = pytest.mark.gpu

BLOCKS, NET_SEED = 2, 7
NO_TAIL = {"SPAI_TAIL_LEAVES": "0", "SPAI_TAIL_TREE_EVALS": "0"}


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def params(spai):
    return spai.init_params(BLOCKS, 64, seed=NET_SEED)


def _engine(spai, params, trees, sims, capacity, seed=0):
    e = spai.Engine(num_searches=sims, max_trees=trees, eval_kind=spai.EVAL_NET, seed=seed)
    if capacity is not None:
        e.set_eval_cache(capacity)
    e.set_net(spai.Net(e, BLOCKS, params))   # closed with the engine
    return e


def test_streamed_self_play_is_identical(spai, params):
    """48 games through 16 slots at 32 simulations, tables of 16 and 4,096 entries: the
    threshold trips again and again, and the games and the sims / evals / games /
    positions are those with the cache off"""
    games_n, slots, sims, seed = 48, 16, 32, 11

    def play(capacity):
        e = _engine(spai, params, slots, sims, capacity, seed=seed)
        games, stats = e.self_play(games_n, window=slots)
        cs = e.eval_cache_stats()
        e.close()
        return {g["game"]: g for g in games}, stats, cs

    ref, ref_stats, _ = play(0)
    assert len(ref) == games_n
    for cap in (16, 4096):
        got, stats, cs = play(cap)
        print("capacity %d: %s" % (cap, cs))
        assert cs["capacity"] == cap and cs["lookups"] == stats["evals"]
        assert sorted(got) == sorted(ref)
        for gid, g in got.items():
            for k in ("moves", "policy", "value", "enc"):
                assert R.same_bits(g[k], ref[gid][k]), (cap, gid, k)
        for k in ("sims", "evals", "games", "positions"):
            assert stats[k] == ref_stats[k], (cap, k, stats[k], ref_stats[k])
        assert cs["thins"] > 0 and cs["evicted"] > 0
        assert cs["clears"] == cs["thins"] + 1   # the table's creation, then thinnings only
        assert cs["live"] <= cs["capacity"]
        assert cs["inserts"] <= stats["evals"] - cs["hits"]


_SEQ = {}


def _sequence(spai, params, capacity, keep):
    """Single trees from the empty board, one search call each (one chain: a
    deterministic order): tree 0 for 32 iterations, tree 1 for 8 (tree 0's first 8
    leaves again), spai_eval_cache_thin(keep), tree 2 for 8, tree 3 for 64.
    -> what the calls returned, and the cache's counters and the forwarded leaves
    (every forward launch counted) after each step.  Run once per (capacity, keep)."""
    if (capacity, keep) in _SEQ:
        return _SEQ[(capacity, keep)]
    os.environ.update(NO_TAIL)
    try:
        e = _engine(spai, params, 4, 64, capacity)
        e.trees_create(4)
        e.set_timing(True, stride=1)
        out, steps = [], []

        def snap():
            cs = e.eval_cache_stats()
            cs["forwarded"] = e.timing()["evaluate"]["items"]
            steps.append(cs)

        for t, iters in ((0, 32), (1, 8)):
            out.append(e.search(np.array([t]), iters))
            snap()
        if keep is not None:
            e.eval_cache_thin(keep)
        snap()
        for t, iters in ((2, 8), (3, 64)):
            out.append(e.search(np.array([t]), iters))
            snap()
        e.close()
    finally:
        for k in NO_TAIL:
            del os.environ[k]
    _SEQ[(capacity, keep)] = (out, steps)
    return out, steps


def _assert_same_calls(got, ref):
    for a, b in zip(got, ref):
        for x, y in zip(a, b):   # policy, child ids, visits, child counts
            assert R.same_bits(x, y)


def test_hit_entries_survive_and_never_hit_ones_go(spai, params):
    """4,096 entries.  Tree 1's 8 leaves are tree 0's first 8, so all of them hit; a
    thinning to 16 keeps those 8 entries (the hit class may take 3/4 of 16) and, of the
    never-hit ones, nothing: they were all born in one call, more than the rest of the
    budget, and a class of equal age stays or goes whole.  Tree 2, a fresh tree, then
    finds all of its 8 leaves in the table and the forward runs no leaf at all; after a
    thinning to 0 it finds none."""
    ref, ref_steps = _sequence(spai, params, 0, None)
    assert ref_steps[-1]["lookups"] == 0 and ref_steps[-1]["live"] == 0
    got, (s0, s1, thinned, s2, _) = _sequence(spai, params, 4096, 16)
    print("after tree 0: %s\nafter tree 1: %s\nthinned: %s\nafter tree 2: %s" % (s0, s1, thinned, s2))
    assert s0["live"] == s0["inserts"] > 16 and s0["dropped"] == 0
    assert s1["lookups"] - s0["lookups"] == s1["hits"] - s0["hits"] >= 8
    assert s1["forwarded"] == s0["forwarded"]
    assert thinned["thins"] == 1 and thinned["clears"] == s1["clears"] + 1
    assert 8 <= thinned["live"] <= 16
    assert thinned["evicted"] == s1["live"] - thinned["live"]
    assert 8 <= thinned["kept_hit"] <= thinned["live"]
    assert thinned["inserts"] == s1["inserts"]           # entries ever claimed
    lookups2 = s2["lookups"] - thinned["lookups"]
    assert lookups2 > 0 and s2["hits"] - thinned["hits"] == lookups2
    assert s2["forwarded"] == thinned["forwarded"]       # the forward ran 0 leaves
    _assert_same_calls(got, ref)

    got0, (_, z1, zthin, z2, _) = _sequence(spai, params, 4096, 0)
    assert zthin["live"] == 0 and zthin["evicted"] == z1["live"] and zthin["kept_hit"] == 0
    assert z2["hits"] == zthin["hits"]                   # tree 2 hit nothing
    assert z2["forwarded"] - zthin["forwarded"] == z2["lookups"] - zthin["lookups"] == lookups2
    _assert_same_calls(got0, ref)


def test_a_budget_at_the_live_count_evicts_nothing(spai, params):
    _, (_, s1, thinned, _, _) = _sequence(spai, params, 4096, 4096)
    assert thinned["live"] == s1["live"] and thinned["evicted"] == 0 and thinned["thins"] == 0


def test_holes_are_reusable(spai, params):
    """after the thinning to 16, tree 3's 64 iterations insert into the thinned buckets:
    the live count grows and no insert is dropped"""
    ref, _ = _sequence(spai, params, 0, None)
    got, (_, _, thinned, s2, s3) = _sequence(spai, params, 4096, 16)
    assert s3["inserts"] > s2["inserts"]
    assert s3["live"] - s2["live"] == s3["inserts"] - s2["inserts"] > 0
    assert s3["live"] > thinned["live"] and s3["dropped"] == 0
    _assert_same_calls(got, ref)


def _one_bucket(spai, params, capacity, calls=None):
    """tree 0 for 3 iterations; tree 1 one iteration per call, until 6 of the 8 ways
    are taken (calls None) or for `calls` calls; a thinning to 4; tree 2 for 32"""
    os.environ.update(NO_TAIL)
    try:
        e = _engine(spai, params, 3, 32, capacity)
        e.trees_create(3)
        out = [e.search(np.array([0]), 3)]
        n = 0
        while n < (40 if calls is None else calls):
            out.append(e.search(np.array([1]), 1))
            n += 1
            if calls is None and e.eval_cache_stats()["live"] >= 6:
                break
        before = e.eval_cache_stats()
        e.eval_cache_thin(4)
        thinned = e.eval_cache_stats()
        out.append(e.search(np.array([2]), 32))
        after = e.eval_cache_stats()
        e.close()
    finally:
        for k in NO_TAIL:
            del os.environ[k]
    return out, n, before, thinned, after


def test_holes_in_the_one_bucket_table(spai, params):
    """capacity 8, every position in the one bucket (where positions that share the
    mover's stones also share an entry's claim word, so fewer are inserted than
    evaluated).  Tree 1 grows by one iteration per call, so its entries are of as many
    ages, until 6 ways are taken: below the threshold, the table was never thinned.  A
    thinning to 4 then leaves holes between the survivors; tree 2's search after it
    equals cache-off and inserts again."""
    got, calls, before, thinned, after = _one_bucket(spai, params, 8)
    ref, _, _, _, _ = _one_bucket(spai, params, 0, calls)
    print("%d calls\nbefore: %s\nthinned: %s\nafter: %s" % (calls, before, thinned, after))
    assert before["capacity"] == 8 and 6 <= before["live"] <= 7
    assert before["hits"] > 0 and before["thins"] == 0 and before["clears"] == 1
    assert thinned["thins"] == 1 and 0 < thinned["live"] <= 4
    assert thinned["evicted"] == before["live"] - thinned["live"]
    assert thinned["kept_hit"] <= 3                      # the hit class's share of 4
    assert after["inserts"] > thinned["inserts"] and after["live"] > thinned["live"]
    assert after["live"] <= 8 and after["thins"] == 1
    assert len(got) == len(ref)
    _assert_same_calls(got, ref)


def test_set_net_after_a_thinning_empties_the_table(spai, params):
    """a thinning keeps the generation, and with it the weights' validity is still the
    generation's business: set_net after it empties the table, and the next games are
    those of a fresh engine with the new weights"""
    games_n, sims, seed = 16, 32, 11
    params_b = spai.init_params(BLOCKS, 64, seed=NET_SEED + 1)
    e = _engine(spai, params, games_n, sims, 4096, seed=seed)
    a = {g["game"]: g for g in e.self_play(games_n)[0]}
    c0 = e.eval_cache_stats()
    e.eval_cache_thin(int(c0["live"]) // 2)
    c1 = e.eval_cache_stats()
    assert c1["thins"] == c0["thins"] + 1 and 0 < c1["live"] <= c0["live"] // 2
    e.set_net(spai.Net(e, BLOCKS, params_b))
    c2 = e.eval_cache_stats()
    assert c2["live"] == 0 and c2["clears"] == c1["clears"] + 1 and c2["thins"] == c1["thins"]
    b = {g["game"]: g for g in e.self_play(games_n)[0]}
    e.close()
    f = _engine(spai, params_b, games_n, sims, 4096, seed=seed)
    fresh = {g["game"]: g for g in f.self_play(games_n)[0]}
    f.close()
    assert sorted(b) == sorted(fresh)
    for gid, g in b.items():
        for k in ("moves", "policy", "value", "enc"):
            assert R.same_bits(g[k], fresh[gid][k]), (gid, k)
    assert any(len(a[g]["moves"]) != len(b[g]["moves"]) or not np.array_equal(a[g]["moves"], b[g]["moves"])
               or not np.array_equal(a[g]["policy"], b[g]["policy"]) for g in a), "net B played net A's games"
