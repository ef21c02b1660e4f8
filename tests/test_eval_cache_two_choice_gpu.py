"""The evaluation cache's two candidate buckets per position (search.hip,
cache_buckets): a lookup reads both, an insert goes to the emptier one.  Which
bucket holds a position, how many buckets there are and whether the table is on
at all must not show in anything a search or a self-play call returns, and at a
load at which one bucket per position drops several per cent of its inserts, two
must drop next to none.

Net: 2 blocks x 64, random init, bf16.  Table sizes: 0 (off), 8 entries (one
bucket: a single candidate), 16 (two buckets: the second candidate is always
first ^ 1), 4,096 (512 buckets) and the default.
"""
import numpy as np
import pytest

import c4_search_ref as R

pytestmark = pytest.mark.gpu

BLOCKS, NET_SEED = 2, 7
TREES, SIMS = 96, 64
CAPACITIES = [0, 8, 16, 4096, None]


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


def _search(spai, params, roots, sims, capacity):
    """one search call over trees rooted at `roots` on a fresh engine -> (what the call
    returned and left in the root's child records, its live leaves, the cache's counters)"""
    n = len(roots)
    e = _engine(spai, params, n, sims, capacity)
    e.trees_create(n)
    for t, s in enumerate(roots):
        e.tree_reset(t, R.key_of(s) + (0,))
    e.set_timing(True, stride=1)   # counts the leaves of every forward launch
    pol, _, vis, nc = e.search(np.arange(n, dtype=np.uint32), sims)
    cs = e.eval_cache_stats()
    forwarded = e.timing()["evaluate"]["items"]
    kids = [e.tree_child_stats(t)[1:] for t in range(n)]   # N, W, P
    roots_nw = [e.tree_node(t, 0)[1:] for t in range(n)]
    e.close()
    out = dict(policy=pol, visits=vis, nc=nc,
               child_n=np.concatenate([k[0] for k in kids]), child_w=np.concatenate([k[1] for k in kids]),
               child_p=np.concatenate([k[2] for k in kids]),
               root_n=np.array([r[0] for r in roots_nw], np.uint32), root_w=np.array([r[1] for r in roots_nw], np.float32))
    return out, forwarded + cs["hits"], cs


def test_search_is_bit_identical_across_capacities(spai, params):
    """96 trees (a third of the roots duplicates, so trees share leaves from the first
    iteration on) x 64 simulations at every table size: the root children's N, W and P,
    the visit policies and the number of live leaves are those of the search with the
    cache off, bit for bit"""
    roots = R.positions(TREES, TREES, duplicates=TREES // 3)
    ref, ref_evals, ref_cs = _search(spai, params, roots, SIMS, 0)
    assert ref_cs["capacity"] == 0 and ref_cs["lookups"] == 0 and ref_cs["hits"] == 0
    assert 0 < ref_evals < TREES * SIMS   # terminal leaves occurred
    for cap in CAPACITIES[1:]:
        got, evals, cs = _search(spai, params, roots, SIMS, cap)
        print("capacity %s: %d entries, lookups %d hits %d inserts %d dropped %d" %
              (cap, cs["capacity"], cs["lookups"], cs["hits"], cs["inserts"], cs["dropped"]))
        if cap is None:
            assert cs["capacity"] > 4096
        else:
            assert cs["capacity"] == cap
        for k in ref:
            assert R.same_bits(got[k], ref[k]), (cap, k)
        assert evals == ref_evals == cs["lookups"], (cap, evals, ref_evals, cs["lookups"])
        assert cs["inserts"] > 0
        if cap is None or cap >= 4096:
            assert cs["hits"] > 0   # the duplicated roots at the least
        if cap is not None and cap <= 16:
            assert cs["dropped"] > 0 and cs["inserts"] <= cap


def test_self_play_stream_is_identical(spai, params):
    """48 games through 16 slots at 32 simulations: the games with a table of 16 entries
    and of 4,096 are those with the cache off, game by game"""
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
        print("capacity %d: hits %.0f inserts %.0f dropped %.0f clears %.0f" %
              (cap, cs["hits"], cs["inserts"], cs["dropped"], cs["clears"]))
        assert cs["capacity"] == cap and cs["lookups"] == stats["evals"] and cs["inserts"] > 0
        assert sorted(got) == sorted(ref)
        for gid, g in got.items():
            for k in ("moves", "policy", "value", "enc"):
                assert R.same_bits(g[k], ref[gid][k]), (cap, gid, k)
        for k in ("sims", "evals", "games", "positions"):
            assert stats[k] == ref_stats[k], (cap, k, stats[k], ref_stats[k])


def test_retention_at_two_thirds_fill(spai, params):
    """A table of 4,096 entries (512 buckets) filled to between 60 % and 74 % by one
    search call, below the fill at which it is emptied: at most 1 % of the insert
    attempts may be dropped.

    The cap is not a measurement.  Random keys thrown at buckets of 8 ways up to 2/3
    fill: 4 % of them find their bucket full when each key has one (2.5 % in a single
    draw at only 512 buckets), and fewer than 0.1 % (none, at 512 buckets) when a key
    goes to the emptier of two (scripts/eval_cache_hitrate.py, bucket_loss;
    tests/test_eval_cache_model_cpu.py), so 1 % separates the schemes with room on both
    sides.

    Inputs: 96 distinct roots (c4_search_ref.positions(96, 96)) x 36 simulations.  With
    the CPU oracle's search behind the fp32 net of the same parameters these give 2,835
    evaluations of 2,802 distinct positions, 68.4 % of the table; the device's bf16 net
    visits a slightly different set, so the fill reached is asserted, not assumed."""
    trees, sims, capacity = 96, 36, 4096
    roots = R.positions(trees, trees)
    assert len({R.key_of(s) for s in roots}) == trees
    _, evals, cs = _search(spai, params, roots, sims, capacity)
    attempts = cs["inserts"] + cs["dropped"]
    fill = cs["inserts"] / capacity
    print("evals %d hits %d inserts %d dropped %d (%.3f %% of %d attempts), fill %.3f, clears %d" %
          (evals, cs["hits"], cs["inserts"], cs["dropped"], 100.0 * cs["dropped"] / max(1, attempts), attempts, fill,
           cs["clears"]))
    assert cs["capacity"] == capacity
    assert cs["clears"] == 1   # the table's creation: it was not emptied on the way
    assert 0.60 <= fill <= 0.74, fill
    assert cs["dropped"] <= 0.01 * attempts, (cs["dropped"], attempts)
