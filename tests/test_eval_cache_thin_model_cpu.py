"""The CPU model of the evaluation cache's thinning (scripts/eval_cache_hitrate.py,
ThinTable; the device: search.hip, "thinning"): past the fill threshold the table
keeps the entries that were hit, up to their share of the budget, and the newest
never-hit ones, in whole ages.  Synthetic key streams: a move is one batch.

Table: 256 entries (32 buckets x 8 ways, two candidate buckets), thinned past 7/8
(224 entries) to 1/2 (128), of which the hit class may take 3/4 (96)."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "scripts"))

CAPACITY, THRESHOLD, BUDGET, HIT_CAP = 256, 224, 128, 96


@pytest.fixture(scope="module")
def model():
    import eval_cache_hitrate
    return eval_cache_hitrate


def keys(tag, n):
    return [b"%s-%d" % (tag, i) for i in range(n)]


def move(t, ks):
    t.batch(ks)
    t.end_move()


def test_cutoff_whole_ages_and_the_guard(model):
    t = model.ThinTable(CAPACITY)
    hist = [[0] * t.AGES, [0] * t.AGES]
    hist[1][1], hist[1][2], hist[1][3] = 50, 50, 50
    hist[0][0], hist[0][1], hist[0][2], hist[0][3] = 50, 10, 10, 10
    # hit: 50, then 100 > 96; never hit: 128 - 50 = 78 takes 50 + 10 + 10, then 80 > 78
    assert t.cutoff(hist, BUDGET) == ([3, 2], [70, 50])
    # no more than the budget in the table: everything stays, whatever the classes
    assert t.cutoff(hist, 230) == ([t.AGES, t.AGES], [80, 150])
    # an age that alone exceeds its budget goes whole, and the older ones with it; the
    # never-hit class then has the whole budget
    hist[1][0] = 97
    assert t.cutoff(hist, BUDGET) == ([t.AGES, 0], [80, 0])
    assert t.cutoff(hist, 0) == ([0, 0], [0, 0])
    unguarded = model.ThinTable(CAPACITY, hit_share=(1, 1))
    hist[1][0] = 0
    assert unguarded.cutoff(hist, BUDGET) == ([0, 3], [0, 100])


def test_hit_keys_survive_and_old_once_seen_keys_go(model):
    t = model.ThinTable(CAPACITY)
    hot, cold1, cold2, cold3 = keys(b"hot", 40), keys(b"a", 60), keys(b"b", 60), keys(b"c", 70)
    move(t, hot + cold1)
    move(t, hot + cold2)            # the hot keys are looked up again: 40 hits
    assert t.hits == 40 and t.thins == 0
    t.batch(cold3)
    before = set(t.entries)
    assert len(before) > THRESHOLD and len(before) + t.dropped == 230
    t.end_move()                    # hit: 40 (of 96); never hit: 128 - 40 = 88 takes this move's 70, not 70 + 60
    assert t.thins == 1 and t.clears == 1 and t.kept_hit == len(before & set(hot))
    assert set(t.entries) == before & set(hot + cold3)
    assert len(t) <= BUDGET and t.evicted == len(before) - len(t)
    assert sum(t.count) == len(t)
    move(t, hot + cold1)            # and they are served on; the evicted ones are inserted again
    assert t.hits == 40 + len(before & set(hot))
    assert set(cold1) & set(t.entries)


def test_the_guard_keeps_fresh_keys_when_hit_keys_exceed_the_budget(model):
    def run(**kw):
        t = model.ThinTable(CAPACITY, **kw)
        old = keys(b"old", 150)
        move(t, old)
        fresh = []
        for m in range(3):          # 50 of the old keys hit per move, and 12 new ones come in
            fresh.append(keys(b"f%d" % m, 12))
            move(t, old[50 * m:50 * m + 50] + fresh[-1])
        newest = keys(b"new", 50)
        t.batch(newest)
        before = set(t.entries)
        assert len(before) > THRESHOLD
        t.end_move()
        assert t.thins == 1 and len(t) <= BUDGET
        return t, before, old, fresh, newest

    # shipped: the hit class is 150 > 96, so only its youngest age (50) stays; the never-hit
    # class gets 78: this move's 50 and two of the three older twelves (at this load a few
    # keys found both their buckets full and never got in: `before` is what did)
    t, before, old, fresh, newest = run()
    assert set(t.entries) == before & set(old[100:] + newest + fresh[2] + fresh[1])
    assert t.kept_hit == len(before & set(old[100:])) <= HIT_CAP
    assert set(newest) & before <= set(t.entries)
    # unguarded, the hit class takes two ages (100 of 128) and no fresh key survives
    u, before, old, fresh, newest = run(hit_share=(1, 1))
    assert set(u.entries) == before & set(old[50:])


def test_live_count_never_exceeds_the_budget(model):
    rng = np.random.default_rng(0)
    t = model.ThinTable(CAPACITY)
    thins = 0
    for m in range(200):
        ks = [b"k%d" % k for k in rng.integers(0, 2000, 30)] + [b"k%d" % k for k in rng.integers(0, 20, 10)]
        move(t, ks)
        assert len(t) <= CAPACITY and sum(t.count) == len(t) and max(t.count) <= 8
        if t.thins > thins:
            thins = t.thins
            assert len(t) <= BUDGET and t.kept_hit <= HIT_CAP
    assert thins > 5 and t.clears == thins and t.hits > 0
    assert t.inserts - t.evicted == len(t)


def test_budget_at_the_capacity_evicts_nothing(model):
    """keep = 1/1: the threshold trips and nothing goes, so the table is the insert-only
    BucketTable that is never emptied (fill 1/1), counter for counter"""
    rng = np.random.default_rng(1)
    t = model.ThinTable(CAPACITY, keep=(1, 1))
    b = model.BucketTable(CAPACITY, 8, 2, (1, 1))
    for m in range(40):
        ks = [b"k%d" % k for k in rng.integers(0, 400, 40)]
        move(t, ks)
        move(b, ks)
    assert len(t) > THRESHOLD and t.evicted == 0 and t.thins == 0
    assert (t.lookups, t.hits, t.clears) == (b.lookups, b.hits, b.clears) == (1600, b.hits, 0)
    assert (t.inserts, t.dropped) == (b.inserts, b.dropped) and set(t.entries) == b.keys
