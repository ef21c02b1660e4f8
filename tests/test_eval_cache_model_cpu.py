"""The CPU model of the evaluation cache's table (scripts/eval_cache_hitrate.py):
buckets of 8 ways, one candidate bucket per key or the emptier of two.  Its
balls-in-bins losses are what the device's two candidate buckets and the bound of
tests/test_eval_cache_two_choice_gpu.py rest on, and with unlimited ways it must
be the fully associative table it replaces."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "scripts"))


@pytest.fixture(scope="module")
def model():
    import eval_cache_hitrate
    return eval_cache_hitrate


def test_candidate_buckets(model):
    """high and low half of the hash; equal halves: first ^ 1; one bucket: one candidate"""
    assert model.candidate_buckets((5 << 32) | 9, 16, 2) == (5, 9)
    assert model.candidate_buckets((5 << 32) | 9, 16, 1) == (5,)
    assert model.candidate_buckets((5 << 32) | 5, 16, 2) == (5, 4)
    assert model.candidate_buckets((4 << 32) | 4, 16, 2) == (4, 5)
    assert model.candidate_buckets((21 << 32) | 5, 16, 2) == (5, 4)   # equal after the mask
    assert model.candidate_buckets((1 << 32) | 0, 2, 2) == (1, 0)
    assert model.candidate_buckets((1 << 32) | 1, 2, 2) == (1, 0)
    assert model.candidate_buckets((7 << 32) | 3, 1, 2) == (0,)


@pytest.mark.parametrize("seed", [0, 1])
def test_loss_at_three_quarters(model, seed):
    """random keys into 2^14 buckets x 8 ways up to 3/4 fill: one bucket per key loses
    5-9 % of them, the emptier of two fewer than 0.1 %"""
    one = model.bucket_loss(1 << 14, 8, 1, 0.75, seed)
    two = model.bucket_loss(1 << 14, 8, 2, 0.75, seed)
    print("loss at 3/4: one bucket %.4f, two buckets %.6f" % (one, two))
    assert 0.05 <= one <= 0.09
    assert two < 0.001


def _stream(seed, batches, per_batch, universe):
    rng = np.random.default_rng(seed)
    return [[int(k).to_bytes(8, "little") for k in rng.integers(0, universe, per_batch)] for _ in range(batches)]


@pytest.mark.parametrize("delay", [0, 1])
def test_unlimited_ways_is_the_fully_associative_table(model, delay):
    """a fixed key stream (repeats inside and across batches, a move every 8 batches,
    capacity reached and cleared several times): the same lookups, hits and clears
    after every batch"""
    old, new = model.Table(512, delay), model.BucketTable(512, None, 2, (3, 4), delay)
    for i, keys in enumerate(_stream(3, 200, 40, 3000)):
        if i and i % 8 == 0:
            old.end_move()
            new.end_move()
        old.batch(keys)
        new.batch(keys)
        assert (old.lookups, old.hits, old.clears) == (new.lookups, new.hits, new.clears), i
    assert old.clears > 2 and 0 < old.hits < old.lookups


def test_bucket_table_drops_and_clears(model):
    """8 ways: the table never holds more than its entries or a bucket more than its
    ways, drops are counted, two candidates drop fewer than one on the same stream, and
    the 7/8 threshold clears later than 3/4"""
    tabs = {(ch, f): model.BucketTable(1024, 8, ch, f) for ch, f in ((1, (3, 4)), (2, (3, 4)), (2, (7, 8)))}
    for i, keys in enumerate(_stream(5, 150, 40, 1 << 40)):
        for t in tabs.values():
            if i and i % 4 == 0:
                t.end_move()
            t.batch(keys)
            assert max(t.count) <= 8 and sum(t.count) == len(t.keys) <= t.capacity == 1024
    one, two, late = tabs[1, (3, 4)], tabs[2, (3, 4)], tabs[2, (7, 8)]
    assert one.buckets == 128 and one.dropped > two.dropped
    assert one.inserts + one.dropped == two.inserts + two.dropped   # every new key is offered once
    assert 0 < late.clears < two.clears
