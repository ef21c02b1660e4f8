#!/usr/bin/env python3
"""Hit rate an evaluation cache would see in Connect4 self-play, measured on the
CPU with the oracle (no GPU): oracle.self_play with the libtorch fp32 net
(refcpu.TorchEval), games played to completion; every leaf batch (one search
iteration over the games in play) is looked up before that batch's own results
are inserted, as the device does it (search.hip, evaluation cache).

Prints the overall hit rate of an unbounded table, the rate per move, and the
rate of bounded insert-only tables that are emptied between moves once fuller
than a threshold: fully associative (Table), and with the device's structure
(BucketTable: buckets of 8 ways, an insert into a full bucket dropped, one
candidate bucket per position or the emptier of two, cleared at 3/4 or 7/8).
A move is `sims` consecutive batches; once the last games of a call run out of
live leaves a batch can be missing, which blurs only the last moves' boundaries.

bucket_loss() is the balls-in-bins figure behind the choice: the share of random
distinct keys that find their bucket(s) full while a table fills to a threshold.

  python3 scripts/eval_cache_hitrate.py --games 128 --sims 800 --blocks 6
"""
import argparse
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))


class Table:
    def __init__(self, capacity, delay=0):
        self.capacity, self.keys, self.lookups, self.hits, self.clears = capacity, set(), 0, 0, 0
        self.pending = [[] for _ in range(delay)]   # batches evaluated but not yet inserted

    def batch(self, keys):
        self.lookups += len(keys)
        self.hits += sum(k in self.keys for k in keys)
        self.pending.append(keys)
        for k in self.pending.pop(0):
            if self.capacity is None or len(self.keys) < self.capacity:
                self.keys.add(k)

    def end_move(self):
        if self.capacity is not None and 4 * len(self.keys) > 3 * self.capacity:
            self.keys.clear()
            self.clears += 1


def key_hash(key):
    """64 bits of a key (bytes), split like the device's hash: high half, low half"""
    return int.from_bytes(hashlib.blake2b(key, digest_size=8).digest(), "little")


def candidate_buckets(h, buckets, choices):
    """the device's rule (search.hip, cache_buckets): the high and the low 32 bits of
    one hash, masked; equal halves give first ^ 1; one bucket has one candidate"""
    mask = buckets - 1
    b0 = (h >> 32) & mask
    if choices == 1:
        return (b0,)
    b1 = h & mask
    if b1 == b0:
        b1 = (b0 ^ 1) & mask
    return (b0,) if b1 == b0 else (b0, b1)


class BucketTable:
    """the device's table: `capacity` entries as buckets (a power of two) of `ways`
    entries, insert-only; a position has one candidate bucket or two (choices), goes
    to the one with more empty ways (ties: the first) and is dropped when they are
    full; emptied between moves once more than fill = (num, den) of the capacity is
    claimed.  ways None: unlimited, which is Table."""

    def __init__(self, capacity, ways=8, choices=1, fill=(3, 4), delay=0):
        self.capacity, self.ways, self.choices, self.fill = capacity, ways, choices, fill
        self.buckets = 1
        while ways is not None and self.buckets * 2 * ways <= capacity:
            self.buckets *= 2
        if ways is not None:
            self.capacity = self.buckets * ways
        self.keys, self.count = set(), [0] * self.buckets
        self.lookups = self.hits = self.clears = self.inserts = self.dropped = 0
        self.pending = [[] for _ in range(delay)]

    def insert(self, k):
        if k in self.keys:
            return
        if len(self.keys) >= self.capacity:
            self.dropped += 1
            return
        if self.ways is not None:
            cand = candidate_buckets(key_hash(k), self.buckets, self.choices)
            b = min(cand, key=lambda c: self.count[c])   # (min takes the first of equals)
            if self.count[b] >= self.ways:
                self.dropped += 1
                return
            self.count[b] += 1
        self.keys.add(k)
        self.inserts += 1

    def batch(self, keys):
        self.lookups += len(keys)
        self.hits += sum(k in self.keys for k in keys)
        self.pending.append(keys)
        for k in self.pending.pop(0):
            self.insert(k)

    def end_move(self):
        if self.fill[1] * len(self.keys) > self.fill[0] * self.capacity:
            self.keys.clear()
            self.count = [0] * self.buckets
            self.clears += 1


def bucket_loss(buckets, ways, choices, fill, seed=0):
    """random distinct keys offered to an empty table until `fill` of its entries are
    claimed -> the share of the offered keys that found their bucket(s) full"""
    rng = np.random.default_rng(seed)
    count = [0] * buckets
    target, claimed, offered = int(fill * buckets * ways), 0, 0
    while claimed < target:
        for h in rng.integers(0, 1 << 63, 65536, dtype=np.int64).tolist():
            h = (h * 2) ^ (h >> 31)   # (64 bits; distinct with all but negligible probability)
            cand = candidate_buckets(h, buckets, choices)
            b = min(cand, key=lambda c: count[c])
            offered += 1
            if count[b] < ways:
                count[b] += 1
                claimed += 1
                if claimed == target:
                    break
    return (offered - claimed) / offered


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--capacities", type=int, nargs="*", default=[65536, 131072, 262144, 524288])
    ap.add_argument("--delay", type=int, default=0,
                    help="batches between a batch's evaluation and its insertion (0: before the next batch's lookup, "
                         "as an insert from the forward; 1: after the next batch's lookup, as an insert from the tree "
                         "kernel that follows its select)")
    args = ap.parse_args()

    import oracle as O
    import refcpu

    tables = [Table(None, args.delay)] + [Table(c, args.delay) for c in args.capacities]
    shaped = [(c, [BucketTable(c, 8, ch, fill, args.delay) for ch, fill in ((1, (3, 4)), (2, (3, 4)), (2, (7, 8)))])
              for c in args.capacities]
    everything = tables + [t for _, ts in shaped for t in ts]
    per_move = {}   # move -> [lookups, hits] of the unbounded table
    dup = [0]

    class Counting(refcpu.TorchEval):
        def __call__(self, user, n, states, priors, values):
            move = self.calls // args.sims
            super().__call__(user, n, states, priors, values)   # leaves the batch's encodings in self.enc
            planes = self.enc[:n, :84] > 0.5                   # the mover's stones, then the opponent's
            keys = [np.packbits(p).tobytes() for p in planes]
            dup[0] += len(keys) - len(set(keys))
            if move != getattr(self, "move", 0):
                for t in everything:
                    t.end_move()
            self.move = move
            before = (tables[0].lookups, tables[0].hits)
            for t in everything:
                t.batch(keys)
            pm = per_move.setdefault(move, [0, 0])
            pm[0] += tables[0].lookups - before[0]
            pm[1] += tables[0].hits - before[1]

    ev = Counting(args.blocks, args.seed, args.threads, args.games)
    r = O.self_play(O.GAME_CONNECT4, args.games, args.sims, args.seed, eval_kind=O.EVAL_NET, eval_fn=ev, max_plies=42)
    u = tables[0]
    print("games %d  sims/move %d  net %dx64  seed %d" % (args.games, args.sims, args.blocks, args.seed))
    print("leaf evaluations %d  distinct positions %d  duplicates inside a batch %d (%.3f)" %
          (u.lookups, len(u.keys), dup[0], dup[0] / max(1, u.lookups)))
    print("unbounded table: hit rate %.3f  (oracle evals %d)" % (u.hits / max(1, u.lookups), int(r["evals"])))
    print("per move (unbounded): " + " ".join("%d:%.2f" % (m, h / max(1, n)) for m, (n, h) in sorted(per_move.items())))
    for t in tables[1:]:
        print("capacity %8d (%6.0f per game): hit rate %.3f  clears %d" %
              (t.capacity, t.capacity / args.games, t.hits / max(1, t.lookups), t.clears))
    for c, ts in shaped:
        for t, name in zip(ts, ("one bucket, clear at 3/4", "two buckets, clear at 3/4", "two buckets, clear at 7/8")):
            print("capacity %8d as %d x 8 ways, %s: hit rate %.3f  inserts %d  dropped %d (%.2f %%)  clears %d" %
                  (t.capacity, t.buckets, name, t.hits / max(1, t.lookups), t.inserts, t.dropped,
                   100.0 * t.dropped / max(1, t.inserts + t.dropped), t.clears))


if __name__ == "__main__":
    main()
