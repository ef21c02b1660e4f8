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
candidate bucket per position or the emptier of two, cleared at 3/4 or 7/8), and
of the table that is thinned past the threshold instead of emptied (ThinTable: the
shipped ranking and the alternatives it was chosen from).  --calls N plays N
successive self_play calls into the same tables.
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


class ThinTable:
    """the device's table with thinning (search.hip, "thinning"): BucketTable's buckets,
    ways, candidate buckets and fill threshold, but past the threshold, between moves
    (the device's search calls), the table is thinned to keep = (num, den) of its
    capacity instead of emptied.  An entry carries the number of the move in which it
    was inserted and of the latest one in which a lookup hit it.  Ranking: the hit class
    (entries with at least min_hits hits) first, but at most hit_share = (num, den) of
    the budget, then the never-hit class in what the hit class left of the budget; in
    each class younger before older (age: moves since the latest stamp, at most
    AGES - 1), whole ages only: an age that would cross the budget goes whole.  A
    thinning counts as a clear too, as on the device.
    The shipped rule is min_hits 1, hit_share 3/4; hit_share (1, 1) is the unguarded
    "hit first", (0, 1) recency alone."""
    AGES = 256

    def __init__(self, capacity, ways=8, choices=2, fill=(7, 8), keep=(1, 2), hit_share=(3, 4), min_hits=1, delay=0):
        self.ways, self.choices, self.fill, self.keep = ways, choices, fill, keep
        self.hit_share, self.min_hits = hit_share, min_hits
        self.buckets = 1
        while self.buckets * 2 * ways <= capacity:
            self.buckets *= 2
        self.capacity = self.buckets * ways
        self.entries, self.count = {}, [0] * self.buckets   # key -> [bucket, born, latest hit (0: none), hits]
        self.seq = 1
        self.lookups = self.hits = self.clears = self.inserts = self.dropped = 0
        self.thins = self.evicted = self.kept_hit = 0
        self.pending = [[] for _ in range(delay)]

    def __len__(self):
        return len(self.entries)

    def lookup(self, k):
        self.lookups += 1
        e = self.entries.get(k)
        if e is None:
            return False
        self.hits += 1
        e[2] = self.seq
        e[3] += 1
        return True

    def insert(self, k):
        if k in self.entries:
            return
        cand = candidate_buckets(key_hash(k), self.buckets, self.choices)
        b = min(cand, key=lambda c: self.count[c])   # (min takes the first of equals)
        if self.count[b] >= self.ways:
            self.dropped += 1
            return
        self.count[b] += 1
        self.entries[k] = [b, self.seq, 0, 0]
        self.inserts += 1

    def batch(self, keys):
        for k in keys:
            self.lookup(k)
        self.pending.append(keys)
        for k in self.pending.pop(0):
            self.insert(k)

    def _bin(self, e):
        hit = e[3] >= self.min_hits
        return int(hit), min(self.AGES - 1, self.seq - (e[2] if hit else e[1]))

    def cutoff(self, hist, keep):
        """hist[cls][age] -> (cut[cls]: the first age dropped, kept[cls]); search.hip, thin_cutoff"""
        cut, kept = [0, 0], [0, 0]
        if sum(hist[0]) + sum(hist[1]) <= keep:
            return [self.AGES, self.AGES], [sum(hist[0]), sum(hist[1])]
        for cls in (1, 0):
            budget = keep * self.hit_share[0] // self.hit_share[1] if cls else keep - kept[1]
            while cut[cls] < self.AGES and kept[cls] + hist[cls][cut[cls]] <= budget:
                kept[cls] += hist[cls][cut[cls]]
                cut[cls] += 1
        return cut, kept

    def thin(self, keep):
        """thin now to at most `keep` entries; with no more than that in the table nothing
        is evicted and nothing counted"""
        hist = [[0] * self.AGES, [0] * self.AGES]
        for e in self.entries.values():
            cls, age = self._bin(e)
            hist[cls][age] += 1
        cut, kept = self.cutoff(hist, keep)
        if sum(kept) == len(self.entries):
            return
        for k in [k for k, e in self.entries.items() if self._bin(e)[1] >= cut[self._bin(e)[0]]]:
            self.count[self.entries.pop(k)[0]] -= 1
        self.thins += 1
        self.clears += 1
        self.evicted += sum(hist[0]) + sum(hist[1]) - sum(kept)
        self.kept_hit = kept[1]
        self.last_hist = hist

    def end_move(self):
        if self.fill[1] * len(self.entries) > self.fill[0] * self.capacity:
            self.thin(self.capacity * self.keep[0] // self.keep[1])
        self.seq += 1


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
    ap.add_argument("--calls", type=int, default=1,
                    help="successive self_play calls (seeds seed, seed + 1, ...) into the same tables: a crude stand-in "
                         "for the stream, where new games keep walking through positions older ones left")
    args = ap.parse_args()

    import oracle as O
    import refcpu

    tables = [Table(None, args.delay)] + [Table(c, args.delay) for c in args.capacities]
    shaped = [(c, [BucketTable(c, 8, ch, fill, args.delay) for ch, fill in ((1, (3, 4)), (2, (3, 4)), (2, (7, 8)))])
              for c in args.capacities]
    # thinning instead of emptying, at 7/8 to 1/2: the shipped rule, then the alternatives it was chosen from
    THIN = (("thin: hit first, at most 3/4 (shipped)", dict()),
            ("thin: recency only", dict(hit_share=(0, 1))),
            ("thin: hit first, unguarded", dict(hit_share=(1, 1))),
            ("thin: hit first, at most 1/2", dict(hit_share=(1, 2))),
            (">= 2 hits first, at most 3/4", dict(min_hits=2)),
            ("thin to 1/4 (shipped rule)", dict(keep=(1, 4))),
            ("thin to 3/4 (shipped rule)", dict(keep=(3, 4))))
    thinned = [(c, [ThinTable(c, delay=args.delay, **kw) for _, kw in THIN]) for c in args.capacities]
    everything = tables + [t for _, ts in shaped + thinned for t in ts]
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

    for call in range(args.calls):   # (the net is the same in every call: TorchEval's seed is the net's)
        ev = Counting(args.blocks, args.seed, args.threads, args.games)
        r = O.self_play(O.GAME_CONNECT4, args.games, args.sims, args.seed + call, eval_kind=O.EVAL_NET, eval_fn=ev,
                        max_plies=42)
        for t in everything:
            t.end_move()
    u = tables[0]
    print("games %d  sims/move %d  net %dx64  seed %d  calls %d" % (args.games, args.sims, args.blocks, args.seed, args.calls))
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
    for c, ts in thinned:
        for t, (name, _) in zip(ts, THIN):
            print("capacity %8d as %d x 8 ways, two buckets, 7/8, %s: hit rate %.3f  inserts %d  dropped %d  thinnings %d  "
                  "evicted %d  hit class kept at the last %d" %
                  (t.capacity, t.buckets, name, t.hits / max(1, t.lookups), t.inserts, t.dropped, t.thins, t.evicted,
                   t.kept_hit))


if __name__ == "__main__":
    main()
