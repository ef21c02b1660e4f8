#!/usr/bin/env python3
"""Hit rate an evaluation cache would see in Connect4 self-play, measured on the
CPU with the oracle (no GPU): oracle.self_play with the libtorch fp32 net
(refcpu.TorchEval), games played to completion; every leaf batch (one search
iteration over the games in play) is looked up before that batch's own results
are inserted, as the device does it (search.hip, evaluation cache).

Prints the overall hit rate of an unbounded table, the rate per move, and the
rate of bounded insert-only tables that are emptied between moves once more
than 3/4 full (fully associative here; the device's 8-way buckets drop a few
more inserts).  A move is `sims` consecutive batches; once the last games of a
call run out of live leaves a batch can be missing, which blurs only the last
moves' boundaries.

  python3 scripts/eval_cache_hitrate.py --games 128 --sims 800 --blocks 6
"""
import argparse
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
                for t in tables:
                    t.end_move()
            self.move = move
            before = (tables[0].lookups, tables[0].hits)
            for t in tables:
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


if __name__ == "__main__":
    main()
