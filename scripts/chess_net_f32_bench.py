#!/usr/bin/env python3
"""Device time of the fp32 chess forward beside the bf16 one (profiles/chess_net_f32).

  python scripts/chess_net_f32_bench.py [--blocks 20] [--n 1 256 1024] [--runs 5] [--out FILE]

The fp32 net (ChessNet(dtype="f32"), csrc/chess_net_f32.hip) is the parity path, not a
throughput path; this record exists so that nobody benchmarks it by accident.

What is timed: the forward launch alone, by the engine's own HIP events around
net_eval (spai_chess_set_timing: iteration 0 of a search is sampled).  A one-iteration
search over n fresh trees evaluates exactly the n roots, so its sampled forward is one
launch over n positions.  Per (dtype, n): one warm-up search, then `runs` searches, the
median and the range of their forward times.  Prints one JSON line and writes --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "self-play-ai_amd")]


def forward_ms(sc, np, eng, n, runs):
    out = []
    for k in range(runs + 1):          # the first is the warm-up
        eng.trees_create(n)
        eng.set_timing(True)           # clears the sums: the figures below are this search's alone
        eng.search(np.arange(n, dtype=np.uint32), num_searches=1)
        ms, launches, items = eng.timing()
        assert launches[1] == 1 and items[1] == n, (launches, items)
        if k:
            out.append(float(ms[1]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--commit", default=None, help="label of the measured tree (default: git HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chess_net_f32", "forward.json"))
    args = ap.parse_args()
    import numpy as np

    import spai_chess as sc
    eng = sc.ChessEngine(num_searches=1, max_trees=max(args.n), eval_kind=sc.EVAL_NET)
    eng.set_timing(True)
    params = sc.init_params(args.blocks, 0)
    rows = []
    for dtype in ("bf16", "f32"):
        net = sc.ChessNet(eng, args.blocks, params, dtype=dtype)
        eng.set_net(net)
        for n in args.n:
            t = forward_ms(sc, np, eng, n, args.runs)
            rows.append(dict(dtype=dtype, n=n, forward_ms_median=statistics.median(t), forward_ms_min=min(t),
                             forward_ms_max=max(t), runs=t))
        eng.set_net(None)
        net.close()
    eng.close()
    for n in args.n:
        b, f = (next(r for r in rows if r["dtype"] == d and r["n"] == n) for d in ("bf16", "f32"))
        f["over_bf16"] = f["forward_ms_median"] / b["forward_ms_median"]
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None
        except OSError:
            commit = None
    rec = dict(what="device ms of one forward launch over n positions (HIP events around net_eval), "
                    "median of %d runs after one warm-up" % args.runs,
               blocks=args.blocks, commit=commit, forward=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
