"""Streamed Connect4 self-play at the bench configuration with root noise off and on
(a record, not a test): what the noise costs and what it buys.

Per configuration, in a fresh child process: --steps x --games games streamed through
--games tree slots at --sims simulations (bench.py's default workload), after --warmup
steps' worth of games.  Reported per configuration:
  sims_per_sec          the timed stream's simulations over its wall time
  cache_hit_rate        evaluation-cache hits / lookups over the timed stream
  leaves_per_forward    forwarded leaves per evaluator launch (the engine's sampled timers)
  distinct_positions    over the first --games games of the timed stream, the number of
                        distinct positions after 1, 2, 4 and 8 plies (games that short
                        are left out)
  timers                the engine's sampled per-kernel averages; the unfused first iteration
                        of a noisy call adds one k_expand and one k_select launch per chain
                        to the call's 2 x sims, and two k_root_noise launches, of which
                        draw_ms bounds one (the draw-only kernel over --games keys of 7
                        children, host wall time with its copies)

  python scripts/c4_noise_bench.py --noise 0.3,0.25 --noise 1.0,0.25 --out profiles/c4_root_noise/noise_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-play-ai_amd"))


def child(args, noise):
    import spai
    G = args.games
    eng = spai.Engine(num_searches=args.sims, max_trees=G, eval_kind=spai.EVAL_NET, seed=args.seed, root_noise=noise)
    eng.set_net(spai.Net(eng, args.blocks, spai.init_params(args.blocks, 64, seed=args.seed)))
    if args.warmup:
        eng.self_play(args.warmup * G, game_id_base=0, collect=False, window=G)
    eng.sync()
    eng.set_timing(True, stride=32)
    c0 = eng.eval_cache_stats()
    base = args.warmup * G
    t0 = time.perf_counter()
    games, st = eng.self_play(args.steps * G, game_id_base=base, collect=lambda gid: gid < base + G, window=G)
    eng.sync()
    dt = time.perf_counter() - t0
    c1 = eng.eval_cache_stats()
    tm = eng.timing()
    distinct = {}
    for k in (1, 2, 4, 8):
        seen = {g["enc"][k].tobytes() for g in games if len(g["value"]) > k}
        distinct[str(k)] = dict(distinct=len(seen), games=sum(len(g["value"]) > k for g in games))
    draw_ms = None
    if noise is not None:
        keys = (np.arange(G, dtype=np.uint64), np.zeros(G, np.uint32), np.full(G, 7, np.uint32))
        eng.root_noise_draws(*keys)
        t1 = time.perf_counter()
        for _ in range(20):
            eng.root_noise_draws(*keys)
        draw_ms = (time.perf_counter() - t1) / 20 * 1e3
    lookups, hits = c1["lookups"] - c0["lookups"], c1["hits"] - c0["hits"]
    out = dict(noise=noise, sims_per_sec=st["sims"] / dt, games_per_sec=st["games"] / dt, seconds=dt,
               sims=st["sims"], evals=st["evals"], search_calls=st["moves"],
               cache_hit_rate=hits / lookups if lookups else 0.0, cache_lookups=lookups, cache_hits=hits,
               leaves_per_forward=tm["evaluate"]["items"] / max(tm["evaluate"]["launches"], 1.0),
               distinct_positions=distinct, game_length_mean=float(np.mean([len(g["value"]) for g in games])),
               timers={k: dict(avg_ms=float(v["avg_ms"]), launches=float(v["launches"])) for k, v in tm.items()},
               draw_ms=draw_ms)
    eng.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--noise", action="append", default=[], metavar="ALPHA,EPS",
                    help="a configuration with noise on (repeatable); noise off always runs first")
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the results as JSON here as well")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child(args, None if args.child == "off" else tuple(float(v) for v in args.child.split(",")))
        return
    results = []
    for cfg in ["off"] + args.noise:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg] + [
            a for k in ("games", "sims", "blocks", "steps", "warmup", "seed") for a in ("--" + k, str(getattr(args, k)))]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"configuration {cfg} failed with status {p.returncode}")
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        results.append(r)
        print(f"noise {cfg:>9}: {r['sims_per_sec'] / 1e6:7.2f}M sims/s, cache hit rate {r['cache_hit_rate']:.3f}, "
              f"{r['leaves_per_forward']:.0f} leaves per forward, distinct positions "
              + ", ".join(f"{k} plies {v['distinct']}/{v['games']}" for k, v in r["distinct_positions"].items()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(config={k: getattr(args, k) for k in ("games", "sims", "blocks", "steps", "warmup", "seed")},
                           results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
