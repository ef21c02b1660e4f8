"""The Connect4 learn loop and its weight refresh, measured (a record, not a test).

  --bench   at 6x64, in one process, the three routes that bring a learner's weights
            into the engine's self-play net, alternated --reps times each (host time
            up to an engine sync, so the device work is counted):
              parent   L.params(), Net(...), Engine.set_net, old net closed -- what the
                       loop had to do before Net.set_params existed
              host     Net.set_params(array): upload + the device pack (and, as
                       host_with_readback, the L.params() read-back spai.learn's
                       refresh="host" pays before it)
              device   Net.set_params(L): the device pack on the learner's parameters
            median and spread (min, max, quartiles) in ms; then spai.learn for two
            iterations at a stated shape with the seconds of iteration 1 spent in
            refresh, self-play and training (iteration 0 has no refresh).
  --learn   a short spai.learn, then Engine.match of the last checkpoint against
            init:<seed> and against uniform MCTS at equal simulations: W/D/L by first
            mover, as scripts/c4_match.py prints it.  Recorded only: playing strength
            after a short run is asserted nowhere.

Both merge their result into --out (default profiles/c4_learn/record.json).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.dirname(os.path.abspath(__file__)), os.path.join(REPO, "self-play-ai_amd")):
    sys.path.insert(0, p)


def _spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(n=len(a), median=float(np.median(a)), min=float(a[0]), max=float(a[-1]),
                q25=float(np.percentile(a, 25)), q75=float(np.percentile(a, 75)))


def _learn_timed(spai, cfg, **kw):
    """spai.learn with the per-iteration seconds by phase"""
    phases = {}

    def on_phase(i, name, s):
        d = phases.setdefault(i, dict(refresh=0.0, self_play=0.0, train=0.0))
        d[name] += s

    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rec = spai.learn(checkpoint_dir=d, on_phase=on_phase, **cfg, **kw)
        secs = time.perf_counter() - t0
        final = spai.load_params(rec[-1]["checkpoint"], cfg["blocks"])
    for r in rec:
        r["checkpoint"] = os.path.basename(r["checkpoint"])
        r["seconds"] = phases.get(r["iteration"])
    return rec, secs, final


def bench(args):
    import spai
    blocks, trees = 6, 100
    eng = spai.Engine(num_searches=32, max_trees=trees, eval_kind=spai.EVAL_NET, seed=0)
    p0 = spai.init_params(blocks, seed=0)
    eng.set_net(spai.Net(eng, blocks, p0))
    eng.trees_create(trees)
    eng.search(np.arange(trees))   # the evaluation cache's table exists: every route clears it
    L = spai.Learner(eng, blocks, p0)
    rng = np.random.default_rng(0)
    x = (rng.random((32, 3, 6, 7)) < 0.3).astype(np.float32)
    pi = rng.dirichlet(np.ones(7), 32).astype(np.float32)
    L.train_batch(x, pi, rng.choice([-1.0, 0.0, 1.0], 32).astype(np.float32))
    P = L.params()

    def parent():
        old = eng.net
        eng.set_net(spai.Net(eng, blocks, L.params()))
        old.close()

    routes = dict(parent=parent, host=lambda: eng.net.set_params(P),
                  host_with_readback=lambda: eng.net.set_params(L.params()), device=lambda: eng.net.set_params(L))
    times = {k: [] for k in routes}
    for rep in range(args.warmup + args.reps):
        for name, fn in routes.items():
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            if rep >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    L.close()
    eng.close()
    refresh = {k: _spread(v) for k, v in times.items()}
    for k, v in refresh.items():
        print(f"refresh {k:>18}: median {v['median']:.3f} ms  [{v['min']:.3f}, {v['max']:.3f}]  n={v['n']}")
    cfg = dict(num_learn_iters=2, num_self_play_iters=4, num_parallel_self_play_games=100, batch_size=32,
               num_epochs=4, num_searches=args.sims, blocks=blocks, seed=0)
    rec, secs, _ = _learn_timed(spai, cfg)
    print(f"learn {cfg}: {secs:.1f} s; iteration 1 seconds {rec[1]['seconds']}")
    return dict(net="6x64 bf16", engine_trees=trees, reps=args.reps, warmup=args.warmup, unit="ms",
                refresh=refresh, learn=dict(config=cfg, refresh="device", seconds=secs, iterations=rec))


def learn(args):
    import c4_match
    import spai
    cfg = dict(num_learn_iters=args.iters, num_self_play_iters=args.self_play_iters,
               num_parallel_self_play_games=args.games, batch_size=args.batch, num_epochs=args.epochs,
               num_searches=args.sims, blocks=args.blocks, seed=args.seed, clone_self_play=not args.distinct)
    noise = tuple(args.root_noise) if args.root_noise else None
    rec, secs, final = _learn_timed(spai, cfg, window=args.window, root_noise=noise)
    for r in rec:
        print(r)
    per_call = args.play_games
    eng = spai.Engine(num_searches=args.play_sims, max_trees=2 * per_call, eval_kind=spai.EVAL_UNIFORM)
    a = (spai.EVAL_NET, spai.Net(eng, args.blocks, final), args.play_sims)
    out = {}
    for spec in (f"init:{args.seed}", "uniform"):
        b = c4_match.make_player(spai, eng, spec, args.play_sims, args.blocks, spai.DTYPE_BF16)
        out[spec] = c4_match.play(spai, eng, a, b, args.play_games, per_call, 4, args.seed)
        print(f"last checkpoint vs {spec}: {json.dumps(out[spec])}")
    eng.close()
    return dict(config=cfg, window=args.window, root_noise=noise, seconds=secs, iterations=rec,
                match=dict(a="last checkpoint", sims=args.play_sims, games=args.play_games, opening_plies=4, vs=out),
                note="recorded only: one short run, strength is not asserted")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "c4_learn", "record.json"))
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--reps", type=int, default=30, help="--bench: timed refreshes per route (at least 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--self-play-iters", type=int, default=4)
    ap.add_argument("--distinct", action="store_true", help="clone_self_play=False")
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--root-noise", type=float, nargs=2, default=None, metavar=("ALPHA", "EPS"),
                    help="--learn: Dirichlet root noise in self-play (spai.learn(root_noise=)); the matches never use it")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--play-sims", type=int, default=100)
    ap.add_argument("--play-games", type=int, default=128)
    args = ap.parse_args()
    if not (args.bench or args.learn):
        ap.error("give --bench and/or --learn")
    if args.bench and args.reps < 20:
        ap.error("--reps must be at least 20")
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    record = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            record = json.load(f)
    record["commit"] = commit
    if args.bench:
        record["bench"] = bench(args)
    if args.learn:
        record["learn"] = learn(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
