"""Chess matches between two evaluators on the device (ChessEngine.match, spai_chess_match_run).

  python scripts/chess_match.py A B [--games N] [--sims-a K] [--sims-b K] [--blocks B]
                                    [--dtype-a {bf16,f32}] [--dtype-b {bf16,f32}]
                                    [--opening-plies P] [--max-plies M] [--seed S] [--max-trees T]

A and B are each a safetensors checkpoint (spai_params_load_safetensors), or one of
  init:<seed>   the random initial weights of that seed
  uniform       plain MCTS on uniform priors and value 0, without a network
  hash          the deterministic hash evaluator of the parity tests
--dtype-a / --dtype-b choose the arithmetic of a net player (ChessNet's dtype, default
bf16): `ckpt ckpt --dtype-b f32` plays one checkpoint's bf16 net against its own
unquantised fp32 net, i.e. measures what bf16 costs it in Elo.  The fp32 net is the
parity path, about 50 times slower (profiles/chess_net_f32): keep --sims and --blocks small.
Prints one JSON line: wins, draws and losses of A split by who moved first, the
games adjudicated a draw at --max-plies, A's score, the Elo difference (A - B) with
a 95 % interval from the trinomial counts (scripts/c4_match.py's arithmetic), and
sims/s.  Games beyond what the engine holds at once are played as further calls
(ids go on, so the pairs and openings are those of one long match).  A game holds
two trees of about 19.5 MB each at 400 simulations: --max-trees bounds the memory.

  --bench   the measurement of DESIGN.md "Chess matches": a 512-game match (2 x 512
            trees) of a net against itself at 400 simulations over --bench-plies
            searched plies, on two streams and with both chains on one stream (and
            the same pair for the net against the uniform player, whose chain runs
            no forward), and
            the self-play move loop (search + advance) at 1,024 trees over the same
            plies, alternated --bench-reps times in one process.  Written to --out
            (default profiles/chess_match/record.json).
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "self-play-ai_amd"), os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from c4_match import elo_from_counts  # noqa: E402  (the scoring is Connect4's, unchanged)

COUNTS = ("a_wins", "draws", "b_wins", "sims", "evals")


def describe(spec, dtype):
    """a player as the report names it: net players with their dtype"""
    return spec if spec in ("uniform", "hash") else f"{spec} ({dtype})"


def make_player(sc, eng, spec, sims, blocks, dtype="bf16"):
    import spai
    if spec == "uniform":
        return (sc.EVAL_UNIFORM, None, sims)
    if spec == "hash":
        return (sc.EVAL_HASH, None, sims)
    if spec.startswith("init:"):
        params = sc.init_params(blocks, int(spec[5:]))
    else:
        params = spai.load_params(spec, blocks, 256, game=sc.GAME_CHESS, n=sc.num_params(blocks))
    return (sc.EVAL_NET, sc.ChessNet(eng, blocks, params, dtype=dtype), sims)


def report(tot, games, seconds):
    """the result line of a match from its summed counts"""
    w, d, l = sum(tot["a_wins"]), sum(tot["draws"]), sum(tot["b_wins"])
    out = dict(games=games, a_wins=tot["a_wins"], draws=tot["draws"], b_wins=tot["b_wins"],
               first_mover="[0]: A moved first, [1]: B moved first", adjudicated=tot["adjudicated"],
               plies=tot["plies"], sims=tot["sims"], evals=tot["evals"], seconds=seconds,
               sims_per_s=sum(tot["sims"]) / seconds if seconds else None)
    out.update(elo_from_counts(w, d, l) or {})
    return out


def play(eng, a, b, games, per_call, opening_plies, max_plies, seed):
    tot = {k: [0.0, 0.0] for k in COUNTS}
    tot.update(adjudicated=0.0, plies=0.0)
    seconds, done = 0.0, 0
    while done < games:
        n = min(per_call, games - done)
        _, st = eng.match(a, b, n, game_id_base=done, opening_plies=opening_plies, max_plies=max_plies, seed=seed,
                          keep_moves=False)
        for k in COUNTS:
            tot[k] = [x + y for x, y in zip(tot[k], st[k])]
        tot["adjudicated"] += st["adjudicated"]
        tot["plies"] += st["plies"]
        seconds += st["seconds"]
        done += n
    return report(tot, games, seconds)


def selfplay_loop(eng, np, trees, sims, plies):
    """self-play's move loop through the public API (scripts/chess_bench.py's): search all
    trees, pick the most-visited child, advance; sims/s over `plies` moves from fresh trees"""
    eng.trees_create(trees)
    live = np.arange(trees, dtype=np.uint32)
    done = 0
    t0 = time.perf_counter()
    for _ in range(plies):
        _, _, vis, _, nc = eng.search(live)
        done += len(live) * sims
        vis[np.arange(vis.shape[1])[None, :] >= nc[:, None]] = -1
        status, _ = eng.advance(live, vis.argmax(1).astype(np.uint32))
        live = live[status == 0]
    return done / (time.perf_counter() - t0)


def bench(args):
    import numpy as np

    import spai_chess as sc
    games, sims, plies, opening = 512, 400, args.bench_plies, 2
    eng = sc.ChessEngine(num_searches=sims, max_trees=2 * games, eval_kind=sc.EVAL_NET, seed=0)
    net = sc.ChessNet(eng, args.blocks, sc.init_params(args.blocks, 1))
    eng.set_net(net)
    pl = (sc.EVAL_NET, net, sims)
    eng.match(pl, pl, 8, opening_plies=opening, max_plies=opening + 1, keep_moves=False)   # warm-up

    uni = (sc.EVAL_UNIFORM, None, sims)

    def match(one_stream, b=None):
        eng.match_one_stream(one_stream)
        try:
            _, st = eng.match(pl, b or pl, games, opening_plies=opening, max_plies=opening + plies, seed=0,
                              keep_moves=False)
        finally:
            eng.match_one_stream(False)
        return sum(st["sims"]) / st["seconds"]

    runs = []
    for _ in range(args.bench_reps):
        two = match(False)
        one = match(True)
        utwo = match(False, uni)
        uone = match(True, uni)
        sp = selfplay_loop(eng, np, 2 * games, sims, plies)
        runs.append(dict(match_two_streams_sims_per_s=two, match_one_stream_sims_per_s=one,
                         net_vs_uniform_two_streams_sims_per_s=utwo, net_vs_uniform_one_stream_sims_per_s=uone,
                         selfplay_loop_sims_per_s=sp, two_over_one=two / one,
                         net_vs_uniform_two_over_one=utwo / uone, two_over_selfplay=two / sp))
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or None
        except OSError:
            commit = None
    rec = dict(config=dict(blocks=args.blocks, games=games, trees=2 * games, sims=sims, opening_plies=opening,
                           searched_plies=plies, players="one bf16 net object (init:1) on both sides; net_vs_uniform: that net against uniform priors"),
               runs=runs, commit=commit,
               note="one process, runs alternated; the self-play figure is the search + advance loop over "
                    "1,024 fresh trees (the root statistics and dense policies copied back each ply)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a", nargs="?")
    ap.add_argument("b", nargs="?")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims-a", type=int, default=400)
    ap.add_argument("--sims-b", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--dtype-a", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--dtype-b", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--opening-plies", type=int, default=2)
    ap.add_argument("--max-plies", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-trees", type=int, default=1024)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-plies", type=int, default=4)
    ap.add_argument("--bench-reps", type=int, default=2)
    ap.add_argument("--commit", default=None, help="label of the measured tree for --bench (default: git HEAD)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chess_match", "record.json"))
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.bench:
        return bench(args)
    if not args.a or not args.b:
        ap.error("two players: a checkpoint, init:<seed>, uniform or hash")
    import spai_chess as sc
    per_call = max(1, min(args.games, args.max_trees // 2))
    eng = sc.ChessEngine(num_searches=max(args.sims_a, args.sims_b), max_trees=2 * per_call,
                         eval_kind=sc.EVAL_UNIFORM)
    a = make_player(sc, eng, args.a, args.sims_a, args.blocks, args.dtype_a)
    b = make_player(sc, eng, args.b, args.sims_b, args.blocks, args.dtype_b)
    out = dict(a=describe(args.a, args.dtype_a), b=describe(args.b, args.dtype_b), sims_a=args.sims_a, sims_b=args.sims_b, opening_plies=args.opening_plies,
               max_plies=args.max_plies, blocks=args.blocks, seed=args.seed)
    out.update(play(eng, a, b, args.games, per_call, args.opening_plies, args.max_plies, args.seed))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
