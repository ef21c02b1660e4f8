"""Connect4 matches between two evaluators on the device (Engine.match, spai_match_run).

  python scripts/c4_match.py A B [--games N] [--sims-a K] [--sims-b K] [--opening-plies P]
                                 [--blocks B] [--dtype bf16|f32] [--seed S]

A and B are each a safetensors checkpoint (spai_params_load_safetensors), or one of
  init:<seed>   the random initial weights of that seed
  uniform       plain MCTS on uniform priors and value 0, without a network
  hash          the deterministic hash evaluator of the parity tests
Prints one JSON line: wins, draws and losses of A split by who moved first, A's
score, the Elo difference (A - B) with a 95 % interval from the trinomial counts,
and sims/s.  Games beyond what the engine holds at once are played as further
calls (ids go on, so the pairs and openings are those of one long match).

  --bench   the measurement of DESIGN.md "Matches": a 2,048-game match of a 6 x 64
            bf16 net against itself at 800 simulations and 4 opening plies, and a
            spai_selfplay_run of 2,048 lockstep games with the same net, alternated
            twice each; then init:1 against uniform over 512 games at 800
            simulations.  Merged into --out (default profiles/match/record.json).
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-play-ai_amd"))


def elo_from_counts(w, d, l):
    """A's score, the Elo difference it stands for, and a 95 % interval: the per-game
    score (1, 1/2, 0) is trinomial, its mean's standard error sqrt(var / n); the
    interval's ends are mapped through the same logistic curve (None where an end
    reaches 0 or 1)"""
    n = w + d + l
    if n == 0:
        return None
    s = (w + 0.5 * d) / n
    var = (w * (1 - s) ** 2 + d * (0.5 - s) ** 2 + l * (0 - s) ** 2) / n
    se = math.sqrt(var / n)

    def elo(x):
        return None if x <= 0 or x >= 1 else -400.0 * math.log10(1.0 / x - 1.0)

    return dict(score=s, elo=elo(s), elo_lo=elo(s - 1.96 * se), elo_hi=elo(s + 1.96 * se), score_se=se)


def make_player(spai, eng, spec, sims, blocks, dtype):
    if spec == "uniform":
        return (spai.EVAL_UNIFORM, None, sims)
    if spec == "hash":
        return (spai.EVAL_HASH, None, sims)
    if spec.startswith("init:"):
        params = spai.init_params(blocks, 64, seed=int(spec[5:]))
    else:
        params = spai.load_params(spec, blocks)
    return (spai.EVAL_NET, spai.Net(eng, blocks, params, dtype=dtype), sims)


def play(spai, eng, a, b, games, per_call, opening_plies, seed):
    tot = {k: [0.0, 0.0] for k in ("a_wins", "draws", "b_wins", "sims", "evals")}
    seconds, done = 0.0, 0
    while done < games:
        n = min(per_call, games - done)
        _, st = eng.match(a, b, n, opening_plies=opening_plies, seed=seed, game_id_base=done)
        for k in tot:
            tot[k] = [x + y for x, y in zip(tot[k], st[k])]
        seconds += st["seconds"]
        done += n
    w, d, l = sum(tot["a_wins"]), sum(tot["draws"]), sum(tot["b_wins"])
    out = dict(games=games, a_wins=tot["a_wins"], draws=tot["draws"], b_wins=tot["b_wins"],
               first_mover="[0]: A moved first, [1]: B moved first", sims=tot["sims"], evals=tot["evals"],
               seconds=seconds, sims_per_s=sum(tot["sims"]) / seconds if seconds else None)
    out.update(elo_from_counts(w, d, l))
    return out


def bench(args):
    import spai
    blocks, games, sims = 6, 2048, 800
    eng = spai.Engine(num_searches=sims, max_trees=2 * games, eval_kind=spai.EVAL_NET, seed=0)
    net = spai.Net(eng, blocks, spai.init_params(blocks, 64, seed=1))
    eng.set_net(net)
    pl = (spai.EVAL_NET, net, sims)
    runs = []
    for rep in range(2):
        c0 = eng.eval_cache_stats()
        m = play(spai, eng, pl, pl, games, games, 4, seed=rep)
        c1 = eng.eval_cache_stats()
        look = c1["lookups"] - c0["lookups"]
        m["cache_hit_rate"] = (c1["hits"] - c0["hits"]) / look if look else None
        _, sp = eng.self_play(games, game_id_base=rep * games, collect=False)
        runs.append(dict(match_sims_per_s=m["sims_per_s"], match_seconds=m["seconds"],
                         match_cache_hit_rate=m["cache_hit_rate"], selfplay_sims_per_s=sp["sims"] / sp["seconds"],
                         selfplay_seconds=sp["seconds"], ratio=m["sims_per_s"] / (sp["sims"] / sp["seconds"])))
    uni = (spai.EVAL_UNIFORM, None, sims)
    strength = play(spai, eng, pl, uni, 512, 512, 4, seed=0)
    rec = dict(config=dict(blocks=blocks, hidden=64, dtype="bf16", games=games, sims=sims, opening_plies=4),
               runs=runs, init1_vs_uniform=strength,
               note="one session; the strength figure is a single 512-game run of untrained weights")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a", nargs="?")
    ap.add_argument("b", nargs="?")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims-a", type=int, default=800)
    ap.add_argument("--sims-b", type=int, default=800)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-trees", type=int, default=4096)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match", "record.json"))
    args = ap.parse_args()
    if args.bench:
        return bench(args)
    if not args.a or not args.b:
        ap.error("two players: a checkpoint, init:<seed>, uniform or hash")
    import spai
    per_call = max(1, min(args.games, args.max_trees // 2))
    eng = spai.Engine(num_searches=max(args.sims_a, args.sims_b), max_trees=2 * per_call, eval_kind=spai.EVAL_UNIFORM)
    dtype = spai.DTYPE_F32 if args.dtype == "f32" else spai.DTYPE_BF16
    a = make_player(spai, eng, args.a, args.sims_a, args.blocks, dtype)
    b = make_player(spai, eng, args.b, args.sims_b, args.blocks, dtype)
    out = dict(a=args.a, b=args.b, sims_a=args.sims_a, sims_b=args.sims_b, opening_plies=args.opening_plies,
               blocks=args.blocks, dtype=args.dtype, seed=args.seed)
    out.update(play(spai, eng, a, b, args.games, per_call, args.opening_plies, args.seed))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
