"""The TicTacToe learner, measured and shown to learn (a record, not a test).

  --bench   train steps/s and samples/s of the device step (spai_ttt.TTTLearner.train_batch,
            upload and loss read-back included) at 4x64, B = 32 and B = 128, after
            warm-up; and PyTorch CPU fp32 doing the same step in the same run (the
            reference's libtorch path), with the ratio.
  --learn   spai_ttt.learn() at a small configuration, then the trained net (greedy on
            visit counts) from the empty board, as X and as O, against an exhaustive
            minimax opponent that picks uniformly among its optimal moves: wins, draws
            and losses for the initial and the final weights.

Both merge their result into --out (default profiles/r07/ttt_learner/record.json).
"""
import argparse
import functools
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "self-play-ai_amd")):
    sys.path.insert(0, p)

LINES = [0o7, 0o70, 0o700, 0o111, 0o222, 0o444, 0o421, 0o124]


# ------------------------------------------------------------------ bench
def bench(args):
    import torch

    import spai_ttt as st
    import ttt_learner_ref as LR
    blocks, out = 4, {}
    torch.set_num_threads(args.cpu_threads)
    p0 = st.init_params(blocks, 0)
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    for B in (32, 128):
        _, _, ((x, pi, z),) = LR.make_batches(B, 1, B)
        L = st.TTTLearner(eng, blocks, p0)
        for _ in range(args.warmup):
            L.train_batch(x, pi, z)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            L.train_batch(x, pi, z)
        dev = (time.perf_counter() - t0) / args.steps
        L.close()
        forward, T, _ = LR.torch_net(p0, blocks)
        opt = torch.optim.Adam([t for t, _ in T if t.requires_grad], lr=1e-3)
        tx, tpi, tz = torch.tensor(x.reshape(-1, 3, 3, 3)), torch.tensor(pi), torch.tensor(z)

        def cpu_step():
            logits, v = forward(tx)
            loss = -(torch.log_softmax(logits, 1) * tpi).sum() / B + ((v - tz) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()

        for _ in range(max(2, args.warmup // 10)):
            cpu_step()
        n_cpu = max(5, args.steps // 10)
        t0 = time.perf_counter()
        for _ in range(n_cpu):
            cpu_step()
        cpu = (time.perf_counter() - t0) / n_cpu
        out[f"B{B}"] = dict(device_steps_per_s=1 / dev, device_samples_per_s=B / dev, device_ms_per_step=dev * 1e3,
                            torch_cpu_steps_per_s=1 / cpu, torch_cpu_samples_per_s=B / cpu,
                            torch_cpu_ms_per_step=cpu * 1e3, device_over_cpu=cpu / dev)
        print(f"B={B}: device {dev * 1e3:.3f} ms/step ({B / dev:.0f} samples/s); torch CPU fp32 "
              f"({args.cpu_threads} threads) {cpu * 1e3:.3f} ms/step ({B / cpu:.0f} samples/s); ratio {cpu / dev:.2f}x")
    eng.close()
    return dict(net="4x64", steps=args.steps, warmup=args.warmup, cpu_threads=args.cpu_threads,
                torch=torch.__version__, results=out)


# ------------------------------------------------------------------ learn + play
def _won(m):
    return any((m & l) == l for l in LINES)


@functools.lru_cache(maxsize=None)
def minimax(x, o, n):
    """(value for the player to move, its optimal moves) by exhaustive search"""
    best, moves = -2, []
    for c in range(9):
        if ((x | o) >> c) & 1:
            continue
        nx, no = (x | (1 << c), o) if n % 2 == 0 else (x, o | (1 << c))
        if _won(nx if n % 2 == 0 else no):
            v = 1
        elif n + 1 == 9:
            v = 0
        else:
            v = -minimax(nx, no, n + 1)[0]
        if v > best:
            best, moves = v, [c]
        elif v == best:
            moves.append(c)
    return best, moves


def play(st, params, blocks, sims, n_games, seed):
    """the net (greedy on visit counts after `sims` searches) against the minimax opponent,
    n_games as X and n_games as O; returns {as_x: [win, draw, loss], as_o: [...]}"""
    rng = np.random.default_rng(seed)
    eng = st.TTTEngine(num_searches=sims, max_trees=n_games, seed=seed)
    eng.set_net(st.TTTNet(eng, blocks, params))
    eng.trees_create(n_games)
    res = {}
    for side in (0, 1):   # the net moves when n % 2 == side
        games = [[0, 0, 0] for _ in range(n_games)]   # x, o, n
        result = [None] * n_games
        while any(r is None for r in result):
            live = [i for i in range(n_games) if result[i] is None]
            net_turn = [i for i in live if games[i][2] % 2 == side]
            moves = {}
            if net_turn:
                for k, i in enumerate(net_turn):
                    x, o, n = games[i]
                    eng.tree_reset(k, np.array((x, o, n, 0, [0, 0]), st.STATE_DTYPE))
                pol, _, _, _ = eng.search(np.arange(len(net_turn)))
                for k, i in enumerate(net_turn):
                    moves[i] = int(np.argmax(pol[k]))
            for i in live:
                x, o, n = games[i]
                c = moves[i] if i in moves else int(rng.choice(minimax(x, o, n)[1]))
                assert not ((x | o) >> c) & 1
                if n % 2 == 0:
                    x |= 1 << c
                else:
                    o |= 1 << c
                games[i] = [x, o, n + 1]
                if _won(x if n % 2 == 0 else o):
                    result[i] = 0 if n % 2 == side else 2
                elif n + 1 == 9:
                    result[i] = 1
        res["as_x" if side == 0 else "as_o"] = [result.count(k) for k in range(3)]
    eng.close()
    return res


def learn(args):
    import spai
    import spai_ttt as st
    p0 = st.init_params(args.blocks, args.seed)
    cfg = dict(num_learn_iters=args.iters, num_self_play_iters=args.self_play_iters,
               num_parallel_self_play_games=args.games, batch_size=args.batch, num_epochs=args.epochs,
               num_searches=args.sims, blocks=args.blocks, seed=args.seed, clone_self_play=not args.distinct)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rec = st.learn(checkpoint_dir=d, **cfg)
        secs = time.perf_counter() - t0
        final = spai.load_params(rec[-1]["checkpoint"], args.blocks, game=spai.GAME_TICTACTOE, n=len(p0))
    for r in rec:
        r["checkpoint"] = os.path.basename(r["checkpoint"])
        print(r)
    before = play(st, p0, args.blocks, args.play_sims, args.play_games, 1)
    after = play(st, final, args.blocks, args.play_sims, args.play_games, 1)
    print(f"learn: {secs:.1f} s; vs minimax [win, draw, loss]: initial {before}  final {after}")
    return dict(config=cfg, seconds=secs, iterations=rec, play=dict(sims=args.play_sims, games_per_side=args.play_games,
                                                                    order="win, draw, loss", initial=before, final=after))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07", "ttt_learner", "record.json"))
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--tag", default="", help="--learn: record under learn_<tag> (several configurations in one file)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--self-play-iters", type=int, default=4)
    ap.add_argument("--distinct", action="store_true", help="clone_self_play=False")
    ap.add_argument("--sims", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--play-sims", type=int, default=60)
    ap.add_argument("--play-games", type=int, default=100)
    args = ap.parse_args()
    if not (args.bench or args.learn):
        ap.error("give --bench and/or --learn")
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
        record["learn" + ("_" + args.tag if args.tag else "")] = learn(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
