"""The chess learner, measured and run end to end (a record, not a test).

  --bench   ms per train step, samples/s and the fraction of the 157.3 TF f32 MFMA
            peak of the device step (spai_chess.ChessLearner.train_batch, upload and
            loss read-back included) at blocks x B in --configs (default 10x32,
            10x128, 20x32, 20x128), after warm-up; and PyTorch CPU fp32 doing the
            same step in the same run (the reference's libtorch path), with the
            ratio (--no-cpu skips it).  FLOPs per step: the three GEMMs (forward,
            data gradient, weight gradient) of the 2 blocks + 1 trunk convs, each
            2 x 64 B x 256 x 2304 (the stem counted as a full conv, the heads not
            at all): 1.19 TFLOP at 20 blocks, B = 128.  --compute bf16 measures the
            mixed-precision step and also gives the fraction of the 2.5 PF bf16
            MFMA peak.
            Then the refresh section (--sections picks step, refresh or both), for the
            bf16 net at 10 and 20 blocks, in one process, the three routes that bring a
            learner's weights into the engine's self-play net, alternated --reps times
            each after a warm-up (host time up to an engine sync, so the device work is
            counted):
              device   ChessNet.set_params(L): the device pack on the learner's parameters
              host     ChessNet.set_params(array): upload + the same device pack
              parent   L.params(), a fresh ChessNet (the host packer), set_net, the old
                       net closed -- what the learn loop did before the device pack
            median and spread in ms, the GB/s the device route reaches against one read
            of the parameters plus one write of the packed image, and one spai_chess.learn
            of two iterations with iteration 1's seconds by phase.  This section goes to
            --refresh-out (default profiles/chess_refresh/record.json).
            The samples section (--sections samples; not part of the default) measures the
            compact self-play samples (spai_chess.ChessSamples) against the dense arrays, in
            one process: bytes per sample over a real self-play run (64 games, 64
            simulations, 10 blocks); ms per train_batch, dense and compact alternated,
            --reps timed runs each after 3 warm-up rounds, at 10 x 32 and 20 x 128; the
            seconds of one train() over the same samples both ways; and the peak host RSS
            (ru_maxrss) of one spai_chess.learn iteration in each mode, each in a fresh
            child process.  It goes to --samples-out (default
            profiles/chess_samples/record.json).
  --learn   spai_chess.learn() at a small configuration: the loss per iteration
            (--compute f32|bf16: the train step's compute type; --samples dense|compact:
            how the samples travel from self-play to the learner).

Both merge their result into --out (default profiles/chess_learner/record.json).
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
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "self-play-ai_amd")):
    sys.path.insert(0, p)

PEAK_F32_MFMA = 157.3e12
PEAK_BF16_MFMA = 2.5e15


def step_flops(blocks, B):
    return 3 * (2 * blocks + 1) * 2 * 64 * B * 256 * 2304


def bench(args):
    import chess_learner_ref as LR
    import spai_chess as sc
    out = {}
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    batches = {B: LR.make_batches(B, 1, B)[2][0] for B in sorted({B for _, B in configs})}
    eng = sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)
    if not args.no_cpu:
        import torch
        torch.set_num_threads(args.cpu_threads)
    for blocks, B in configs:
        x, pi, z = batches[B]
        p0 = sc.init_params(blocks, 0)
        L = sc.ChessLearner(eng, blocks, p0, compute=args.compute)
        for _ in range(args.warmup):
            L.train_batch(x, pi, z)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = L.train_batch(x, pi, z)
        dev = (time.perf_counter() - t0) / args.steps
        L.close()
        assert np.isfinite(loss).all()
        fl = step_flops(blocks, B)
        r = dict(device_ms_per_step=dev * 1e3, device_samples_per_s=B / dev, step_gflop=fl / 1e9,
                 device_tflops=fl / dev / 1e12, fraction_of_f32_mfma_peak=fl / dev / PEAK_F32_MFMA)
        line = (f"{blocks}x256 B={B}: device ({args.compute}) {dev * 1e3:.2f} ms/step, {B / dev:.0f} samples/s, "
                f"{fl / dev / 1e12:.1f} TF = {fl / dev / PEAK_F32_MFMA:.3f} of the f32 MFMA peak")
        if args.compute == "bf16":
            r["fraction_of_bf16_mfma_peak"] = fl / dev / PEAK_BF16_MFMA
            line += f", {fl / dev / PEAK_BF16_MFMA:.4f} of the bf16 MFMA peak"
        if not args.no_cpu:
            forward, T, _ = LR.torch_net(p0, blocks, torch.float32)
            opt = torch.optim.Adam([t for t, _ in T if t.requires_grad], lr=1e-3)
            tx, tpi, tz = torch.tensor(x.reshape(-1, 19, 8, 8)), torch.tensor(pi), torch.tensor(z)

            def cpu_step():
                logits, v = forward(tx)
                l = -(torch.log_softmax(logits, 1) * tpi).sum() / B + ((v - tz) ** 2).mean()
                opt.zero_grad()
                l.backward()
                opt.step()

            cpu_step()
            t0 = time.perf_counter()
            for _ in range(args.cpu_steps):
                cpu_step()
            cpu = (time.perf_counter() - t0) / args.cpu_steps
            r.update(torch_cpu_ms_per_step=cpu * 1e3, torch_cpu_samples_per_s=B / cpu, device_over_cpu=cpu / dev)
            line += f"; torch CPU fp32 ({args.cpu_threads} threads) {cpu * 1e3:.0f} ms/step; ratio {cpu / dev:.1f}x"
        out[f"{blocks}x{B}"] = r
        print(line, flush=True)
    eng.close()
    rec = dict(steps=args.steps, warmup=args.warmup, compute=args.compute, peak_f32_mfma_tflops=PEAK_F32_MFMA / 1e12,
               results=out)
    if args.compute == "bf16":
        rec["peak_bf16_mfma_tflops"] = PEAK_BF16_MFMA / 1e12
    if not args.no_cpu:
        rec.update(cpu_threads=args.cpu_threads, cpu_steps=args.cpu_steps, torch=torch.__version__)
    return rec


def _spread(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return dict(n=len(a), median=float(np.median(a)), min=float(a[0]), max=float(a[-1]),
                q25=float(np.percentile(a, 25)), q75=float(np.percentile(a, 75)))


def refresh_bench(args):
    import spai_chess as sc
    out = {}
    rng = np.random.default_rng(0)
    x = (rng.random((8, 19 * 64)) < 0.3).astype(np.float32)
    pi = rng.dirichlet(np.ones(64), 8).astype(np.float32)
    pi = np.concatenate([pi, np.zeros((8, sc.POLICY - 64), np.float32)], 1)
    z = rng.choice([-1.0, 0.0, 1.0], 8).astype(np.float32)
    for blocks in (10, 20):
        eng = sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)
        p0 = sc.init_params(blocks, 0)
        eng.set_net(sc.ChessNet(eng, blocks, p0))
        L = sc.ChessLearner(eng, blocks, p0)
        L.train_batch(x, pi, z)
        P = L.params()
        sync = lambda: sc._check(sc.lib().spai_chess_sync(eng.h))   # noqa: E731

        def parent():
            old = eng.net
            eng.set_net(sc.ChessNet(eng, blocks, L.params()))
            old.close()

        routes = dict(device=lambda: eng.net.set_params(L), host=lambda: eng.net.set_params(P), parent=parent)
        times = {k: [] for k in routes}
        for rep in range(args.refresh_warmup + args.reps):
            for name, fn in routes.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                if rep >= args.refresh_warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        read_b, write_b = 4 * P.size, int(eng.net.image().size)
        L.close()
        eng.close()
        r = {k: _spread(v) for k, v in times.items()}
        gbs = (read_b + write_b) / (r["device"]["median"] * 1e-3) / 1e9
        for k, v in r.items():
            print(f"{blocks} blocks, refresh {k:>7}: median {v['median']:.3f} ms  [{v['min']:.3f}, {v['max']:.3f}]  "
                  f"n={v['n']}", flush=True)
        print(f"{blocks} blocks, device route: {read_b / 1e6:.1f} MB read + {write_b / 1e6:.1f} MB written at "
              f"{gbs:.0f} GB/s; parent / device = {r['parent']['median'] / r['device']['median']:.0f}x", flush=True)
        out[f"{blocks}x256"] = dict(refresh=r, bytes_read=read_b, bytes_written=write_b, device_gb_per_s=gbs,
                                    parent_over_device=r["parent"]["median"] / r["device"]["median"])
    cfg = dict(num_learn_iters=2, num_self_play_iters=2, num_parallel_self_play_games=8, batch_size=32, num_epochs=1,
               num_searches=16, blocks=10, seed=0)
    phases = {}

    def on_phase(i, name, secs):
        d = phases.setdefault(i, dict(refresh=0.0, self_play=0.0, train=0.0))
        d[name] += secs

    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rec = sc.learn(checkpoint_dir=d, on_phase=on_phase, **cfg)
        secs = time.perf_counter() - t0
    for r in rec:
        r["checkpoint"] = os.path.basename(r["checkpoint"])
        r["seconds"] = phases.get(r["iteration"])
    print(f"learn {cfg}: {secs:.1f} s; iteration 1 seconds {rec[1]['seconds']}", flush=True)
    return dict(net="bf16", reps=args.reps, warmup=args.refresh_warmup, unit="ms", results=out,
                learn=dict(config=cfg, refresh="device", seconds=secs, iterations=rec))


DENSE_BYTES = (19 * 64 + 4672 + 1) * 4   # a dense sample: encoding, policy row, value
RSS_CONFIG = dict(num_learn_iters=1, num_self_play_iters=8, num_parallel_self_play_games=16, batch_size=32,
                  num_epochs=1, num_searches=16, blocks=2, seed=0)


def rss_child(mode):
    """one learn iteration in this (fresh) process; prints its peak RSS"""
    import resource

    import spai_chess as sc
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rec = sc.learn(checkpoint_dir=d, samples=mode, **RSS_CONFIG)
        secs = time.perf_counter() - t0
    print(json.dumps(dict(mode=mode, ru_maxrss_kb=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss,
                          samples=rec[0]["samples"], loss=rec[0]["loss"], seconds=secs)), flush=True)


def samples_bench(args):
    import spai_chess as sc
    out = {}
    # ---- bytes per sample over a real self-play run
    G, sims, blocks = 64, 64, 10
    eng = sc.ChessEngine(num_searches=sims, max_trees=G, seed=0)
    eng.set_net(sc.ChessNet(eng, blocks, sc.init_params(blocks, 0)))
    t0 = time.perf_counter()
    games, stats = eng.self_play(G, samples="compact")
    secs = time.perf_counter() - t0
    eng.close()
    cs = sc.ChessSamples.concat(g["samples"] for g in games)
    plies = np.array([g["n"] for g in games])
    nch = cs.samples["n_children"]
    out["bytes"] = dict(games=G, num_searches=sims, blocks=blocks, self_play_seconds=secs, samples=cs.n,
                        plies_per_game=dict(min=int(plies.min()), median=float(np.median(plies)), max=int(plies.max())),
                        children_per_sample=dict(min=int(nch.min()), mean=float(nch.mean()), max=int(nch.max())),
                        dense_bytes_per_sample=DENSE_BYTES, compact_bytes_per_sample=cs.nbytes / cs.n,
                        dense_total_bytes=DENSE_BYTES * cs.n, compact_total_bytes=cs.nbytes,
                        ratio=DENSE_BYTES * cs.n / cs.nbytes)
    print(f"{cs.n} samples of {G} games ({secs:.1f} s): dense {DENSE_BYTES} B, compact {cs.nbytes / cs.n:.1f} B a "
          f"sample, {DENSE_BYTES * cs.n / cs.nbytes:.1f}x; plies {out['bytes']['plies_per_game']}, children "
          f"{out['bytes']['children_per_sample']}", flush=True)
    # ---- ms per train_batch, dense against compact, alternated
    pick = np.random.default_rng(0).permutation(cs.n)
    eng = sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)
    out["train_batch_ms"] = {}
    for blocks, B in ((10, 32), (20, 128)):
        q = cs.take(pick[:B])
        dense = q.expand()
        L = sc.ChessLearner(eng, blocks, sc.init_params(blocks, 0), compute=args.compute)
        routes = dict(dense=lambda: L.train_batch(*dense), compact=lambda: L.train_batch(q))
        times = {k: [] for k in routes}
        for rep in range(3 + args.reps):
            for name, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                if rep >= 3:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        L.close()
        r = {k: _spread(v) for k, v in times.items()}
        spread = r["dense"]["max"] - r["dense"]["min"]
        r["compact_minus_dense_median"] = r["compact"]["median"] - r["dense"]["median"]
        r["dense_spread"] = spread
        r["compact_within_dense_spread"] = bool(r["compact"]["median"] <= r["dense"]["median"] + spread)
        out["train_batch_ms"][f"{blocks}x{B}"] = r
        for k in routes:
            print(f"{blocks}x256 B={B} train_batch {k:>7}: median {r[k]['median']:.3f} ms  [{r[k]['min']:.3f}, "
                  f"{r[k]['max']:.3f}]  n={r[k]['n']}", flush=True)
        print(f"{blocks}x256 B={B}: compact - dense = {r['compact_minus_dense_median']:+.3f} ms, dense spread "
              f"{spread:.3f} ms, within: {r['compact_within_dense_spread']}", flush=True)
    # ---- one train() over the same samples, both ways
    n = min(cs.n, args.train_samples)
    q = cs.take(pick[:n])
    blocks = 10
    res = {}
    for mode in ("dense", "compact"):
        L = sc.ChessLearner(eng, blocks, sc.init_params(blocks, 0), compute=args.compute)
        t0 = time.perf_counter()
        loss = L.train(*q.expand(), epochs=1, batch=32) if mode == "dense" else L.train(q, epochs=1, batch=32)
        res[mode] = dict(seconds=time.perf_counter() - t0, loss=[float(v) for v in loss])
        L.close()
    assert res["dense"]["loss"] == res["compact"]["loss"]
    out["train_seconds"] = dict(samples=n, blocks=blocks, batch=32, epochs=1, note="dense includes expand() on the host",
                                **res)
    print(f"train over {n} samples, {blocks} blocks: dense {res['dense']['seconds']:.2f} s, compact "
          f"{res['compact']['seconds']:.2f} s", flush=True)
    eng.close()
    # ---- peak host RSS of one learn iteration, each mode in a fresh child process
    out["learn_rss"] = dict(config=RSS_CONFIG)
    for mode in ("dense", "compact"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rss-child", mode], capture_output=True,
                           text=True, check=True)
        out["learn_rss"][mode] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"learn, one iteration, {mode}: peak RSS {out['learn_rss'][mode]['ru_maxrss_kb'] / 1024:.0f} MiB, "
              f"{out['learn_rss'][mode]['samples']} samples, {out['learn_rss'][mode]['seconds']:.1f} s", flush=True)
    assert out["learn_rss"]["dense"]["loss"] == out["learn_rss"]["compact"]["loss"]
    return dict(compute=args.compute, reps=args.reps, warmup_rounds=3, unit="ms", **out)


def learn(args):
    import spai_chess as sc
    cfg = dict(num_learn_iters=args.iters, num_self_play_iters=args.self_play_iters,
               num_parallel_self_play_games=args.games, batch_size=args.batch, num_epochs=args.epochs,
               num_searches=args.sims, blocks=args.blocks, seed=args.seed, clone_self_play=not args.distinct,
               window=args.window, compute=args.compute, samples=args.samples,
               root_noise=tuple(args.root_noise) if args.root_noise else None)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rec = sc.learn(checkpoint_dir=d, **cfg)
        secs = time.perf_counter() - t0
    for r in rec:
        r["checkpoint"] = os.path.basename(r["checkpoint"])
        print("iteration %d: %d samples from %d games, loss %.4f (policy %.4f, value %.4f)"
              % (r["iteration"], r["samples"], r["games"], *r["loss"]))
    print(f"learn: {secs:.1f} s")
    return dict(config=cfg, seconds=secs, iterations=rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chess_learner", "record.json"))
    ap.add_argument("--refresh-out", default=os.path.join(REPO, "profiles", "chess_refresh", "record.json"))
    ap.add_argument("--sections", default="step,refresh",
                    help="--bench: step, refresh, samples or several, comma separated")
    ap.add_argument("--samples-out", default=os.path.join(REPO, "profiles", "chess_samples", "record.json"))
    ap.add_argument("--train-samples", type=int, default=2048, help="--bench samples: samples of the timed train()")
    ap.add_argument("--samples", choices=("dense", "compact"), default="dense",
                    help="--learn: how the samples reach the learner")
    ap.add_argument("--rss-child", choices=("dense", "compact"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=20, help="--bench refresh: timed refreshes per route (at least 20)")
    ap.add_argument("--refresh-warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--tag", default="", help="record under bench_<tag> / learn_<tag>")
    ap.add_argument("--configs", default="10x32,10x128,20x32,20x128", help="--bench: blocks x B, comma separated")
    ap.add_argument("--compute", choices=("f32", "bf16"), default="f32", help="the train step's compute type")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="--bench: skip the PyTorch CPU step")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--games", type=int, default=8)
    ap.add_argument("--self-play-iters", type=int, default=2)
    ap.add_argument("--distinct", action="store_true", help="clone_self_play=False")
    ap.add_argument("--window", type=int, default=None, help="--learn: self-play through this many tree slots")
    ap.add_argument("--root-noise", type=float, nargs=2, metavar=("ALPHA", "EPS"), default=None,
                    help="--learn: Dirichlet noise at the self-play roots (default: off, the reference's search)")
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.rss_child:
        return rss_child(args.rss_child)
    if not (args.bench or args.learn):
        ap.error("give --bench and/or --learn")
    sections = set(args.sections.split(","))
    if not sections or sections - {"step", "refresh", "samples"}:
        ap.error("--sections: step, refresh, samples")
    if args.bench and sections & {"refresh", "samples"} and args.reps < 20:
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
    sfx = "_" + args.tag if args.tag else ""
    if args.bench and "refresh" in sections:
        os.makedirs(os.path.dirname(os.path.abspath(args.refresh_out)), exist_ok=True)
        with open(args.refresh_out, "w") as f:
            json.dump(dict(commit=commit, bench=refresh_bench(args)), f, indent=1)
            f.write("\n")
    if args.bench and "samples" in sections:
        os.makedirs(os.path.dirname(os.path.abspath(args.samples_out)), exist_ok=True)
        rec = dict(commit=commit, bench=samples_bench(args))
        with open(args.samples_out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    if args.bench and "step" in sections:
        record["bench" + sfx] = bench(args)
    if args.learn:
        record["learn" + sfx] = learn(args)
    if args.learn or (args.bench and "step" in sections):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
