"""The evaluation cache's own counters at the benchmark's scale: one warm-up step,
then one self_play of FS_STEPS (20) x 4,096 games streamed through 4,096 slots
(800 sims, 6x64), and spai_eval_cache_get_stats over that call -> one JSON line.
SPAI_LIB chooses the library, SPAI_EVAL_CACHE the capacity (profiles/eval_cache_two_choice);
SPAI_EVAL_CACHE_THIN_LOG=1 adds one line per thinning on stderr: the classes' sizes and
what was kept of each (profiles/eval_cache_thin).

  python3 scripts/eval_cache_fullstats.py
"""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "self-play-ai_amd"))
import spai
G, STEPS = 4096, int(os.environ.get("FS_STEPS", "20"))
e = spai.Engine(num_searches=800, max_trees=G, eval_kind=spai.EVAL_NET, seed=0)
e.set_net(spai.Net(e, 6, spai.init_params(6, 64, seed=0)))
e.self_play(G, collect=False, window=G)   # warm-up (the table keeps what it learnt, as in the bench)
c0 = e.eval_cache_stats()
t0 = time.perf_counter()
_, st = e.self_play(STEPS * G, game_id_base=G, collect=False, window=G)
dt = time.perf_counter() - t0
c1 = e.eval_cache_stats()
d = {k: (c1[k] if k in ("capacity", "live", "kept_hit") else c1[k] - c0[k]) for k in c1}   # states, else totals
d["hit_rate"] = d["hits"] / d["lookups"]
d["drop_share_of_attempts"] = d["dropped"] / (d["inserts"] + d["dropped"])
d["sims_per_sec"] = st["sims"] / dt
d["build"] = os.path.basename(os.environ.get("SPAI_LIB", "libspai.so"))
d["SPAI_EVAL_CACHE"] = os.environ.get("SPAI_EVAL_CACHE", "")
print(json.dumps(d))
e.close()
