"""bench.py's entry point on the CPU (no GPU, no library calls): how `--gpus N`
becomes N rank processes (the worker fan-out of main.rs:169-186,220-234 as one
process per GPU).

* `--gpus 1` without a launcher runs in-process (no spawn);
* `--gpus N` without a launcher spawns N ranks with RANK = LOCAL_RANK = r,
  WORLD_SIZE = N and MASTER_* on 127.0.0.1, the parent never importing spai;
* under a launcher WORLD_SIZE must equal --gpus;
* a rank that fails stops the others (a rank blocked in the host group's
  barrier would otherwise wait forever) and the parent exits non-zero.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import REPO


class _Reached(Exception):
    pass


def _bench(monkeypatch, argv, env):
    sys.path.insert(0, REPO)
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    calls = []

    def fake_spawn(n):
        calls.append(n)
        return 0

    def fake_dist():
        raise _Reached()

    monkeypatch.setattr(bench, "spawn_ranks", fake_spawn)
    monkeypatch.setattr(bench, "Dist", fake_dist)
    return bench, calls


def test_gpus_one_runs_in_process(monkeypatch):
    bench, calls = _bench(monkeypatch, ["--gpus", "1"], {})
    with pytest.raises(_Reached):
        bench.main()
    assert calls == []


def test_gpus_n_spawns_ranks(monkeypatch):
    bench, calls = _bench(monkeypatch, ["--gpus", "4", "--steps", "1"], {})
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert calls == [4] and ex.value.code == 0


def test_launcher_world_must_match(monkeypatch):
    bench, calls = _bench(monkeypatch, ["--gpus", "2"], {"WORLD_SIZE": "3", "RANK": "0"})
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert calls == [] and "WORLD_SIZE=3" in str(ex.value.code)
    bench, calls = _bench(monkeypatch, ["--gpus", "2"], {"WORLD_SIZE": "2", "RANK": "0"})
    with pytest.raises(_Reached):   # a matching launcher world runs the rank in-process
        bench.main()
    assert calls == []


def test_spawned_ranks_env_and_failure(tmp_path):
    """the real spawn with a stand-in rank program: every rank sees its env; one
    rank failing stops a rank that would block forever, and the parent reports it"""
    sys.path.insert(0, REPO)
    import bench
    prog = tmp_path / "rank.py"
    prog.write_text(
        "import json, os, sys, time\n"
        "keys = ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'SPAI_GROUP_PORT')\n"
        "open(os.path.join(%r, 'r%%s.json' %% os.environ['RANK']), 'w').write(json.dumps({k: os.environ[k] for k in keys}))\n"
        "if os.environ['RANK'] == '1' and 'FAIL' in sys.argv: sys.exit(3)\n"
        "if os.environ['RANK'] == '0' and 'FAIL' in sys.argv: time.sleep(600)\n" % str(tmp_path))
    old_file, old_argv = bench.__file__, sys.argv
    try:
        bench.__file__ = str(prog)
        sys.argv = ["bench.py", "--gpus", "3"]
        assert bench.spawn_ranks(3) == 0
        envs = [json.loads((tmp_path / ("r%d.json" % r)).read_text()) for r in range(3)]
        for r, e in enumerate(envs):
            assert e["RANK"] == e["LOCAL_RANK"] == str(r) and e["WORLD_SIZE"] == "3"
            assert e["MASTER_ADDR"] == "127.0.0.1"
        assert len({e["MASTER_PORT"] for e in envs}) == 1 and len({e["SPAI_GROUP_PORT"] for e in envs}) == 1
        sys.argv = ["bench.py", "--gpus", "2", "FAIL"]
        t0 = time.time()
        assert bench.spawn_ranks(2) == 3
        assert time.time() - t0 < 60
    finally:
        bench.__file__, sys.argv = old_file, old_argv


def test_parent_does_not_load_the_library(tmp_path):
    """`python bench.py --gpus 2` as a process: its ranks fail here (no GPU), the
    parent exits non-zero without having imported spai (checked by a stand-in
    SPAI_LIB that does not exist: only a rank would try to load it)"""
    env = dict(os.environ, SPAI_LIB=str(tmp_path / "absent.so"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "rank exit status" in p.stderr
    assert "not built" in p.stderr   # the ranks, not the parent, reached the library


def test_schedule_flags_parse(monkeypatch):
    """the streamed schedule is the default; --lockstep selects one lockstep batch
    per step; --stream (the round-5 A/B flag) still parses"""
    sys.path.insert(0, REPO)
    import bench
    for argv, lock in (([], False), (["--lockstep"], True), (["--stream"], False)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        a = bench.parse()
        assert a.lockstep is lock and not a.no_lockstep_ref


def test_full_and_dump_flags_parse(monkeypatch):
    """a plain run measures the headline only: --full (off by default) turns the other
    measurements on, their --no-* switches still parse, --dump-outputs takes a directory"""
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-chess", "--no-cpu-baseline", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.no_chess and a.no_cpu_baseline and a.dump_outputs == "d"


def test_dump_sample_and_files(tmp_path):
    """--dump-outputs: the kept ids are a fixed function of the arguments (all of a small
    step, a seeded DUMP_GAMES-subset of a large one, inside the step's id range), and the
    files hold the kept games in id order whatever order they finished in, as float32 /
    float64"""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    assert bench.dump_ids(192, 96, 0) == frozenset(range(192, 288))
    big = bench.dump_ids(8192, 4096, 0)
    assert big == bench.dump_ids(8192, 4096, 0) and len(big) == bench.DUMP_GAMES
    assert min(big) >= 8192 and max(big) < 8192 + 4096 and big != bench.dump_ids(8192, 4096, 1)
    # the whole dump stays far below 64 MB at the longest possible games
    assert bench.DUMP_GAMES * 42 * (126 + 7 + 1 + 1) * 4 < 64e6

    def game(gid, n):
        return dict(game=gid, enc=np.full((n, 126), gid, np.float32), policy=np.full((n, 7), gid, np.float32),
                    value=np.full(n, gid, np.float32), moves=np.full(n, gid, np.int32))

    counters = dict(sims=5.0, evals=4.0, games=2.0, positions=5.0, moves=3.0)
    bench.dump_outputs(str(tmp_path / "a"), [game(7, 3), game(5, 2)], counters)
    bench.dump_outputs(str(tmp_path / "b"), [game(5, 2), game(7, 3)], counters)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("game_id", "positions", "enc", "policy", "value", "moves", "counters"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert list(np.load(tmp_path / "a" / "game_id.npy")) == [5, 7]
    assert list(np.load(tmp_path / "a" / "positions.npy")) == [2, 3]
    assert list(np.load(tmp_path / "a" / "value.npy")) == [5, 5, 7, 7, 7]
    assert np.load(tmp_path / "a" / "enc.npy").shape == (5, 126)
    assert list(np.load(tmp_path / "a" / "counters.npy")) == [5, 4, 2, 5]


@pytest.mark.parametrize("world", [1, 2, 8])
def test_stream_game_ids_partition(world):
    """the streamed bench's game ids: the ranks' ranges tile the job's range with no
    overlap, the warm-up stream's ids are disjoint from the timed region's, and at
    world 1 the stream plays the lockstep steps' ids (step i: [i G, (i + 1) G))"""
    sys.path.insert(0, REPO)
    import bench
    G, k, w = 96, 3, 2

    def ids(first, steps):
        out = []
        for r in range(world):
            b = bench.stream_base(first, steps, world, r, G)
            out.extend(range(b, b + steps * G))
        return out

    timed, warm = ids(0, k), ids(-w, w)
    assert sorted(timed) == list(range(0, k * world * G))
    assert sorted(warm) == list(range(-w * world * G, 0))
    if world == 1:
        assert timed == [g for i in range(k) for g in range(i * G, (i + 1) * G)]


_RCCL_FAIL = r"""
import sys
sys.path.insert(0, {repo!r})
import bench

class G:
    def allgather(self, x):
        return [0, 1] if isinstance(x, int) else [x, x]
    def broadcast_bytes(self, b):
        return b or bytes(128)

class D:
    world, rank, local = {world}, 0, 0
    g = G()

class S:
    @staticmethod
    def comm_unique_id():
        return bytes(128)
    class Comm:
        def __init__(self, *a):
            raise RuntimeError("ncclCommInitRank failed (simulated)")

comm, note = bench.rccl_comm(D(), S)
print("returned", comm, note)
"""


@pytest.mark.parametrize("world", [1, 2])
def test_rccl_failure_is_agreed_and_reported(tmp_path, world):
    """an RCCL communicator failure on a rank must not leave its peers
    blocked in a collective.  spai_comm_create waits with a bound (a failed or absent
    peer returns an error), the ranks then agree over the host group, and without a
    communicator on every rank none uses one: the line reports it and the run goes on
    (the host group carries the reductions)"""
    p = subprocess.run([sys.executable, "-c", _RCCL_FAIL.format(repo=REPO, world=world)], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert "returned None RCCL communicator failed (rank 0: RuntimeError('ncclCommInitRank failed (simulated)')" \
        in p.stdout and "host group only" in p.stdout, p.stdout
