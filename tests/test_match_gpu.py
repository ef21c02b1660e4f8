"""Engine.match / spai_match_run on the device against the CPU restatement
(tests/match_ref.py, pinned by test_match_ref_cpu.py): move lists, results and the
per-player simulation and evaluation counts, to the bit.

Shapes.  Stub evaluators: 1, 2, 5 and 72 games (72: 36 trees per chain, 4.5 blocks
of 8), openings of 0, 1 and 6 plies, simulations (A, B) of (1, 1), (16, 16) and
(8, 24).  fp32 nets: 1 block x 64, 4 games, 8 simulations, 2 opening plies, games
of 12-15 plies played to the end; measured, the whole net-against-net case
(device and restatement) takes 0.85 s on the MI355X host and the case against
UNIFORM 0.22 s, well inside the 10 s the restatement's side may take.
Cache: two bf16 nets of 2 x 64, 64 games (128 trees), 32 simulations.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NAN = -1, -5


@pytest.fixture(scope="module")
def spai():
    import spai as s
    s.lib()
    return s


@pytest.fixture(scope="module")
def ref(oracle):
    import match_ref
    return match_ref


@pytest.fixture(scope="module")
def stub_engine(spai):
    e = spai.Engine(num_searches=24, max_trees=144, eval_kind=spai.EVAL_HASH)
    yield e
    e.close()


def _same(dev, exp):
    (dg, ds), (eg, es) = dev, exp
    assert dg == eg
    for k in ("a_wins", "draws", "b_wins", "sims", "evals"):
        assert ds[k] == es[k], k


# (games, opening plies, A's simulations, B's, A = UNIFORM and B = HASH instead, first game id)
STUB_CASES = [
    (1, 0, 16, 16, False, 0),
    (1, 1, 16, 16, True, 0),
    (2, 0, 8, 24, False, 0),
    (2, 6, 16, 16, True, 0),
    (5, 1, 8, 24, False, 0),
    (5, 1, 8, 24, True, 0),
    (5, 6, 16, 16, False, 3),
    (72, 1, 16, 16, False, 0),
    (72, 6, 8, 24, True, 0),
    (72, 0, 24, 8, True, 10),
]


@pytest.mark.parametrize("n,plies,sa,sb,swap,base", STUB_CASES)
def test_stub_players_bit_exact(spai, oracle, ref, stub_engine, n, plies, sa, sb, swap, base):
    ka, kb = (spai.EVAL_UNIFORM, spai.EVAL_HASH) if swap else (spai.EVAL_HASH, spai.EVAL_UNIFORM)
    dev = stub_engine.match((ka, None, sa), (kb, None, sb), n, opening_plies=plies, seed=11, game_id_base=base)
    exp = ref.play_match((ka, None, sa), (kb, None, sb), n, plies, seed=11, game_id_base=base)
    _same(dev, exp)
    assert sum(len(g["moves"]) for g in dev[0]) >= 7 * n


def _selfplay_stub(e, n):
    games, stats = e.self_play(n)
    return ([(g["game"], g["moves"].tolist(), g["policy"].tobytes(), g["value"].tobytes()) for g in games],
            stats["sims"], stats["evals"])


def test_match_neither_samples_nor_disturbs_the_timers(spai, oracle, ref):
    """self-play's search calls and a match's share one launcher; only the former sample
    the engine's timers.  HASH against UNIFORM, 5 games, simulations (8, 24), 1 opening ply."""
    a, b = (spai.EVAL_HASH, None, 8), (spai.EVAL_UNIFORM, None, 24)
    engines = [spai.Engine(num_searches=24, max_trees=144, eval_kind=spai.EVAL_HASH) for _ in range(2)]
    for e in engines:
        e.set_timing(True, stride=1)
    e, fresh = engines
    before = {k: v["launches"] for k, v in e.timing().items()}
    _same(e.match(a, b, 5, opening_plies=1, seed=11), ref.play_match(a, b, 5, 1, seed=11))
    assert {k: v["launches"] for k, v in e.timing().items()} == before
    after = _selfplay_stub(e, 5)
    assert e.timing()["evaluate"]["launches"] > 0
    assert after == _selfplay_stub(fresh, 5)
    for e in engines:
        e.close()


def test_unequal_and_empty_chains(spai, oracle, ref, stub_engine):
    """one game, simulations (24, 8), no opening: every ply has one chain without trees and
    the other alternates between 24 and 8 iterations; then 72 games at (8, 24), both chains
    full, on the same engine"""
    h, u = spai.EVAL_HASH, spai.EVAL_UNIFORM
    for n, sa, sb in ((1, 24, 8), (72, 8, 24)):
        _same(stub_engine.match((h, None, sa), (u, None, sb), n, opening_plies=0, seed=11),
              ref.play_match((h, None, sa), (u, None, sb), n, 0, seed=11))


@pytest.mark.parametrize("n", [1, 5])
def test_one_simulation_is_err_nan_on_both_sides(spai, oracle, ref, stub_engine, n):
    """simulations (1, 1): the only simulation expands the root and visits no child, so
    there is no move to play: SPAI_ERR_NAN here, MatchNaN in the restatement"""
    a, b = (spai.EVAL_HASH, None, 1), (spai.EVAL_UNIFORM, None, 1)
    with pytest.raises(ref.MatchNaN):
        ref.play_match(a, b, n, 1, seed=11)
    with pytest.raises(spai.SpaiError) as ei:
        stub_engine.match(a, b, n, opening_plies=1, seed=11)
    assert ei.value.code == ERR_NAN
    # the engine goes on
    _same(stub_engine.match((spai.EVAL_HASH, None, 16), b[:2] + (16,), n, opening_plies=1, seed=11),
          ref.play_match((spai.EVAL_HASH, None, 16), b[:2] + (16,), n, 1, seed=11))


@pytest.mark.parametrize("vs_uniform", [False, True])
def test_f32_nets_bit_exact(spai, oracle, ref, vs_uniform):
    """two fp32 nets (seeds 1 and 2), and a net against UNIFORM: 1 x 64, 4 games, 8 simulations"""
    blocks, n, sims, plies = 1, 4, 8, 2
    p1, p2 = spai.init_params(blocks, 64, seed=1), spai.init_params(blocks, 64, seed=2)
    e = spai.Engine(num_searches=sims, max_trees=2 * n, eval_kind=spai.EVAL_UNIFORM)
    d1, d2 = spai.Net(e, blocks, p1, dtype=spai.DTYPE_F32), spai.Net(e, blocks, p2, dtype=spai.DTYPE_F32)
    o1, o2 = (oracle.Net(oracle.GAME_CONNECT4, blocks, 64, p) for p in (p1, p2))
    if vs_uniform:
        dev = e.match((spai.EVAL_NET, d1, sims), (spai.EVAL_UNIFORM, None, sims), n, opening_plies=plies, seed=3)
        exp = ref.play_match((oracle.EVAL_NET, o1, sims), (oracle.EVAL_UNIFORM, None, sims), n, plies, seed=3)
    else:
        dev = e.match((spai.EVAL_NET, d1, sims), (spai.EVAL_NET, d2, sims), n, opening_plies=plies, seed=3)
        exp = ref.play_match((oracle.EVAL_NET, o1, sims), (oracle.EVAL_NET, o2, sims), n, plies, seed=3)
    _same(dev, exp)
    d1.close()
    d2.close()
    e.close()


def _strip(result):
    games, stats = result
    return games, {k: v for k, v in stats.items() if k != "seconds"}


def _selfplay(spai, params, blocks, e=None):
    own = e is None
    if own:
        e = spai.Engine(num_searches=32, max_trees=128, eval_kind=spai.EVAL_NET, seed=7)
    net = spai.Net(e, blocks, params)
    e.set_net(net)
    games, stats = e.self_play(16)
    out = [(g["game"], g["moves"].tolist(), g["policy"].tobytes(), g["value"].tobytes()) for g in games]
    e.set_net(None)
    net.close()
    if own:
        e.close()
    return out, (stats["sims"], stats["evals"], stats["positions"])


def test_cache_on_off_one_bucket_and_selfplay_after(spai):
    blocks, n, sims = 2, 64, 32
    pa, pb = spai.init_params(blocks, 64, seed=1), spai.init_params(blocks, 64, seed=2)
    e = spai.Engine(num_searches=sims, max_trees=2 * n, eval_kind=spai.EVAL_NET, seed=7)
    na, nb = spai.Net(e, blocks, pa), spai.Net(e, blocks, pb)
    a, b = (spai.EVAL_NET, na, sims), (spai.EVAL_NET, nb, sims)
    s0 = e.eval_cache_stats()
    default = _strip(e.match(a, b, n, opening_plies=4, seed=5))
    s1 = e.eval_cache_stats()
    assert s1["capacity"] > 8
    assert s1["lookups"] - s0["lookups"] == sum(default[1]["evals"]) > 0
    assert s1["hits"] - s0["hits"] > 0
    e.set_eval_cache(0)
    off = _strip(e.match(a, b, n, opening_plies=4, seed=5))
    s2 = e.eval_cache_stats()
    assert s2["capacity"] == 0 and s2["lookups"] == s1["lookups"]
    e.set_eval_cache(8)
    one = _strip(e.match(a, b, n, opening_plies=4, seed=5))
    s3 = e.eval_cache_stats()
    assert s3["capacity"] == 8 and s3["lookups"] - s2["lookups"] == sum(default[1]["evals"])
    assert default == off == one
    # the players are different: a net mix-up between the chains would show here
    swapped = _strip(e.match(b, a, n, opening_plies=4, seed=5))
    assert swapped[0] != default[0]
    # a later self-play call on this engine sees none of the matches' entries
    e.set_eval_cache(1 << 16)
    e.match(a, b, n, opening_plies=4, seed=5)
    assert _selfplay(spai, pb, blocks, e) == _selfplay(spai, pb, blocks)
    na.close()
    nb.close()
    e.close()


def test_identical_players_mirror_and_replay(spai, oracle):
    blocks, n, sims = 2, 8, 16
    e = spai.Engine(num_searches=sims, max_trees=2 * n, eval_kind=spai.EVAL_UNIFORM)
    net = spai.Net(e, blocks, spai.init_params(blocks, 64, seed=4))
    pl = (spai.EVAL_NET, net, sims)
    games, stats = e.match(pl, pl, n, opening_plies=4, seed=2)
    for p in range(n // 2):
        g0, g1 = games[2 * p], games[2 * p + 1]
        assert g0["moves"] == g1["moves"] and g0["result_a"] == -g1["result_a"]
    assert sum(g["result_a"] for g in games) == 0
    assert stats["sims"][0] == stats["sims"][1] and stats["evals"][0] == stats["evals"][1]
    acts = np.full((n, 42), -1, np.int32)
    for i, g in enumerate(games):
        acts[i, :len(g["moves"])] = g["moves"]
    rep = oracle.c4_replay(acts)
    for i, g in enumerate(games):
        m = len(g["moves"])
        assert (rep["rc"][i, :m] == 0).all() and (rep["status"][i, :m] == oracle.ONGOING).all()
        last_mover_is_a = ((g["game"] ^ (m - 1)) & 1) == 0
        won = rep["status"][i, m] == oracle.WON
        assert rep["status"][i, m] in (oracle.WON, oracle.TIED)
        assert g["result_a"] == ((1 if last_mover_is_a else -1) if won else 0)
    net.close()
    e.close()


def test_validation_and_engine_usable_after(spai, oracle, ref):
    e = spai.Engine(num_searches=16, max_trees=8, eval_kind=spai.EVAL_HASH)
    h, u = (spai.EVAL_HASH, None, 16), (spai.EVAL_UNIFORM, None, 16)
    bad = [
        dict(a=h, b=u, n_games=2, opening_plies=7),
        dict(a=h, b=u, n_games=5, opening_plies=2),                          # 10 trees > max_trees
        dict(a=(spai.EVAL_HASH, None, 0), b=u, n_games=2, opening_plies=2),
        dict(a=h, b=(spai.EVAL_UNIFORM, None, 17), n_games=2, opening_plies=2),
        dict(a=(spai.EVAL_NET, None, 16), b=u, n_games=2, opening_plies=2),
    ]
    for kw in bad:
        with pytest.raises(spai.SpaiError) as ei:
            e.match(**kw)
        assert ei.value.code == ERR_INVALID, kw
        _same(e.match(h, u, 4, opening_plies=2, seed=1), ref.play_match(h, u, 4, 2, seed=1))
    # a search and a self-play call after a match equal those of a fresh engine
    fresh = spai.Engine(num_searches=16, max_trees=8, eval_kind=spai.EVAL_HASH)
    outs = []
    for eng in (e, fresh):
        eng.trees_create(4)
        pol, _ids, vis, nc = eng.search([0, 1, 2, 3], 16)
        games, st = eng.self_play(8)
        outs.append((pol.tobytes(), vis.tobytes(), nc.tobytes(),
                     [(g["game"], g["moves"].tolist(), g["policy"].tobytes()) for g in games], st["sims"], st["evals"]))
    assert outs[0] == outs[1]
    fresh.close()
    e.close()
