"""The Connect4 search with the bf16 net -- the path bench.py times: k_forward
launched through net_eval_batch with a device-side leaf count, two search chains,
the group-size policy, tail mode and the evaluation cache -- against the CPU
oracle's Mcts::search, self-play and match with Net.predict of the same
parameters on the device behind the oracle's callback (tests/c4_search_ref.py,
pinned by tests/test_c4_search_ref_cpu.py).  Predict and the search's evaluation
launch the same kernel and predict's output does not depend on the batch
(test_net_group_size_invariance), so the oracle must reproduce the device search
bit for bit: every comparison here is ==, on visit counts, policies and the root
children's N, W and P records (Engine.tree_child_stats).  The CPU file shows why
the records: last-bit differences of the priors move no visit count.

Nets: 2 x 64 from init_params (seed 7), and for one deep search 6 x 64 from
bf16_ref.trained_like parameters (non-identity batch norms).  Roots:
c4_search_ref.positions(trees, seed = trees, a tenth of them duplicates).

Group sizes and rounds assume the MI355X's 256 CUs:
  trees  chains  leaves per launch  regime
    100  one     100                S = 1
    200  two     100 each           two chains below SPAI_CONC_MIN_COUNT, S = 1
    700  two     350 each           S = 2
  1,300  two     650 each           the two-chain policy chooses S from 3 upward
  4,100  two     2,050 each         two rounds per launch, a partial last group
The deep searches run with the cache off, so the forwarded leaves are the trees'
(each compares the device's count of forwarded leaves with the oracle's
evaluations).  No process-wide knob is set."""
import os
import time

import numpy as np
import pytest

import c4_search_ref as R

pytestmark = pytest.mark.gpu

NETS = {"2x64": 2, "2x64b": 2, "6x64-trained": 6}


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def net_params(spai, name):
    if name == "2x64":
        return spai.init_params(2, 64, seed=7)
    if name == "2x64b":
        return spai.init_params(2, 64, seed=8)
    import bf16_ref
    return bf16_ref.trained_like(spai.init_params(6, 64, seed=56), bf16_ref.c4_layout(6), 66)


@pytest.fixture(scope="module")
def yard(spai):
    """name -> (params, Evaluator over Net.predict of those parameters on an engine of
    its own, shared by every test: a position costs one forward in the whole module)"""
    made = {}

    def get(name):
        if name not in made:
            params = net_params(spai, name)
            e = spai.Engine(num_searches=1, max_trees=1)
            net = spai.Net(e, NETS[name], params)
            made[name] = (params, R.Evaluator(net.predict), e, net)
        return made[name][:2]

    yield get
    for _, _, e, net in made.values():
        net.close()
        e.close()


def engine(spai, name, params, trees, sims, cache=None, seed=0):
    e = spai.Engine(num_searches=sims, max_trees=trees, eval_kind=spai.EVAL_NET, seed=seed)
    if cache is not None:
        e.set_eval_cache(cache)
    e.set_net(spai.Net(e, NETS[name], params))   # closed with the engine
    return e


def load(e, roots, trees=None):
    e.trees_create(len(roots) if trees is None else trees)
    for t, s in enumerate(roots):
        e.tree_reset(t, R.key_of(s) + (0,))


def compare(e, rs, dev, ref, trees, root_ids, what):
    """the device's search result over `trees` (in that order) and those trees' records
    against the oracle's (search result indexed by tree); root_ids: the device's root node"""
    pol, ids, vis, nc = dev
    bad = {}

    def note(kind, t):
        bad.setdefault(kind, []).append(int(t))

    for i, t in enumerate(trees):
        k = int(ref["nc"][t])
        if int(nc[i]) != k:
            note("n_children", t)
            continue
        if not R.same_bits(vis[i], ref["visits"][t]):
            note("visits", t)
        if not R.same_bits(pol[i], ref["policy"][t]):
            note("policy", t)
        cid, cn, cw, cp = e.tree_child_stats(t)
        _, rn, rw, rp = rs.children(t)
        if not np.array_equal(cid, ids[i, :k]):
            note("child ids", t)
        if not R.same_bits(cn, rn):
            note("child N", t)
        if not R.same_bits(cw, rw):
            note("child W", t)
        if not R.same_bits(cp, rp):
            note("child P", t)
        _, n_root, w_root = e.tree_node(t, root_ids[t])
        rn_root, rw_root = rs.root(t)
        if n_root != rn_root:
            note("root N", t)
        if not R.same_bits(np.float32(w_root), rw_root):
            note("root W", t)
    report = {k: (len(v), v[:8]) for k, v in bad.items()}
    assert not bad, "%s: trees that differ from the oracle (count, first ones): %s" % (what, report)


# ---------------------------------------------------------------- A: one simulation
def test_one_simulation(spai, yard):
    n = 100
    params, ev = yard("2x64")
    roots = R.positions(n, n, duplicates=n // 10)
    keys = [R.key_of(s) for s in roots]
    e = engine(spai, "2x64", params, n, 1, cache=0)
    load(e, roots)
    # the engine's own net and the yardstick's give the same bytes
    own_p, own_v = e.net.predict([k + (0,) for k in keys])
    for t, k in enumerate(keys):
        p, v = ev.entry(k)
        assert R.same_bits(own_p[t], p) and R.same_bits(own_v[t], v), t
    # unexpanded: no children, and reading changes nothing
    for t in (0, 1, n - 1):
        for _ in range(2):
            assert all(len(a) == 0 for a in e.tree_child_stats(t))
            assert e.tree_node(t, 0)[1:] == (0, 0.0)
    with pytest.raises(spai.SpaiError):
        e.tree_child_stats(n)
    order = np.random.default_rng(1).permutation(n).astype(np.uint32)   # batch slot != tree
    assert (order != np.arange(n)).sum() > n // 2
    dev = e.search(order, 1)
    rs = R.RefSearch(roots, ev)
    ref = rs.search(1)
    for i, t in enumerate(order):
        cols = roots[t].valid_actions()
        cid, cn, cw, cp = e.tree_child_stats(t)
        assert len(cid) == len(cols) == int(dev[3][i]), t
        assert R.same_bits(cp, own_p[t][cols]), (t, cp, own_p[t][cols])   # predict's priors at the legal columns
        assert not cn.any() and not cw.any(), t
        assert list(cid) == list(range(int(cid[0]), int(cid[0]) + len(cols))), t
        _, n_root, w_root = e.tree_node(t, 0)
        assert n_root == 1 and R.same_bits(np.float32(w_root), own_v[t]), (t, w_root, own_v[t])
        again = e.tree_child_stats(t)
        assert all(R.same_bits(a, b) for a, b in zip(again, (cid, cn, cw, cp))), t
    compare(e, rs, dev, ref, order, [0] * n, "one simulation")
    rs.close()
    e.close()


# ---------------------------------------------------------------- B: deep searches, cache off
DEEP = [(100, 48, "2x64", 1), (200, 32, "2x64", 2), (700, 32, "6x64-trained", 2), (1300, 24, "2x64", 2),
        (4100, 24, "2x64", 2)]


@pytest.mark.parametrize("trees,sims,name,chains", DEEP)
def test_deep_search_cache_off(spai, yard, trees, sims, name, chains):
    params, ev = yard(name)
    roots = R.positions(trees, trees, duplicates=trees // 10)
    e = engine(spai, name, params, trees, sims, cache=0)
    load(e, roots)
    e.set_timing(True, stride=1)   # counts the leaves of every forward launch
    order = np.arange(trees, dtype=np.uint32)
    dev = e.search(order, sims)
    tm = e.timing()["evaluate"]
    cs = e.eval_cache_stats()
    rs = R.RefSearch(roots, ev)
    ref = rs.search(sims)
    print("%d trees x %d simulations, %s: %d leaves forwarded in %d launches (oracle: %d evaluations, %d distinct "
          "positions in the memo)" % (trees, sims, name, tm["items"], tm["launches"], ref["evals"], len(ev.index)))
    assert cs["capacity"] == 0 and cs["hits"] == 0
    assert tm["items"] == ref["evals"] < trees * sims   # terminal leaves occurred
    assert tm["launches"] == chains * sims
    compare(e, rs, dev, ref, order, [0] * trees, "%d trees" % trees)
    rs.close()
    e.close()


def test_one_ulp_in_the_yardstick_would_show(spai, yard):
    """the control of the comparisons above: the 100-tree search against an oracle whose
    predict carries one float32 ulp of noise on the priors (c4_search_ref.Fault).  Every
    tree whose root entry the noise changed differs in its root children's P bits, so a
    forward whose last bits depended on the launch would fail the tests of this file;
    the visit counts alone would let it pass in the trees counted here."""
    trees, sims, name = 100, 24, "2x64"
    params, ev = yard(name)
    roots = R.positions(trees, trees, duplicates=trees // 10)
    e = engine(spai, name, params, trees, sims, cache=0)
    load(e, roots)
    vis = e.search(np.arange(trees, dtype=np.uint32), sims)[2]
    fault = R.Fault(ev.predict, R.Fault.ULP_NOISE, seed=1, amp=1)
    rs = R.RefSearch(roots, R.Evaluator(fault))
    ref = rs.search(sims)
    noised = [t for t, s in enumerate(roots) if R.key_of(s) in fault.changed]
    p_differs = [t for t in range(trees) if not R.same_bits(e.tree_child_stats(t)[3], rs.children(t)[3])]
    same_visits = [t for t in range(trees) if R.same_bits(vis[t], ref["visits"][t])]
    print("one ulp of noise behind the oracle: root entry changed in %d of %d trees, root-child P bits differ in %d, "
          "visit counts still equal in %d" % (len(noised), trees, len(p_differs), len(same_visits)))
    assert len(noised) >= trees // 2 and set(noised) <= set(p_differs)
    rs.close()
    e.close()


# ---------------------------------------------------------------- C: the cache
def test_cache_capacities(spai, yard):
    """700 trees with 70 duplicate roots, 32 simulations, at the default capacity, at 8
    entries (one bucket) and at 0: the oracle's records each time.  With the default
    capacity the big call hits.  One bucket is full after the first iteration with
    positions that need not come again, so a hit is shown where it must happen: two more
    trees with one root, never searched before, the first for 6 simulations (at most 6
    entries, the root's among them; no clear, 6 is not above 3/4 of 8), then the second,
    whose first leaf is that root.  Those two calls are compared with the oracle too."""
    trees, sims, name = 700, 32, "2x64"
    params, ev = yard(name)
    roots = R.positions(trees, trees, duplicates=trees // 10)
    assert len({R.key_of(s) for s in roots}) == trees - trees // 10
    extra = R.positions(40, 5)[-1]
    all_roots = roots + [extra, extra]
    rs = R.RefSearch(all_roots, ev)
    order = np.arange(trees, dtype=np.uint32)
    big = orc_search(rs, range(trees), sims)
    big_records = [(rs.children(t), rs.root(t)) for t in range(trees)]
    small = [orc_search(rs, [trees], 6), orc_search(rs, [trees + 1], sims)]
    for cap in (None, 8, 0):
        e = engine(spai, name, params, trees + 2, sims, cache=cap)
        load(e, all_roots)
        dev = e.search(order, sims)
        c1 = e.eval_cache_stats()
        bad = []
        for t in range(trees):
            (_, rn, rw, rp), (n_root, w_root) = big_records[t]
            cid, cn, cw, cp = e.tree_child_stats(t)
            node = e.tree_node(t, 0)
            ok = (R.same_bits(cn, rn) and R.same_bits(cw, rw) and R.same_bits(cp, rp) and node[1] == n_root and
                  R.same_bits(np.float32(node[2]), w_root) and R.same_bits(dev[2][t], big["visits"][t]) and
                  R.same_bits(dev[0][t], big["policy"][t]) and int(dev[3][t]) == int(big["nc"][t]))
            if not ok:
                bad.append(t)
        assert not bad, "capacity %s: %d trees differ from the oracle, first %s" % (cap, len(bad), bad[:8])
        d1 = e.search(np.array([trees], np.uint32), 6)
        d2 = e.search(np.array([trees + 1], np.uint32), sims)
        c2 = e.eval_cache_stats()
        for (pol, _, vis, nc), r in ((d1, small[0]), (d2, small[1])):
            assert int(nc[0]) == int(r["nc"][0]) and R.same_bits(vis[0], r["visits"][0]) and \
                R.same_bits(pol[0], r["policy"][0]), cap
        for t in (trees, trees + 1):
            got, want = e.tree_child_stats(t)[1:], rs.children(t)[1:]
            assert all(R.same_bits(a, b) for a, b in zip(got, want)), (cap, t)
        print("capacity %s: %d entries; the 700-tree call: lookups %d hits %d inserts %d dropped %d; after the two "
              "single trees: hits %d" % (cap, c1["capacity"], c1["lookups"], c1["hits"], c1["inserts"], c1["dropped"],
                                         c2["hits"]))
        if cap == 0:
            assert c2["capacity"] == 0 and c2["hits"] == 0 and c2["lookups"] == 0
        else:
            assert c1["lookups"] == big["evals"]
            assert c2["hits"] > c1["hits"]          # the second single tree's first leaf
            if cap is None:
                assert c1["hits"] > 0 and c1["capacity"] > 8
            else:
                assert c1["capacity"] == 8 and c1["dropped"] > 0
        e.close()
    rs.close()


def orc_search(rs, trees, sims):
    """Mcts::search over a subset of rs's trees -> the result indexed by position in `trees`"""
    import oracle as orc
    rc, pol, ids, vis, nc = orc.search_c4(None, sims, eval_kind=orc.EVAL_NET, c=rs.c,
                                          trees=[rs.trees[t] for t in trees], eval_fn=rs.ev)
    rs.ev.check()
    assert rc >= 0
    return dict(policy=pol, ids=ids, visits=vis, nc=nc, evals=rc)


# ---------------------------------------------------------------- D: subtree reuse
def test_subtree_reuse(spai, yard):
    """160 trees (two chains), three rounds of 32 simulations, after each use_subtree on
    the last most-visited child that is not terminal, on the device and in the oracle
    (the new root keeps N and W); the default cache, and from the second round on the
    engine's own tail-mode policy"""
    trees, sims, name = 160, 32, "2x64"
    params, ev = yard(name)
    roots = R.positions(trees, trees, duplicates=trees // 10)
    e = engine(spai, name, params, trees, sims)
    load(e, roots)
    rs = R.RefSearch(roots, ev)
    order = np.arange(trees, dtype=np.uint32)
    root_ids = [0] * trees
    moved = 0
    for rnd in range(3):
        dev = e.search(order, sims)
        ref = rs.search(sims)
        compare(e, rs, dev, ref, order, root_ids, "round %d" % rnd)
        for t in range(trees):
            k = int(ref["nc"][t])
            if k == 0:
                continue
            j = R.most_visited_last(ref["visits"][t], k)
            s = rs.root_state(t)
            if s.next_state(s.valid_actions()[j]).status != 0:
                continue
            e.use_subtree(t, dev[1][t, j])
            rs.advance(t, j)
            root_ids[t] = int(dev[1][t, j])
            moved += 1
    print("re-rooted %d times; cache hits %d" % (moved, e.eval_cache_stats()["hits"]))
    assert moved > trees   # more than the first round alone can give: later rounds re-rooted too
    rs.close()
    e.close()


# ---------------------------------------------------------------- E: self-play
GAMES, SP_SIMS, SP_SEED = 160, 32, 11
SP_CASES = {
    "lockstep": dict(),
    "lockstep, cache off": dict(cache=0),
    "streamed": dict(window=64),
    "streamed, cache off": dict(window=64, cache=0),
    # the settings of test_self_play_tail_mode_matches_oracle (read per search call)
    "tail 8 leaves": dict(env={"SPAI_TAIL_LEAVES": "8", "SPAI_TAIL_TREE_EVALS": "0", "SPAI_TAIL_RUN": "64"}),
    "tail 64 leaves": dict(env={"SPAI_TAIL_LEAVES": "64", "SPAI_TAIL_TREE_EVALS": "0", "SPAI_TAIL_RUN": "1000"}),
    "tail every call": dict(env={"SPAI_TAIL_LEAVES": "0", "SPAI_TAIL_TREE_EVALS": "1000", "SPAI_TAIL_RUN": "64"}),
    "tail every call, run 3": dict(env={"SPAI_TAIL_LEAVES": "0", "SPAI_TAIL_TREE_EVALS": "1000", "SPAI_TAIL_RUN": "3"},
                                   cache=0),
}


@pytest.fixture(scope="module")
def self_play_ref(spai, yard):
    import oracle as orc
    _, ev = yard("2x64")
    t0 = time.perf_counter()
    ref = orc.self_play(orc.GAME_CONNECT4, GAMES, SP_SIMS, SP_SEED, eval_kind=orc.EVAL_NET, eval_fn=ev, max_plies=42)
    ev.check()
    print("oracle self-play: %d games, %d samples, %.0f evaluations, %.2f s" %
          (GAMES, len(ref["value"]), ref["evals"], time.perf_counter() - t0))
    by_game = {}
    for g in dict.fromkeys(ref["game"].tolist()):
        rows = np.flatnonzero(ref["game"] == g)
        assert np.all(np.diff(rows) == 1)
        by_game[g] = (int(rows[0]), len(rows))
    return ref, by_game


@pytest.mark.parametrize("case", list(SP_CASES))
def test_self_play(spai, yard, self_play_ref, case):
    """160 games at 32 simulations: encodings, visit policies, signed values and moves of
    every game, the emission order of a lockstep run, sims and evals"""
    ref, by_game = self_play_ref
    cfg = SP_CASES[case]
    params, _ = yard("2x64")
    env = cfg.get("env", {})
    os.environ.update(env)
    try:
        e = engine(spai, "2x64", params, GAMES, SP_SIMS, cache=cfg.get("cache"), seed=SP_SEED)
        games, stats = e.self_play(GAMES, window=cfg.get("window"))
        cs = e.eval_cache_stats()
        e.close()
    finally:
        for k in env:
            del os.environ[k]
    print("%s: evals %.0f, cache hits %.0f" % (case, stats["evals"], cs["hits"]))
    assert sorted(g["game"] for g in games) == sorted(by_game) and len(games) == GAMES
    if cfg.get("window") is None:
        assert [g["game"] for g in games] == list(by_game)   # the oracle's emission order
    bad = []
    for g in games:
        k, m = by_game[g["game"]]
        ok = (len(g["value"]) == m and R.same_bits(g["enc"], ref["enc"][k:k + m]) and
              R.same_bits(g["policy"], ref["policy"][k:k + m]) and R.same_bits(g["value"], ref["value"][k:k + m]) and
              list(g["moves"]) == list(ref["moves"][g["game"], :m]))
        if not ok:
            bad.append(g["game"])
    assert not bad, "%s: %d games differ from the oracle's, first %s" % (case, len(bad), sorted(bad)[:8])
    assert stats["games"] == GAMES and stats["positions"] == len(ref["value"])
    assert stats["sims"] == ref["sims"] and stats["evals"] == ref["evals"]
    if cfg.get("cache") == 0:
        assert cs["hits"] == 0
    else:
        assert cs["hits"] > 0


# ---------------------------------------------------------------- F: match
@pytest.mark.parametrize("vs_uniform", [False, True])
def test_match(spai, yard, vs_uniform):
    """8 games, 24 simulations, 2 opening plies: two different bf16 nets, and a net
    against UNIFORM, against match_ref.play_match with the callbacks as players"""
    import match_ref
    import oracle as orc
    n, sims, plies, seed = 8, 24, 2, 3
    (pa, eva), (pb, evb) = yard("2x64"), yard("2x64b")
    e = spai.Engine(num_searches=sims, max_trees=2 * n, eval_kind=spai.EVAL_UNIFORM)
    na, nb = spai.Net(e, 2, pa), spai.Net(e, 2, pb)
    if vs_uniform:
        dev = e.match((spai.EVAL_NET, na, sims), (spai.EVAL_UNIFORM, None, sims), n, opening_plies=plies, seed=seed)
        exp = match_ref.play_match((orc.EVAL_NET, eva, sims), (orc.EVAL_UNIFORM, None, sims), n, plies, seed=seed)
    else:
        dev = e.match((spai.EVAL_NET, na, sims), (spai.EVAL_NET, nb, sims), n, opening_plies=plies, seed=seed)
        exp = match_ref.play_match((orc.EVAL_NET, eva, sims), (orc.EVAL_NET, evb, sims), n, plies, seed=seed)
    eva.check()
    evb.check()
    (dg, ds), (eg, es) = dev, exp
    assert dg == eg
    for k in ("a_wins", "draws", "b_wins", "sims", "evals"):
        assert ds[k] == es[k], (k, ds[k], es[k])
    assert sum(len(g["moves"]) for g in dg) >= 7 * n
    na.close()
    nb.close()
    e.close()
