"""Weight refresh of a Connect4 net in place (spai_net_set_params,
spai_net_set_params_from_learner; net_c4_pack.hip): a HIP kernel folds BatchNorm
and packs the bf16 fragments (or lays out the fp32 net's buffer) from the flat
parameters on the device.  The yardstick is spai_net_create's host packing: after
a refresh the net must be indistinguishable from a fresh one, so every comparison
here is np.array_equal against Net(engine, blocks, P) -- forward, predict, and
whole searches -- and the evaluation cache may not carry an old evaluation across.

Parameters are trained-like (bf16_ref.trained_like: BatchNorm statistics, biases
and negative gammas that make the fold non-trivial) or a learner's after three
steps.  Positions: the trained-params fixture's 64 inputs through forward (group
size 8), and reachable positions through predict at 1, 3 and 300 (the issue's
sizes) and at 3 * CUs - 5, where the kernel's own rule picks groups of 3."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import bf16_ref as R
from test_net_small_groups_gpu import cu_count, mixed_positions

pytestmark = pytest.mark.gpu

CASES = [(d, b) for d in ("bf16", "f32") for b in (0, 1, 2)] + [("bf16", 6)]


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def _dtype(spai, name):
    return spai.DTYPE_F32 if name == "f32" else spai.DTYPE_BF16


def _params(spai, blocks):
    """P1: init parameters; P2: trained-like ones of another seed"""
    p1 = spai.init_params(blocks, seed=1)
    p2 = R.trained_like(spai.init_params(blocks, seed=2), R.c4_layout(blocks), 7 + blocks)
    return p1, p2


@pytest.fixture(scope="module")
def inputs(spai):
    """x for forward, and the position sets for predict"""
    x = np.load(os.path.join(GOLDEN, "trained_like_nets.npz"))["c4_x"]
    big = 3 * cu_count(spai) - 5
    pos = mixed_positions(spai, max(big, 300), seed=5)
    return x, [pos[:1], pos[1:4], pos[:300], pos[:big]]


def _outputs(net, inputs):
    x, sets = inputs
    out = list(net.forward(x))
    for s in sets:
        out += list(net.predict(s))
    return out


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype,blocks", CASES)
def test_host_refresh_equals_fresh_net(spai, inputs, dtype, blocks):
    p1, p2 = _params(spai, blocks)
    dt = _dtype(spai, dtype)
    e = spai.Engine(num_searches=1, max_trees=1)
    fresh1, fresh2 = spai.Net(e, blocks, p1, dtype=dt), spai.Net(e, blocks, p2, dtype=dt)
    want1, want2 = _outputs(fresh1, inputs), _outputs(fresh2, inputs)
    assert all(np.isfinite(a).all() for a in want1 + want2)
    assert not any(np.array_equal(a, b) for a, b in zip(want1, want2))
    net = spai.Net(e, blocks, p1, dtype=dt)
    h = net.h.value
    assert _same(_outputs(net, inputs), want1)
    net.set_params(p2)
    assert net.h.value == h
    got = _outputs(net, inputs)
    for i, (a, b) in enumerate(zip(got, want2)):
        np.testing.assert_array_equal(a, b, err_msg="output %d after set_params(P2)" % i)
    net.set_params(p1)
    for i, (a, b) in enumerate(zip(_outputs(net, inputs), want1)):
        np.testing.assert_array_equal(a, b, err_msg="output %d after set_params(P1) again" % i)
    for n in (net, fresh1, fresh2):
        n.close()
    e.close()


def _stepped_learner(spai, e):
    """three train steps on the learner golden's batches (test_c4_learner_params_into_bf16_net)"""
    z = np.load(os.path.join(GOLDEN, "learner_c4_1x64.npz"))
    blocks, hidden, seed, B, K = [int(v) for v in z["meta"]]
    assert (blocks, hidden, K) == (1, 64, 3)
    L = spai.Learner(e, blocks, spai.init_params(blocks, hidden, seed=seed), hidden=hidden)
    for k in range(K):
        L.train_batch(z["states"][k], z["policies"][k], z["values"][k])
    return L


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_device_refresh_equals_fresh_net(spai, inputs, dtype):
    dt = _dtype(spai, dtype)
    e = spai.Engine(num_searches=1, max_trees=1)
    p1 = spai.init_params(1, seed=1)
    net, net_h = spai.Net(e, 1, p1, dtype=dt), spai.Net(e, 1, p1, dtype=dt)
    before = _outputs(net, inputs)
    L = _stepped_learner(spai, e)
    net.set_params(L)            # straight behind the last step, no host copy in between
    got = _outputs(net, inputs)
    p = L.params()
    d = R.unflatten(p, R.c4_layout(1))
    assert np.abs(d["stem.mu"]).max() > 1e-3 and np.abs(d["res1.var"] - 1).max() > 1e-3   # the statistics moved
    fresh = spai.Net(e, 1, p, dtype=dt)
    want = _outputs(fresh, inputs)
    net_h.set_params(p)
    via_host = _outputs(net_h, inputs)
    assert not any(np.array_equal(a, b) for a, b in zip(before, want))
    for i, (a, b, c) in enumerate(zip(got, want, via_host)):
        np.testing.assert_array_equal(a, b, err_msg="output %d: set_params(learner) vs a fresh net" % i)
        np.testing.assert_array_equal(c, b, err_msg="output %d: set_params(learner.params()) vs a fresh net" % i)
    L.close()
    for n in (net, net_h, fresh):
        n.close()
    e.close()


# ---------------------------------------------------------------- search and the evaluation cache
TREES, SIMS = 8, 64


def _engine(spai, blocks, params):
    e = spai.Engine(num_searches=SIMS, max_trees=TREES, eval_kind=spai.EVAL_NET, seed=3)
    e.set_eval_cache(1 << 16)
    e.set_net(spai.Net(e, blocks, params))
    e.trees_create(TREES)
    return e


def _roots(e):
    return [e.tree_child_stats(t) for t in range(TREES)]


def _search_fresh(e):
    for t in range(TREES):
        e.tree_reset(t)
    out = e.search(np.arange(TREES))
    return list(out) + [a for r in _roots(e) for a in r]


def _assert_equal_lists(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg="%s, array %d" % (what, i))


def test_cache_does_not_survive_a_refresh(spai):
    p1, p2 = _params(spai, 1)
    e = _engine(spai, 1, p1)
    first = _search_fresh(e)
    c0 = e.eval_cache_stats()
    assert c0["capacity"] > 0 and c0["live"] > 0 and c0["inserts"] > 0
    e.net.set_params(p2)
    c1 = e.eval_cache_stats()
    assert c1["live"] == 0 and c1["clears"] == c0["clears"] + 1
    got = _search_fresh(e)
    ref = _engine(spai, 1, p2)
    want = _search_fresh(ref)
    ref.close()
    _assert_equal_lists(got, want, "search after set_params(P2)")
    assert not all(np.array_equal(a, b) for a, b in zip(got, first)), "the refreshed net searched like the old one"
    # the same from a learner's device parameters
    L = _stepped_learner(spai, e)
    c2 = e.eval_cache_stats()
    assert c2["live"] > 0
    e.net.set_params(L)
    c3 = e.eval_cache_stats()
    assert c3["live"] == 0 and c3["clears"] == c2["clears"] + 1
    got = _search_fresh(e)
    ref = _engine(spai, 1, L.params())
    want = _search_fresh(ref)
    ref.close()
    _assert_equal_lists(got, want, "search after set_params(learner)")
    # a net the engine does not search with leaves the table alone
    c4 = e.eval_cache_stats()
    assert c4["live"] > 0
    other = spai.Net(e, 1, p1)
    other.set_params(p2)
    other.set_params(L)
    c5 = e.eval_cache_stats()
    assert c5["live"] == c4["live"] and c5["clears"] == c4["clears"]
    other.close()
    L.close()
    e.close()


def _kept_tree_run(spai, p1, p2, in_place):
    e = _engine(spai, 1, p1)
    pol, ids, vis, nc = e.search(np.arange(TREES))
    for t in range(TREES):
        e.use_subtree(t, ids[t, t % int(nc[t])])
    if in_place:
        e.net.set_params(p2)
    else:
        e.set_net(spai.Net(e, 1, p2))
    out = [pol, ids, vis, nc] + list(e.search(np.arange(TREES))) + [a for r in _roots(e) for a in r]
    e.close()
    return out


def test_refresh_between_searches_of_a_kept_tree(spai):
    p1, p2 = _params(spai, 1)
    got = _kept_tree_run(spai, p1, p2, True)
    want = _kept_tree_run(spai, p1, p2, False)
    _assert_equal_lists(got, want, "kept tree, set_params against set_net(Net(P2))")


def test_errors_leave_the_weights_alone(spai, inputs):
    p1, p2 = _params(spai, 1)
    e, e2 = spai.Engine(num_searches=1, max_trees=1), spai.Engine(num_searches=1, max_trees=1)
    for dt in (spai.DTYPE_BF16, spai.DTYPE_F32):
        net = spai.Net(e, 1, p1, dtype=dt)
        want = _outputs(net, inputs)
        with pytest.raises(spai.SpaiError) as ei:
            net.set_params(p2[:-1])
        assert ei.value.code == -1
        L2 = spai.Learner(e, 2, spai.init_params(2, seed=2))      # another blocks
        with pytest.raises(spai.SpaiError) as ei:
            net.set_params(L2)
        assert ei.value.code == -1 and "blocks" in str(ei.value)
        L2.close()
        Lo = spai.Learner(e2, 1, p2)                                # another engine
        with pytest.raises(spai.SpaiError) as ei:
            net.set_params(Lo)
        assert ei.value.code == -1 and "engine" in str(ei.value)
        Lo.close()
        _assert_equal_lists(_outputs(net, inputs), want, "outputs after the refused refreshes")
        net.close()
    e.close()
    e2.close()
