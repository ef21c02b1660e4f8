"""The fused Connect4 forward at group sizes 2 and 3 (net_c4.hip: the row tables
kRowTab and the taps they skip).  A position's priors and value may not depend on
the group size it ran at, the row it was given or the positions beside it, so
every batch here is compared bit for bit with the same positions evaluated one per
workgroup (S = 1, position-major rows, nothing skipped) and inside one S = 5 batch
(cell-major rows).

The group size follows the kernel's own rule from the device's CU count: grid =
min(CUs, n), S = ceil(n / grid).  Positions are reachable ones up to ply 36, so
full columns and the top row are occupied: those are the rows whose taps the edge
tiles drop.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_ROW = sum(1 << (c * 7 + 5) for c in range(7))   # bit = column * 7 + row
COLUMN = 0x3F
HIP_ATTR_MULTIPROCESSOR_COUNT = 63   # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


def reachable_positions(spai, games, plies, seed):
    """ongoing positions after `plies` random legal moves (device rules)"""
    e = spai.Engine(num_searches=1, max_trees=1)
    rng = np.random.default_rng(seed)
    e.games_resize(games)
    for _ in range(plies):
        lm = e.legal_mask(games)
        r = rng.random((games, 7)) * ((lm[:, None] >> np.arange(7)) & 1)
        e.apply(np.argmax(r, 1).astype(np.int32), check=False)
    st = e.games_read(games)
    e.close()
    return [tuple(int(v) for v in (r["x"], r["o"], r["n"], r["status"])) for r in st if r["status"] == 0]


def mixed_positions(spai, n, seed):
    """n ongoing positions with plies 4..36 interleaved, so every group mixes early and late ones"""
    per = [reachable_positions(spai, 2 * n, plies, seed + plies) for plies in (4, 13, 22, 29, 36)]
    out = [p for group in itertools.zip_longest(*per) for p in group if p is not None][:n]
    assert len(out) == n, "too few ongoing late positions"
    return out


def cu_count(spai):
    """the device's compute units, as net_create reads them (the HIP runtime that libspai.so links)"""
    v = ctypes.c_int(0)
    rc = spai.lib().hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0)
    assert rc == 0 and 16 <= v.value <= 1024, (rc, v.value)
    return v.value


def group_size(n, cus):
    grid = min(cus, n)
    return -(-n // grid)


@pytest.fixture(scope="module")
def case(spai):
    cus = cu_count(spai)
    states = mixed_positions(spai, 5 * cus, seed=3)
    occ = [s[0] | s[1] for s in states[:3 * cus]]
    assert any(o & TOP_ROW for o in occ), "no position reaches the top row"
    assert any((o >> (7 * c)) & COLUMN == COLUMN for o in occ for c in range(7)), "no position has a full column"
    e = spai.Engine(num_searches=1, max_trees=1)
    net = spai.Net(e, 6, spai.init_params(6, 64, seed=2))
    # S = 1: at most one position per workgroup
    small = [net.predict(states[i:i + cus]) for i in range(0, 3 * cus, cus)]
    small_p, small_v = np.concatenate([p for p, _ in small]), np.concatenate([v for _, v in small])
    assert group_size(5 * cus, cus) == 5
    large_p, large_v = net.predict(states)   # one round of S = 5
    yield {"cus": cus, "states": states, "net": net, "small": (small_p, small_v), "large": (large_p, large_v)}
    net.close()
    e.close()


def test_references_agree(case):
    n = 3 * case["cus"]
    np.testing.assert_array_equal(case["small"][0], case["large"][0][:n])
    np.testing.assert_array_equal(case["small"][1], case["large"][1][:n])
    assert np.all(np.isfinite(case["small"][0])) and np.all(np.abs(case["small"][1]) <= 1)
    assert len(np.unique(case["small"][1])) > n // 2   # the net tells the positions apart


# (batch size as a function of the CU count, group size, first position)
BATCHES = [
    pytest.param(lambda c: c + 1, 2, 0, id="S2-partial-last-group"),
    pytest.param(lambda c: 2 * c, 2, 0, id="S2-full"),
    pytest.param(lambda c: 2 * c + 2, 3, 0, id="S3-partial-last-group"),
    pytest.param(lambda c: 3 * c, 3, 0, id="S3-full"),
    pytest.param(lambda c: 2 * c - 3, 2, 1, id="S2-other-rows"),
    pytest.param(lambda c: 3 * c - 4, 3, 2, id="S3-other-rows"),
]


@pytest.mark.parametrize("size, S, first", BATCHES)
def test_small_group_batches_equal_other_group_sizes(case, size, S, first):
    n = size(case["cus"])
    assert group_size(n, case["cus"]) == S
    p, v = case["net"].predict(case["states"][first:first + n])
    for ref_p, ref_v in (case["small"], case["large"]):
        np.testing.assert_array_equal(p, ref_p[first:first + n])
        np.testing.assert_array_equal(v, ref_v[first:first + n])


# A 64-tree search forwards at most 64 leaves per launch, one per workgroup on any
# device of 64 CUs or more.  SPAI_FWD_GRID caps the forward's grid (read once per
# process, hence the child process): 24 workgroups run the 64 trees' leaves at S = 3
# and a half's 32 at S = 2; launches that the cache or finished trees thin out run
# at S = 1 or 2.
SEARCH_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import spai
from test_net_small_groups_gpu import reachable_positions

TREES, SIMS = 64, 32
roots = (reachable_positions(spai, 3 * TREES, 6, 4) + reachable_positions(spai, 3 * TREES, 17, 5))[::2][:TREES]
assert len(roots) == TREES
params = spai.init_params(6, 64, seed=5)


def search(trees, cache):
    e = spai.Engine(num_searches=SIMS, max_trees=len(trees), eval_kind=spai.EVAL_NET, max_moves=2)
    e.set_eval_cache(cache)
    net = spai.Net(e, 6, params)
    e.set_net(net)
    e.trees_create(len(trees))
    for i, r in enumerate(trees):
        e.tree_reset(i, r)
    pol, ids, vis, nc = e.search(np.arange(len(trees)), SIMS)
    net.close()
    e.close()
    return pol, vis, nc


ref = None
for cache in (0, 1 << 16):
    whole = search(roots, cache)
    halves = [search(roots[:TREES // 2], cache), search(roots[TREES // 2:], cache)]
    assert np.all(whole[1].sum(1) > 0)
    for k in range(3):
        np.testing.assert_array_equal(whole[k], np.concatenate([h[k] for h in halves]))
    if ref is None:
        ref = whole
    for k in range(3):
        np.testing.assert_array_equal(whole[k], ref[k])   # cache on == cache off
print("search ok")
"""


def test_search_at_small_groups_split_and_cache_invariance(spai):
    """64 trees x 32 sims through the net at S = 2..3: visit counts, policies and child counts equal those of the
    same trees searched in two halves, with the evaluation cache off and on"""
    env = dict(os.environ, SPAI_FWD_GRID="24")
    code = SEARCH_CHILD % {"pkg": os.path.join(REPO, "self-play-ai_amd"), "tests": os.path.join(REPO, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "search ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
