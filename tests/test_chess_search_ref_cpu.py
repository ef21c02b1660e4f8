"""The net-search reference (tests/chess_search_ref.py) must react to the faults
it exists for, and must not react to last-bits noise in the priors.  No GPU: the
evaluator is chessref.net_forward, the float64 restatement of the chess net, at
1 block and 32 channels with random parameters.

Over the 24 positions of chess_search_ref.positions(), 48 simulations per tree:
each injected fault of the search's net path changes the root visit counts of at
least a quarter of the trees; noise of up to 64 float32 ulp on every softmax
entry changes none."""
import numpy as np
import pytest

import chess_search_ref as R

BLOCKS, HIDDEN, SIMS = 1, 32, 48


def random_params(blocks, hidden, seed):
    """uniform +-sqrt(6 / fan_in) weights (the activations keep their scale through the ReLU
    layers, so logits and values spread as a trained net's do: a flat net's search ignores its
    value), biases a tenth of that, identity batch norms, in chessref's layout"""
    import chessref as ch
    rng = np.random.default_rng(seed)
    out = []
    bound = 1.0
    for kind, shp in ch.net_param_shapes(blocks, hidden):
        if kind == "bn":
            out += [np.ones(shp), np.zeros(shp), np.zeros(shp), np.ones(shp)]
        elif kind == "bias":
            out.append(rng.uniform(-0.1 * bound, 0.1 * bound, shp))
        else:
            bound = np.sqrt(6.0 / np.prod(shp[1:]))
            out.append(rng.uniform(-bound, bound, shp).ravel())
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in out])


@pytest.fixture(scope="module")
def setup():
    import chessref as ch
    ch.lib()
    params = random_params(BLOCKS, HIDDEN, 3)
    states = [s for _, _, s in R.positions()]
    ev = R.Evaluator(lambda x: ch.net_forward(params, BLOCKS, x, hidden=HIDDEN))

    def run(fault=None, noise=None, evaluator=ev):
        rs = R.RefSearch(states, evaluator, fault=fault, noise=noise)
        try:
            return R.visit_table(rs.search(SIMS)), rs
        finally:
            rs.close()

    base, rs = run()
    yield dict(ch=ch, states=states, run=run, base=base, base_search=rs, params=params)
    ch.arena_reset()


def test_positions_cover_the_planes(setup):
    states = setup["states"]
    assert len(states) == R.N_POSITIONS and all(s.status == 0 for s in states)
    enc = np.stack([s.encoding() for s in states])
    assert {s.side for s in states} == {0, 1}
    assert any(s.repetitions() == 2 for s in states)
    assert any(s.st.fifty > 0 for s in states)
    for p in (12, 13, 14, 15):
        assert {float(v) for v in enc[:, p, 0, 0]} == {0.0, 1.0}, p
    assert len({e.tobytes() for e in enc}) == len(states)


def test_search_is_reproducible_and_consistent(setup):
    again, rs = setup["run"]()
    assert again == setup["base"]
    assert all(sum(v) == SIMS - 1 for v in setup["base"])   # the first simulation expands the root, the rest pass a child
    assert rs.evals == setup["base_search"].evals
    assert rs.sides == {0, 1}
    assert len(rs.seen) > R.N_POSITIONS * 20


@pytest.mark.parametrize("fault", R.Fault.ALL)
def test_fault_changes_visit_counts(setup, fault):
    ch = setup["ch"]
    # encoding faults evaluate other inputs: a cache of their own
    ev = R.Evaluator(lambda x: ch.net_forward(setup["params"], BLOCKS, x, hidden=HIDDEN))
    got, _ = setup["run"](fault=fault, evaluator=ev)
    changed = sum(a != b for a, b in zip(got, setup["base"]))
    print(f"{fault}: {changed} of {len(got)} trees changed")
    assert 4 * changed >= len(got), (fault, changed)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_64_ulp_noise_changes_nothing(setup, seed):
    got, _ = setup["run"](noise=(seed, 64))
    changed = [t for t, (a, b) in enumerate(zip(got, setup["base"])) if a != b]
    assert not changed, changed


def test_large_noise_changes_trees(setup):
    """the noise reaches the search: at 100,000 ulp (1.2 %) trees do change"""
    got, _ = setup["run"](noise=(1, 100000))
    assert sum(a != b for a, b in zip(got, setup["base"])) >= 1
