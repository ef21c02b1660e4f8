"""The three device learners' optimizer on the MI355X: the Adam step pinned entry by
entry to exact references, every spai_adam_config field at a non-default value, and
the config's validation.

Adam, step by step (adam_ref.check_adam_steps).  After every device step the
gradient and the parameters are read back; three references (float64, float32 in
the kernels' operation order, float32 in the "hat" order) make the same step from
the device's previous parameters with the device's gradient and their own moments.
  tier 1  |P - adam64| <= 1 ulp32(|p|) + 4 x the references' own spread, every entry
  tier 2  P == adam32 bit for bit wherever no intermediate is subnormal
  tier 3  entries with zero gradient and zero moments keep their bits
and the running statistics' gradient is exactly 0.  Config B (lr 3e-3, betas 0.8 /
0.95, eps 1e-3, BatchNorm momentum 0.3, eps 1e-2) moves every field off its default
with eps comparable to sqrt(v), so its placement matters; config C (lr 0, beta1 0,
beta2 0.5) must leave every trainable entry's bits alone while the running
statistics still move.  tests/test_adam_ref_cpu.py proves the yardstick: adam64 is
torch.optim.Adam, the bar holds between the references, each planted mistake
(a lost or misplaced bias correction, t off by one, swapped betas, eps inside the
root or before the correction, (1 - b1) on m, each field hard-coded to its default)
lands >= 100 x the bar away, and these inputs keep the subnormal mask under 1 %.
The references' spread on these cases: 6.0e-8 .. 1.2e-7, one ulp32 of the largest |p|.

BatchNorm settings (config B, two steps, trained-like start): every step's loss,
gradient (under the device's ReLU masks) and running statistics against the float64
restatement called with the same settings, started at every step from the device's
own parameters before it, so Adam's noise on ill-conditioned entries stays out.
Bars: the project's (loss rtol 1e-4 at step 1 and 1e-3 later, gradient 3e-4 max|g|,
running statistics rtol 1e-4 + atol 1e-5), or 3 x the CPU-measured distance of
PyTorch fp32 from the restatement where that is over a third of the bar
(optimizer_cases.MEASURED_B, the table in test_adam_ref_cpu.py).  The CPU file also
asserts that config B's restatement differs from the defaults' by >= 10 x these
bars in the running mean, the running variance and the gradient at every shape.
The parameters after each step are held by check_adam_steps.

Outcome on the MI355X: tier 2 holds bit for bit in every case (no entry of any step
differs from adam32; sqrtf and the division are correctly rounded, nothing is
contracted), tier 1 sits at <= 0.17 x the bar, float32(1 - 0.9^t) is exactly 1 from
step 165, and no device gradient put an entry into the subnormal mask.
"""
import ctypes as C

import numpy as np
import pytest

import adam_ref as AR
import optimizer_cases as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spai():
    import spai as s
    assert s.device_count() > 0, "no GPU visible"
    return s


@pytest.fixture(scope="module")
def st():
    import spai_ttt
    return spai_ttt


@pytest.fixture(scope="module")
def sc():
    import spai_chess
    return spai_chess


class _Game:
    """one game's engine, device batches and learner constructor behind one interface"""

    def __init__(self, game, spai, st, sc):
        self.game, self.spai, self.st, self.sc = game, spai, st, sc
        if game == "connect4":
            self.eng = spai.Engine(num_searches=1, max_trees=1)
        elif game == "tictactoe":
            self.eng = st.TTTEngine(num_searches=1, max_trees=1)
        else:
            from test_chess_learner_gpu import _engine
            self.eng = _engine(sc)

    def batches(self, B, steps, seed):
        if self.game == "connect4":
            from test_learner_shapes_gpu import _batches
            return _batches(self.spai, self.eng, [B] * steps, seed=seed)
        if self.game == "tictactoe":
            from test_ttt_learner_gpu import _device_batches
            return _device_batches(self.eng, B, steps, seed)
        from test_chess_learner_gpu import _device_batches
        return _device_batches(self.sc, self.eng, B, steps, seed)

    def learner(self, blocks, params, cfg):
        if self.game == "connect4":
            return self.spai.Learner(self.eng, blocks, params, **cfg)
        if self.game == "tictactoe":
            return self.st.TTTLearner(self.eng, blocks, params, **cfg)
        return self.sc.ChessLearner(self.eng, blocks, params, **cfg)

    def masks(self, L, blocks):
        return [L.activation(l) > 0 for l in range(OC.restatement(self.game)[2](blocks))]

    def close(self):
        self.eng.close()


# ------------------------------------------------------------------ Adam, step by step
def _adam_case(G, blocks, B, cfg_name, K, start, between=None):
    cfg = AR.CONFIGS[cfg_name]
    batches = G.batches(B, 3, OC.seed_of(G.game, blocks, B))
    assert not any(np.array_equal(batches[a][0], batches[b][0]) for a in range(3) for b in range(a))
    p0 = OC.start(G.game, blocks, start)
    _, n, tr = OC.layout(G.game, blocks)
    L = G.learner(blocks, p0, cfg)
    assert np.array_equal(L.params(), p0)

    def read_step(k):
        if between:
            between(L, k)
        loss = L.train_batch(*batches[(k - 1) % 3])
        assert np.all(np.isfinite(loss)), (k, loss)
        return L.grads(), L.params()

    rep = AR.check_adam_steps(read_step, p0, tr, cfg, K)
    P = L.params()
    L.close()
    return rep, p0, P, tr


@pytest.mark.parametrize("game,blocks,B,cfg_name,K,start", OC.ADAM_CASES)
def test_adam_steps(spai, st, sc, game, blocks, B, cfg_name, K, start):
    """every case of optimizer_cases.ADAM_CASES: the smallest shapes that reach k_adam
    (Connect4) and k_lc_adam (TicTacToe, chess); 200 steps pass the point where
    float32(1 - 0.9^t) is exactly 1; chess (0, 1) from init_params is the head-only
    path, whose policy rows of unreachable moves have exactly zero gradient"""
    G = _Game(game, spai, st, sc)
    rep, p0, P, tr = _adam_case(G, blocks, B, cfg_name, K, start)
    if K == 200:
        assert rep["bc1"][-1] == np.float32(1.0) and rep["bc1"][11] < np.float32(1.0)
        print("bc1 is exactly 1.0f from step", 1 + next(i for i, b in enumerate(rep["bc1"]) if b == np.float32(1.0)))
    if cfg_name == "C":   # lr = 0: no trainable bit moves; the running statistics do
        assert np.array_equal(P[tr].view(np.uint32), p0[tr].view(np.uint32))
        assert np.all(P[~tr] != p0[~tr])
    else:
        assert rep["moved"] > 0
    if (game, blocks) == ("chess", 0):
        assert min(rep["idle"]) > 1000, "expected the unreachable moves' policy rows under tier 3: %s" % rep["idle"]
    G.close()


def test_adam_steps_across_compute_switch(spai, st, sc):
    """chess, config B: bf16 compute after step 4, back to f32 after step 8.  The
    moments and the step count survive set_compute, so the references just carry on."""
    G = _Game("chess", spai, st, sc)
    seen = []

    def between(L, k):
        if k == 5:
            L.set_compute("bf16")
        if k == 9:
            L.set_compute("f32")
        seen.append(L.compute())

    _adam_case(G, 1, 2, "B", 12, "trained", between)
    assert seen == ["f32"] * 4 + ["bf16"] * 4 + ["f32"] * 4
    G.close()


# ------------------------------------------------------------------ train_batches and train at config B
def test_train_batches_is_train_batch_at_config_b(spai, st, sc):
    """Connect4: train_batches(k = 6) stages each step's bias corrections with its batch;
    at config B it equals six train_batch calls bit for bit, losses and parameters"""
    G = _Game("connect4", spai, st, sc)
    k, B, blocks = 6, 5, 1
    batches = G.batches(B, k, 61)
    p0 = OC.start("connect4", blocks)
    one = G.learner(blocks, p0, AR.CONFIG_B)
    losses = np.array([one.train_batch(*b) for b in batches])
    many = G.learner(blocks, p0, AR.CONFIG_B)
    got = many.train_batches(*(np.concatenate([b[i] for b in batches]) for i in range(3)), k)
    assert np.array_equal(got, losses) and np.all(np.isfinite(got))
    assert np.array_equal(many.params(), one.params()) and np.array_equal(many.grads(), one.grads())
    default = G.learner(blocks, p0, {})
    for b in batches:
        default.train_batch(*b)
    assert not np.array_equal(default.params(), one.params())   # the settings reached the step
    for L in (one, many, default):
        L.close()
    G.close()


@pytest.mark.parametrize("game", OC.GAMES)
def test_second_train_is_a_fresh_learner_at_config_b(spai, st, sc, game):
    """train() starts Adam over and keeps the settings: a second call on the same learner
    equals, bit for bit, a fresh learner created from the first call's parameters"""
    G = _Game(game, spai, st, sc)
    blocks, n = 1, 5
    (x, pi, z), = G.batches(n, 1, 23)
    p0 = OC.start(game, blocks)
    A = G.learner(blocks, p0, AR.CONFIG_B)
    A.train(x, pi, z, epochs=2, batch=2, seed=3)
    P1 = A.params()
    loss_a = A.train(x, pi, z, epochs=1, batch=2, seed=4)
    F = G.learner(blocks, P1, AR.CONFIG_B)
    loss_f = F.train(x, pi, z, epochs=1, batch=2, seed=4)
    assert np.array_equal(A.params(), F.params()) and np.array_equal(A.grads(), F.grads())
    assert np.array_equal(np.asarray(loss_a), np.asarray(loss_f)) and np.all(np.isfinite(loss_a))
    D = G.learner(blocks, P1, {})
    D.train(x, pi, z, epochs=1, batch=2, seed=4)
    assert not np.array_equal(D.params(), F.params())   # the settings reached train()
    for L in (A, F, D):
        L.close()
    G.close()


# ------------------------------------------------------------------ BatchNorm settings
def _check_bn_step(game, case, k, p_before, batch, blocks, masks, loss, g, P, tr):
    """one device step at config B against the restatement from the same parameters"""
    bars = OC.bn_bars(case)
    OC.grads_same_masks(game, masks, g, p_before, batch, blocks, AR.CONFIG_B, bars["grad"])
    P_ref, _, loss_ref = OC.forward_backward(game, p_before, batch, blocks, AR.CONFIG_B, masks=masks)
    rtol = bars["loss"] if k == 1 else bars["loss_later"]
    run = OC.running_err(P.astype(np.float64), P_ref, tr)
    print("step %d: loss %s vs %s (rtol %.3g), running statistics %.3g of rtol 1e-4 + atol 1e-5 (bar %.3g)" % (
        k, loss, loss_ref, rtol, run, bars["run"]))
    np.testing.assert_allclose(loss, loss_ref, rtol=rtol, atol=1e-5 if k == 1 else 1e-4)
    assert run <= bars["run"], run
    assert np.all(g[~tr] == 0)


@pytest.mark.parametrize("game,blocks,B", OC.BN_CASES)
def test_bn_settings_vs_restatement(spai, st, sc, game, blocks, B):
    """k_lc_bn_fwd<9> (TicTacToe), k_lc_bn_fwd<64> (chess), k_bn_fwd in registers (Connect4,
    B = 5) and with its re-read loops (B = 150) at momentum 0.3 and eps 1e-2"""
    G = _Game(game, spai, st, sc)
    batches = G.batches(B, OC.BN_STEPS, OC.seed_of(game, blocks, B))
    p0 = OC.start(game, blocks)
    _, n, tr = OC.layout(game, blocks)
    L = G.learner(blocks, p0, AR.CONFIG_B)
    state = {"p": p0}

    def read_step(k):
        loss = L.train_batch(*batches[k - 1])
        g, P = L.grads(), L.params()
        _check_bn_step(game, (game, blocks, B), k, state["p"], batches[k - 1], blocks, G.masks(L, blocks), loss, g, P, tr)
        state["p"] = P
        return g, P

    AR.check_adam_steps(read_step, p0, tr, AR.CONFIG_B, OC.BN_STEPS)
    L.close()
    G.close()


def test_bn_settings_one_step(spai, st, sc):
    """Connect4 (2, 8), config B, one step from the trained-like start: two residual
    blocks at a batch between BN_CASES' 5 and 150, the same bars against the same
    restatement"""
    game, blocks, B = OC.BN_ONE_STEP_CASE
    G = _Game(game, spai, st, sc)
    batch, = G.batches(B, 1, OC.seed_of(game, blocks, B))
    p0 = OC.start(game, blocks)
    _, n, tr = OC.layout(game, blocks)
    L = G.learner(blocks, p0, AR.CONFIG_B)
    loss = L.train_batch(*batch)
    g, P = L.grads(), L.params()
    _check_bn_step(game, OC.BN_ONE_STEP_CASE, 1, p0, batch, blocks, G.masks(L, blocks), loss, g, P, tr)
    AR.check_adam_steps(lambda k: (g, P), p0, tr, AR.CONFIG_B, 1)
    L.close()
    G.close()


# ------------------------------------------------------------------ validation
NAN, INF = float("nan"), float("inf")
REJECTED = [("lr", -1e-3), ("lr", NAN), ("lr", INF),
            ("beta1", -0.1), ("beta1", 1.0), ("beta1", NAN), ("beta2", -0.1), ("beta2", 1.0), ("beta2", NAN),
            ("eps", 0.0), ("eps", -1e-8), ("eps", NAN), ("eps", INF),
            ("bn_momentum", -0.1), ("bn_momentum", 1.5), ("bn_momentum", NAN),
            ("bn_eps", 0.0), ("bn_eps", -1e-5), ("bn_eps", NAN), ("bn_eps", INF)]
ACCEPTED = [dict(lr=0.0), dict(beta1=0.0), dict(beta2=0.0), dict(bn_momentum=0.0), dict(bn_momentum=1.0)]


def _raw_create(G, blocks, p0, cfg):
    """the C entry point itself: (return code, the handle it left in *out, the message)"""
    import spai
    c = spai.AdamConfig()
    assert spai.lib().spai_adam_config_default(C.byref(c)) == 0
    for k, v in cfg.items():
        setattr(c, k, float(v))
    h = C.c_void_p(0xDEAD)   # create must overwrite it with NULL on failure
    p = np.ascontiguousarray(p0, np.float32)
    ptr = p.ctypes.data_as(C.c_void_p)
    if G.game == "connect4":
        lib = spai.lib()
        rc = lib.spai_learner_create(G.eng.h, blocks, 64, ptr, p.size, C.byref(c), C.byref(h))
    elif G.game == "tictactoe":
        lib = G.st.lib()
        rc = lib.spai_ttt_learner_create(G.eng.h, blocks, ptr, p.size, C.byref(c), C.byref(h))
    else:
        lib = G.sc.lib()
        rc = lib.spai_chess_learner_create(G.eng.h, blocks, ptr, p.size, C.byref(c), C.byref(h))
    return rc, h.value, lib.spai_last_error().decode()


@pytest.mark.parametrize("game", OC.GAMES)
def test_create_validates_the_config(spai, st, sc, game):
    """every out-of-range field: SPAI_ERR_INVALID (-1), a message naming the field, *out
    NULL; the ends of the ranges are accepted; and after the rejections a learner with
    the defaults still trains on the same engine"""
    G = _Game(game, spai, st, sc)
    blocks = 0
    p0 = OC.init_params(game, blocks, 3)
    for field, value in REJECTED:
        rc, h, msg = _raw_create(G, blocks, p0, {field: value})
        assert rc == -1 and h is None, (field, value, rc, h)
        assert ("adam config: %s must" % field) in msg, (field, value, msg)
        with pytest.raises(spai.SpaiError) as ei:
            G.learner(blocks, p0, {field: value})
        assert ei.value.code == -1
    for cfg in ACCEPTED:
        G.learner(blocks, p0, cfg).close()
    batch, = G.batches(2, 1, 5)
    L = G.learner(blocks, p0, {})
    loss = L.train_batch(*batch)
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(L.params())) and not np.array_equal(L.params(), p0)
    L.close()
    G.close()
