"""The CPU proof behind tests/test_learner_optimizer_gpu.py: the yardstick
(tests/adam_ref.py) is right, sharp enough, and fed inputs it can judge.

  * adam64 is torch.optim.Adam (float64, foreach=False): 12 steps on 10^5 entries
    with gradient magnitudes 1e-7 .. 1, sign changes, 2 % exact zeros and a block
    that never sees a gradient, at configs A, B and C, to rtol 1e-12.
  * adam32 (the kernels' order) and adam32_alt (the "hat" order) stay within the bar
    of adam64 at every step; the checker accepts both (tier 2 only for adam32).
  * every planted mistake is rejected, the worst entry >= 100 x its bar away.
  * the learners' inputs of the GPU file keep the subnormal mask under 1 % (the
    float64 restatements' gradients for the same batches, steps and configs).
  * config B's BatchNorm settings are visible: the restatements at config B differ
    from the defaults by >= 10 x the applied bars in the running mean, the running
    variance and the gradient at every shape of the GPU file's BatchNorm check.
  * the distance of PyTorch CPU fp32 from the restatements at config B, which
    decides whether a project bar stands (optimizer_cases.MEASURED_B, bn_bars).

Measured here (the synthetic run: 10^5 entries, p ~ N(0, 0.4), 12 steps):

    config  spread: the largest distance between adam32, adam32_alt and adam64 on p_prev - p_new
    A       1.19e-07 (1.2e-4 lr): one ulp32 of the largest |p| in [1, 2), p's own rounding
    B       1.19e-07 (4.0e-5 lr)
    C       0 (lr = 0: nobody moves)
    the learners' cases of the GPU file: 5.96e-08 .. 1.19e-07 (|p| up to [0.5, 1) or [1, 2))

    tier 1 of adam32 and of adam32_alt: at most 0.1 x the bar; the two float32 orders
    differ in the bits of ~5 % of the entry-steps, so tier 2 tells them apart.

    mistake                         distance of the worst entry, in bars:  A         B
    no bc1                                                                 1.9e+03   5.0e+03
    no bc2                                                                 6.4e+04   2.2e+04
    t off by one                                                           5.4e+02   1.4e+03
    betas swapped                                                          7.0e+02   3.2e+03
    eps inside the square root                                             2.1e+03   5.3e+03
    eps added before the bias correction                                   1.5e+03   2.3e+03
    (1 - b1) on m instead of g                                             1.7e+04   1.9e+04
    lr / beta1 / beta2 / eps at its default                                -         4.5e+03 / 2.1e+03 / 3.1e+02 / 6.6e+03

    subnormal mask, the GPU file's cases with the restatements' gradients: at most 0.23 %
    of the trainable entries (TicTacToe, 200 steps); the limit is 1 %.

    config B against the defaults, in units of the applied bar (>= 10 asserted):
    (game, blocks, B)     running mean  running variance  gradient
    (tictactoe, 1,   5)   1.6e+04       2.5e+03           189
    (chess,     1,   5)   1.8e+04       2.5e+03           748
    (connect4,  1,   5)   1.6e+04       3.0e+03           697
    (connect4,  1, 150)   1.5e+04       3.2e+03           107
    (connect4,  2,   8)   1.9e+04       4.2e+03           205

    PyTorch CPU fp32 against the float64 restatement at config B, every step from the
    same parameters, two steps (one for the one-step case (connect4, 2, 8)): loss
    (relative), gradient / max|g|, running statistics in units of rtol 1e-4 + atol
    1e-5.  The project's bars are 1e-4 (1e-3 later), 3e-4 and 1; every figure is under a
    third of its bar, so all of them stand (optimizer_cases.MEASURED_B, bn_bars):
    (game, blocks, B)     loss      gradient  running statistics
    (tictactoe, 1,   5)   6.9e-08   6.7e-07   2.0e-03
    (chess,     1,   5)   3.9e-08   1.4e-06   2.9e-03
    (connect4,  1,   5)   7.1e-08   8.1e-07   3.2e-03
    (connect4,  1, 150)   3.3e-08   1.2e-06   2.2e-03
    (connect4,  2,   8)   1.7e-07   1.3e-06   2.8e-03
"""
import numpy as np
import pytest

import adam_ref as AR
import optimizer_cases as OC

N, K = 100_000, 12
DEAD = slice(0, 1000)   # a block whose gradient is always 0


@pytest.fixture(scope="module")
def synthetic():
    """(p0, [G_1 .. G_K]) float32: per-entry gradient magnitude 10^U(-7, 0), held over
    the steps up to a factor U(0.5, 1.5) (so a small gradient stays small and eps
    counts), sign flipped with probability 0.3 per step, 2 % exact zeros per step, and
    the block DEAD always 0"""
    rng = np.random.default_rng(12)
    p0 = rng.normal(0, 0.4, N).astype(np.float32)
    mag = 10.0 ** rng.uniform(-7, 0, N)
    sign = rng.choice([-1.0, 1.0], N)
    grads = []
    for _ in range(K):
        sign = np.where(rng.random(N) < 0.3, -sign, sign)
        g = (sign * mag * rng.uniform(0.5, 1.5, N)).astype(np.float32)
        g[rng.random(N) < 0.02] = 0.0
        g[DEAD] = 0.0
        grads.append(g)
    for a in [p0] + grads:
        a.setflags(write=False)
    return p0, grads


def _fake_device(step_fn, p0, grads, cfg):
    """read_step of a `device` that makes its steps with step_fn(p, g, m, v, t, cfg) -> (p, m, v, ...)"""
    st = dict(p=p0, m=np.zeros(len(p0), np.float32), v=np.zeros(len(p0), np.float32))

    def read_step(k):
        out = step_fn(st["p"], grads[k - 1], st["m"], st["v"], k, cfg)
        st.update(p=np.asarray(out[0], np.float32), m=out[1], v=out[2])
        return grads[k - 1], st["p"]

    return read_step


# ------------------------------------------------------------------ adam64 is torch.optim.Adam
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_adam64_is_torch_adam(synthetic, name):
    import torch
    p0, grads = synthetic
    cfg = AR.CONFIGS[name]
    s = AR.settings(cfg)
    t = torch.tensor(p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([t], lr=s["lr"], betas=(s["beta1"], s["beta2"]), eps=s["eps"], foreach=False)
    p, m, v = p0.astype(np.float64), np.zeros(N), np.zeros(N)
    for k, g in enumerate(grads, 1):
        t.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        p, m, v = AR.adam64(p, g, m, v, k, cfg)
        np.testing.assert_allclose(p, t.detach().numpy(), rtol=1e-12, atol=1e-15)
    assert np.array_equal(p[DEAD], p0[DEAD].astype(np.float64))
    assert (name == "C") == np.array_equal(p, p0.astype(np.float64))


# ------------------------------------------------------------------ the float32 forms within the bar
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_float32_forms_within_the_bar(synthetic, name):
    p0, grads = synthetic
    cfg = AR.CONFIGS[name]
    tr = np.ones(N, bool)
    rep = AR.check_adam_steps(_fake_device(AR.adam32, p0, grads, cfg), p0, tr, cfg, K)
    alt = AR.check_adam_steps(_fake_device(AR.adam32_alt, p0, grads, cfg), p0, tr, cfg, K, tier2=False)
    print("config %s: spread %.3g (lr %.3g), tier 1 worst %.3g / %.3g x the bar, hat form off adam32 in %d entries" % (
        name, rep["spread"], rep["cfg"]["lr"], max(rep["tier1"]), max(alt["tier1"]), sum(alt["tier2"])))
    assert min(rep["idle"]) >= 1000
    if name != "C":
        assert 0 < rep["spread"] <= 1e-3 * rep["cfg"]["lr"]   # the issue's estimate: about 1e-5 lr per step
        assert sum(alt["tier2"]) > 0   # tier 2 tells the two float32 orders apart


# ------------------------------------------------------------------ planted mistakes
def _mutant(kind):
    """adam32 with one mistake; `kind` names it"""
    def step(p, g, m, v, t, cfg):
        s = AR.settings(cfg)
        d = AR.settings({})
        f = np.float32
        for field in ("lr", "beta1", "beta2", "eps"):
            if kind == field + " hard-coded":
                s[field] = d[field]
        lr, b1, b2, eps = f(s["lr"]), f(s["beta1"]), f(s["beta2"]), f(s["eps"])
        if kind == "betas swapped":
            b1, b2 = b2, b1
        tt = t + 1 if kind == "t off by one" else t
        bc1 = f(1.0 - float(b1) ** tt)
        bc2 = f(np.sqrt(1.0 - float(b2) ** tt))
        if kind == "no bc1":
            bc1 = f(1.0)
        if kind == "no bc2":
            bc2 = f(1.0)
        one = f(1.0)
        if kind == "(1 - b1) on m":
            mi = (one - b1) * m + b1 * g
        else:
            mi = b1 * m + (one - b1) * g
        vi = b2 * v + (one - b2) * g * g
        if kind == "eps inside the root":
            den = np.sqrt(vi + eps) / bc2
        elif kind == "eps before the correction":
            den = (np.sqrt(vi) + eps) / bc2
        else:
            den = np.sqrt(vi) / bc2 + eps
        return p - (lr / bc1) * (mi / den), mi, vi
    return step


MUTANTS = ["no bc1", "no bc2", "t off by one", "betas swapped", "eps inside the root", "eps before the correction",
           "(1 - b1) on m"]
HARD_CODED = ["lr hard-coded", "beta1 hard-coded", "beta2 hard-coded", "eps hard-coded"]


@pytest.mark.parametrize("name,kind", [(n, k) for n in "AB" for k in MUTANTS] + [("B", k) for k in HARD_CODED])
def test_checker_rejects_planted_mistakes(synthetic, name, kind):
    p0, grads = synthetic
    cfg = AR.CONFIGS[name]
    tr = np.ones(N, bool)
    rep = AR.adam_steps_report(_fake_device(_mutant(kind), p0, grads, cfg), p0, tr, cfg, K)
    print("config %s, %-28s worst entry %.3g x its bar (spread %.3g), %d entries off adam32" % (
        name, kind + ":", max(rep["tier1"]), rep["spread"], sum(rep["tier2"])))
    assert max(rep["tier1"]) >= 100.0
    assert sum(rep["tier2"]) > 0
    with pytest.raises(AssertionError):
        AR.assert_adam_report(rep)


def test_mutant_without_a_mistake_is_adam32(synthetic):
    """the mutants' scaffold itself is exact: kind = none passes all three tiers"""
    p0, grads = synthetic
    AR.check_adam_steps(_fake_device(_mutant("none"), p0, grads, AR.CONFIG_B), p0, np.ones(N, bool), AR.CONFIG_B, K)


# ------------------------------------------------------------------ the GPU file's inputs under the mask limit
@pytest.mark.parametrize("game,blocks,B,name,steps,start", OC.ADAM_CASES)
def test_learner_inputs_stay_under_the_mask_limit(game, blocks, B, name, steps, start):
    """every case of the GPU file with the float64 restatement as the device's forward and
    backward (its gradient rounded to float32) and adam32 as its optimizer: the checker
    passes, so in particular the subnormal mask stays under 1 % at every step"""
    cfg = AR.CONFIGS[name]
    p0 = OC.start(game, blocks, start)
    _, n, tr = OC.layout(game, blocks)
    batches = OC.cpu_batches(game, B, 3, OC.seed_of(game, blocks, B))
    st = dict(p=p0, m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))

    def read_step(k):
        P, G, loss = OC.forward_backward(game, st["p"], batches[(k - 1) % 3], blocks, cfg)
        assert np.all(np.isfinite(loss))
        G, P = G.astype(np.float32), P.astype(np.float32)
        p, m, v, _ = AR.adam32(P, G, st["m"], st["v"], k, cfg)
        p[~tr] = P[~tr]
        st.update(p=p, m=m, v=v)
        return G, p

    rep = AR.check_adam_steps(read_step, p0, tr, cfg, steps)
    print("%s (%d, %d) config %s, %d steps: masked at most %.3g of the trainable entries" % (
        game, blocks, B, name, steps, max(rep["masked"])))


# ------------------------------------------------------------------ BatchNorm settings: visible, and the bars
ALL_BN = OC.BN_CASES + [OC.BN_ONE_STEP_CASE]


@pytest.mark.parametrize("game,blocks,B", ALL_BN)
def test_config_b_batchnorm_settings_are_visible(game, blocks, B):
    p0 = OC.start(game, blocks)
    convs, n, tr = OC.layout(game, blocks)
    batch = OC.cpu_batches(game, B, 1, OC.seed_of(game, blocks, B))[0]
    Pb, Gb, _ = OC.forward_backward(game, p0, batch, blocks, AR.CONFIG_B)
    Pa, Ga, _ = OC.forward_backward(game, p0, batch, blocks, AR.CONFIG_A)
    bars = OC.bn_bars((game, blocks, B))
    mean, var = np.zeros(n, bool), np.zeros(n, bool)
    for c in convs:
        mean[c["mu"]:c["mu"] + c["co"]] = True
        var[c["var"]:c["var"] + c["co"]] = True
    tol = OC.PROJECT["run_atol"] + OC.PROJECT["run_rtol"] * np.abs(Pb)
    d_mean = (np.abs(Pb - Pa) / tol)[mean].max() / bars["run"]
    d_var = (np.abs(Pb - Pa) / tol)[var].max() / bars["run"]
    d_grad = np.abs(Gb - Ga).max() / np.abs(Gb).max() / bars["grad"]
    print("%s (%d, %d): config B vs the defaults: running mean %.3g, running variance %.3g, gradient %.3g x the bar" % (
        game, blocks, B, d_mean, d_var, d_grad))
    assert d_mean >= 10 and d_var >= 10 and d_grad >= 10


def _torch_fp32_steps(game, p0, batches, blocks, cfg):
    """PyTorch CPU fp32 at cfg: per step (parameters before, loss[3], gradient, parameters after)"""
    import torch
    kw = AR.restatement_kw(cfg)
    if game != "connect4":
        M = OC.restatement(game)[0]
        extra = dict(dtype=torch.float32) if game == "chess" else {}
        got = M.torch_train(p0, batches, blocks, **extra, **kw)
        before = [np.asarray(p0, np.float64)] + [np.asarray(g[2], np.float64) for g in got[:-1]]
        return [(b, np.asarray(g[0], np.float64), np.asarray(g[1], np.float64), np.asarray(g[2], np.float64))
                for b, g in zip(before, got)]
    from test_learner_ref_cpu import C4_DIMS, torch_forward_backward
    _, n, tr = OC.layout(game, blocks)
    p, m, v, out = np.asarray(p0, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), []
    for k, batch in enumerate(batches, 1):
        P, G, loss = torch_forward_backward(p, *batch, blocks, C4_DIMS, torch.float32, kw["momentum"], kw["bn_eps"])
        q, m, v, _ = AR.adam32(P, G, m, v, k, cfg)
        q[~tr] = P.astype(np.float32)[~tr]
        out.append((p.astype(np.float64), loss, G, q.astype(np.float64)))
        p = q
    return out


@pytest.mark.parametrize("game,blocks,B", ALL_BN)
def test_fp32_distance_at_config_b(game, blocks, B):
    """the figures behind optimizer_cases.MEASURED_B, live: a figure may not leave the
    table (beyond 2 x, or a thirtieth of its bar where the table's figure is tiny), so
    bn_bars keeps deciding from what this CPU measures"""
    steps = 1 if (game, blocks, B) == OC.BN_ONE_STEP_CASE else OC.BN_STEPS
    p0 = OC.start(game, blocks)
    _, n, tr = OC.layout(game, blocks)
    batches = OC.cpu_batches(game, B, steps, OC.seed_of(game, blocks, B))
    el = eg = er = 0.0
    for (before, loss, G, after), batch in zip(_torch_fp32_steps(game, p0, batches, blocks, AR.CONFIG_B), batches):
        P_ref, G_ref, loss_ref = OC.forward_backward(game, before, batch, blocks, AR.CONFIG_B)
        el = max(el, float(np.abs(loss - loss_ref).max() / np.abs(loss_ref).max()))
        eg = max(eg, float(np.abs(G - G_ref).max() / np.abs(G_ref).max()))
        er = max(er, OC.running_err(after, P_ref, tr))
    tab = OC.MEASURED_B[game, blocks, B]
    print("%-9s (%d, %3d): loss %.1e, gradient %.1e, running statistics %.1e (table: %.1e, %.1e, %.1e)" % (
        (game, blocks, B, el, eg, er) + tab))
    for live, t, b in zip((el, eg, er), tab, (OC.PROJECT["loss"], OC.PROJECT["grad"], 1.0)):
        assert live <= max(2 * t, b / 30), (live, t, b)


def test_torch_fp32_distance_takes_the_settings():
    """ttt_learner_ref / chess_learner_ref.torch_fp32_distance at config B (the smallest
    shapes): finite, and not what the defaults give"""
    kw = AR.restatement_kw(AR.CONFIG_B)
    for game, blocks, B in (("tictactoe", 1, 5), ("chess", 0, 2)):
        M = OC.restatement(game)[0]
        p0 = OC.start(game, blocks)
        batches = OC.cpu_batches(game, B, 2, OC.seed_of(game, blocks, B))
        at_b, at_a = M.torch_fp32_distance(p0, batches, blocks, **kw), M.torch_fp32_distance(p0, batches, blocks)
        print(game, "config B", at_b, "defaults", at_a)
        assert np.all(np.isfinite(at_b)) and at_b[0] < 1e-4 and at_b[1] < 3e-4 and tuple(at_b) != tuple(at_a)
