"""What tests/test_learner_optimizer_gpu.py (the device) and tests/test_adam_ref_cpu.py
(the CPU proof behind it) share: the three learners' float64 restatements behind
one interface, the start parameters, the CPU-side inputs, the cases and the bars
of the BatchNorm-settings check."""
import numpy as np

import adam_ref as AR

GAMES = ("tictactoe", "connect4", "chess")


def restatement(game):
    """(module, hidden, number of ReLU layers for `blocks`) of the game's float64 restatement"""
    if game == "connect4":
        import learner_ref as M
        return M, 64, lambda blocks: 2 * blocks + 3
    if game == "tictactoe":
        import ttt_learner_ref as M
        return M, 64, lambda blocks: 2 * blocks + 3
    import chess_learner_ref as M
    return M, 256, lambda blocks: 2 * blocks + 4


def layout(game, blocks):
    """(the conv records, the number of parameters, the trainable mask)"""
    M, hidden, _ = restatement(game)
    convs, _, n = M._layout(blocks, hidden)
    return convs, n, AR.trainable_mask(convs, n)


def forward_backward(game, p, batch, blocks, cfg, masks=None, diag=None):
    """the restatement's train-mode forward + backward at cfg's BatchNorm settings:
    (parameters with the running statistics updated, gradients, loss[3]), float64"""
    M, hidden, _ = restatement(game)
    s = AR.settings(cfg)
    return M.forward_backward(p, *batch, blocks, hidden, s["bn_momentum"], s["bn_eps"], masks, diag)


def init_params(game, blocks, seed):
    if game == "connect4":
        import spai
        return spai.init_params(blocks, 64, seed=seed)
    if game == "tictactoe":
        import spai_ttt
        return spai_ttt.init_params(blocks, seed)
    import spai_chess
    return spai_chess.init_params(blocks, seed)


def start(game, blocks, kind="trained"):
    """the learner tests' start parameters: init_params(blocks, blocks + 7), made
    trained-like with seed 60 + blocks"""
    import bf16_ref as R
    from learner_checks import start_params
    lay = {"connect4": lambda: R.c4_layout(blocks), "tictactoe": lambda: R.c4_layout(blocks, 64, (3, 3, 3, 9)),
           "chess": lambda: R.chess_layout(blocks)}[game]()
    return np.asarray(start_params(init_params(game, blocks, blocks + 7), lay, kind, 60 + blocks), np.float32)


def cpu_batches(game, B, steps, seed):
    """the inputs on the CPU.  TicTacToe and chess: exactly what the device tests feed
    (their _device_batches assert that the device's encodings equal these).  Connect4:
    the device tests take positions from random legal play on the device, so the CPU
    stands in with bf16_ref's random reachable positions and the same pi and z law."""
    if game == "connect4":
        from test_learner_ref_cpu import c4_batch
        return [c4_batch(B, seed + 97 * k) for k in range(steps)]
    M = restatement(game)[0]
    return M.make_batches(B, steps, seed)[2]


def seed_of(game, blocks, B):
    return 7000 + 100 * blocks + B


# ------------------------------------------------------------------ the Adam cases
# (game, blocks, B, config name, steps, start); three distinct batches, cycled
ADAM_CASES = [
    ("tictactoe", 1, 5, "A", 12, "trained"), ("tictactoe", 1, 5, "B", 12, "trained"), ("tictactoe", 1, 5, "C", 12, "trained"),
    ("tictactoe", 1, 5, "A", 200, "trained"),
    ("connect4", 1, 5, "A", 12, "trained"), ("connect4", 1, 5, "B", 12, "trained"),
    ("chess", 1, 2, "A", 12, "trained"), ("chess", 1, 2, "B", 12, "trained"),
    ("chess", 0, 1, "B", 3, "init"),
]

# ------------------------------------------------------------------ the BatchNorm-settings cases
# (game, blocks, B): config B, two steps, trained-like start; (connect4, 1, 150) is past
# the 146 samples whose 6144 values per channel k_bn_fwd keeps in registers
BN_CASES = [("tictactoe", 1, 5), ("chess", 1, 5), ("connect4", 1, 5), ("connect4", 1, 150)]
BN_ONE_STEP_CASE = ("connect4", 2, 8)   # two residual blocks, one step
BN_STEPS = 2
PROJECT = dict(loss=1e-4, loss_later=1e-3, grad=3e-4, run_rtol=1e-4, run_atol=1e-5)

# measured on the CPU at config B (test_adam_ref_cpu.test_fp32_distance_at_config_b prints
# and re-checks it): the distance of PyTorch CPU fp32 from the float64 restatement, both
# started at every step from the same parameters: (loss, relative, worst step; gradient /
# max|g|, worst step; running statistics, worst entry in units of rtol 1e-4 + atol 1e-5)
MEASURED_B = {
    ("tictactoe", 1, 5): (6.9e-08, 6.7e-07, 2.0e-03),
    ("chess", 1, 5): (3.9e-08, 1.4e-06, 2.9e-03),
    ("connect4", 1, 5): (7.1e-08, 8.1e-07, 3.2e-03),
    ("connect4", 1, 150): (3.3e-08, 1.2e-06, 2.2e-03),
    ("connect4", 2, 8): (1.7e-07, 1.3e-06, 2.8e-03),   # one step
}


def bn_bars(case):
    """the project's bars, or 3 x the measured PyTorch fp32 distance where that is over a
    third of the bar: loss rtol at step 1 and later, gradient / max|g|, and the factor on
    the running statistics' rtol 1e-4 + atol 1e-5"""
    el, eg, er = MEASURED_B[case]
    pick = lambda m, b: b if m <= b / 3 else 3 * m   # noqa: E731
    return dict(loss=pick(el, PROJECT["loss"]), loss_later=pick(el, PROJECT["loss_later"]), grad=pick(eg, PROJECT["grad"]),
                run=pick(er, 1.0))


def running_err(P, P_ref, tr):
    """worst running-statistic entry in units of rtol 1e-4 |ref| + atol 1e-5"""
    r = ~tr
    return float((np.abs(P[r] - P_ref[r]) / (PROJECT["run_atol"] + PROJECT["run_rtol"] * np.abs(P_ref[r]))).max())


def grads_same_masks(game, masks, g, p, batch, blocks, cfg, bar):
    """the device gradient g against the restatement run from p with the DEVICE's ReLU
    masks (activation > 0) at cfg's BatchNorm settings: the method of
    learner_checks.check_grads_same_masks.  The masks may differ from the restatement's
    own (pre > 0) only where its pre-activation is within 1e-4 of its layer's scale of
    zero; every entry within bar * max|g|.  Returns (error / max|g|, flips)."""
    diag = {}
    _, ref, _ = forward_backward(game, p, batch, blocks, cfg, masks=masks, diag=diag)
    flips = 0
    for l, mk in enumerate(masks):
        pre = diag["pre"][l]
        diff = np.asarray(mk).reshape(pre.shape) != (pre > 0)
        flips += int(diff.sum())
        assert np.all(np.abs(pre[diff]) <= 1e-4 * np.abs(pre).max()), (l, np.abs(pre[diff]).max())
    err = float(np.abs(g - ref).max() / np.abs(ref).max())
    print("grad vs f64 (device masks) %.3g of max|g|, flips %d, bar %.3g" % (err, flips, bar))
    assert err <= bar, (err, flips)
    return err, flips
