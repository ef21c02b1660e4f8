"""CPU checks behind the learner GPU tests at batches past 128 and from trained-like
parameters (test_learner_shapes_gpu.py, test_ttt_learner_gpu.py):

  * the float64 restatements of the train step (oracle/learner_ref.py,
    tests/ttt_learner_ref.py) against PyTorch float64 autograd, live, at those
    batches and from those parameters (negative gammas included), so they are a
    valid reference there;
  * sensitivity: restatement variants that make the mistakes a device kernel
    could make unnoticed at init / B <= 128 move the gradients (or the running
    mean) by at least 10 x the GPU tests' bar at the shapes and starts that are
    meant to catch them, and by exactly nothing where the older shapes sit.
"""
import numpy as np
import pytest

import bf16_ref as R
import learner_ref as LR
from learner_checks import start_params

C4_DIMS, TTT_DIMS = (3, 6, 7, 7), (3, 3, 3, 9)
REG_VALUES = 6144      # learner.hip: kBn * kBnPer values of a channel live in registers
REDUCE_SAMPLES = 128   # learner.hip: kWgReduceBatch chunks of kWgSamples samples per reduce trip
GPU_GRAD_BAR = 3e-4    # check_grads_same_masks


# ------------------------------------------------------------------ inputs
def c4_batch(B, seed):
    rng = np.random.default_rng(seed)
    x = R.c4_encode(R.c4_random_states(B, 24, seed)).reshape(B, 126)
    pi = rng.random((B, 7)).astype(np.float32) ** 2
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    return x, pi, rng.choice(np.array([-1, 0, 1], np.float32), B)


def c4_params(oracle, blocks, start):
    return start_params(oracle.init_params(oracle.GAME_CONNECT4, blocks, 64, blocks + 7), R.c4_layout(blocks), start,
                        60 + blocks)


# ------------------------------------------------------------------ PyTorch autograd
def torch_forward_backward(params, x, pi, z, blocks, dims, dtype, momentum=0.1, bn_eps=1e-5):
    """the model of gen_golden.learner_golden from a flat parameter vector, without the
    optimizer: train-mode forward, -(log_softmax(p) * pi).sum() / B + mse(v, z),
    backward.  Returns (parameters with the running statistics updated, gradients,
    loss[3]) as float64 arrays in the flat order."""
    import torch
    import torch.nn.functional as F
    C, H, W, A = dims
    layout = R.c4_layout(blocks, 64, dims)
    flat = torch.tensor(np.asarray(params, np.float64), dtype=dtype)
    T, off = {}, 0
    for name, shp in layout:
        n = int(np.prod(shp))
        t = flat[off:off + n].clone().reshape(shp)
        if name.split(".")[1] not in ("mu", "var"):
            t.requires_grad_(True)
        T[name] = t
        off += n
    assert off == len(params)

    def cbn(t, name, res=None):
        t = F.conv2d(t, T[name + ".w"], T[name + ".b"], padding=1)
        t = F.batch_norm(t, T[name + ".mu"], T[name + ".var"], T[name + ".g"], T[name + ".be"], training=True,
                         momentum=momentum, eps=bn_eps)
        return F.relu(t if res is None else t + res)

    B = len(x)
    t = cbn(torch.tensor(np.asarray(x, np.float64), dtype=dtype).reshape(B, C, H, W), "stem")
    for k in range(blocks):
        t = cbn(cbn(t, "res%d" % (2 * k)), "res%d" % (2 * k + 1), res=t)
    logits = F.linear(cbn(t, "pol").flatten(1), T["pol_lin.w"], T["pol_lin.b"])
    value = torch.tanh(F.linear(cbn(t, "val").flatten(1), T["val_lin.w"], T["val_lin.b"])).reshape(-1)
    pi_t = torch.tensor(np.asarray(pi, np.float64), dtype=dtype)
    z_t = torch.tensor(np.asarray(z, np.float64), dtype=dtype)
    lp = -(torch.log_softmax(logits, 1) * pi_t).sum() / B
    lv = ((value - z_t) ** 2).mean()
    (lp + lv).backward()
    P = np.concatenate([T[name].detach().numpy().reshape(-1) for name, _ in layout]).astype(np.float64)
    G = np.concatenate([(np.zeros(int(np.prod(shp))) if T[name].grad is None else T[name].grad.numpy().reshape(-1))
                        for name, shp in layout]).astype(np.float64)
    return P, G, np.array([(lp + lv).item(), lp.item(), lv.item()])


def _compare_with_torch(tag, ref, got, running):
    (P, G, loss), (Pt, Gt, losst) = ref, got
    eg = np.abs(G - Gt).max() / np.abs(G).max()
    el = np.abs(loss - losst).max()
    er = np.abs(P[running] - Pt[running]).max()
    print("%s: gradient %.2g of max|g|, loss %.2g, running statistics %.2g (bars 1e-10)" % (tag, eg, el, er))
    assert eg <= 1e-10 and el <= 1e-10 and er <= 1e-10
    assert np.array_equal(P[~running], Pt[~running])   # neither side moves a trainable parameter


def _running_mask(convs, n):
    running = np.zeros(n, bool)
    for c in convs:
        running[c["mu"]:c["mu"] + 2 * c["co"]] = True   # mu, then var
    return running


@pytest.mark.parametrize("blocks,B", [(1, 1), (1, 147), (1, 172), (2, 48)])
def test_c4_restatement_vs_torch_float64(oracle, blocks, B):
    """oracle/learner_ref.forward_backward against PyTorch float64 autograd from
    trained-like parameters: gradients within 1e-10 of max|g|, losses and updated
    running statistics within 1e-10.  Both sides are float64 (agreement is ~1e-15),
    so the bar fails on any real disagreement."""
    import torch
    p = c4_params(oracle, blocks, "trained")
    batch = c4_batch(B, 1000 * blocks + B)
    convs, _, n = LR._layout(blocks, 64)
    _compare_with_torch("c4 %d x %d" % (blocks, B), LR.forward_backward(p, *batch, blocks, 64),
                        torch_forward_backward(p, *batch, blocks, C4_DIMS, torch.float64), _running_mask(convs, n))


def test_ttt_restatement_vs_torch_float64():
    """tests/ttt_learner_ref.forward_backward against PyTorch float64 autograd from
    trained-like parameters, 2 blocks, B = 33 (the same bars)"""
    import spai_ttt
    import torch
    import ttt_learner_ref as TR
    blocks, B = 2, 33
    p = start_params(spai_ttt.init_params(blocks, blocks + 7), R.c4_layout(blocks, 64, TTT_DIMS), "trained", 60 + blocks)
    _, _, (batch,) = TR.make_batches(B, 1, 1000 * blocks + B)
    convs, _, n = TR._layout(blocks)
    _compare_with_torch("ttt %d x %d" % (blocks, B), TR.forward_backward(p, *batch, blocks),
                        torch_forward_backward(p, *batch, blocks, TTT_DIMS, torch.float64), _running_mask(convs, n))


# ------------------------------------------------------------------ sensitivity
def _per_channel(t):
    """[B][co][6][7] -> [co][B * 42] in the BatchNorm kernels' order (sample-major)"""
    return t.transpose(1, 0, 2, 3).reshape(t.shape[1], -1)


def _no_gamma(gam, inv, nn_):
    """k_bn_bwd's g without gamma[c]"""
    return inv / nn_


def _running_mean_without_old(old, mu, momentum):
    """k_bn_fwd's running mean without its (1 - momentum) * old term"""
    return momentum * mu


def _wgrad_first_trip(dzf, cols):
    """k_wgrad_reduce stopped after its first trip: the first 128 samples' chunks"""
    rows = REDUCE_SAMPLES * LR.CELLS
    return _WGRAD(dzf, cols) if len(dzf) <= rows else dzf[:rows].T @ cols[:rows]


def _bwd_sums_registers_only(dy, xhat):
    """k_bn_bwd's sums without the re-read loop: the first 6144 values of a channel"""
    if dy.shape[0] * LR.CELLS <= REG_VALUES:
        return _BWD_SUMS(dy, xhat)
    d, x = _per_channel(dy)[:, :REG_VALUES], _per_channel(xhat)[:, :REG_VALUES]
    return d.sum(1), (d * x).sum(1)


def _fwd_stats_registers_only(zz):
    """k_bn_fwd's sum and squared-deviation sum without the re-read loops: the first
    6144 values of a channel, still divided by all B * 42"""
    n = zz.shape[0] * LR.CELLS
    if n <= REG_VALUES:
        return _FWD_STATS(zz)
    v = _per_channel(zz)[:, :REG_VALUES]
    mu = v.sum(1) / n
    return mu, ((v - mu[:, None]) ** 2).sum(1) / n


SHAPES = [("init", 5), ("init", 129), ("init", 147), ("init", 172), ("trained", 5), ("trained", 172)]
_BWD_SUMS, _FWD_STATS, _WGRAD = LR._bn_bwd_sums, LR._bn_batch_stats, LR._wgrad

# mistake -> (the hook of learner_ref it replaces, the wrong version, what it moves,
#             the (start, B) that must catch it; every other (start, B) must see exactly 0)
MISTAKES = {
    # init_params draws gamma from U(0, 1) (tch's BatchNorm default), so a lost gamma shows at
    # every start; trained_like adds gammas above 1 and negative ones
    "bn backward without gamma": ("_bn_bwd_scale", _no_gamma, "grad", set(SHAPES)),
    "running mean loses (1-m)*old": ("_bn_running_mean", _running_mean_without_old, "running",
                                     {("trained", 5), ("trained", 172)}),
    "weight gradient from the first 128 samples": ("_wgrad", _wgrad_first_trip, "grad",
                                                   {("init", 129), ("init", 147), ("init", 172), ("trained", 172)}),
    "bn backward sums over the first 6144 values": ("_bn_bwd_sums", _bwd_sums_registers_only, "grad",
                                                    {("init", 147), ("init", 172), ("trained", 172)}),
    "bn forward statistics over the first 6144 values": ("_bn_batch_stats", _fwd_stats_registers_only, "grad",
                                                         {("init", 147), ("init", 172), ("trained", 172)}),
}


@pytest.fixture(scope="module")
def correct_steps(oracle):
    """the unmodified restatement at every (start, B), 1 block: computed once"""
    out = {}
    for start, B in SHAPES:
        p, batch = c4_params(oracle, 1, start), c4_batch(B, B)
        out[start, B] = (p, batch) + tuple(LR.forward_backward(p, *batch, 1, 64))
    return out


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_mistakes_show_where_they_should(correct_steps, monkeypatch, mistake):
    """Each mistake moves the gradient by >= 10 x the GPU bar (3e-3 of max|g|), or the
    running mean by >= 10 x check_learner_params' step-1 tolerance (1e-5 + 1e-4 |r|),
    at the starts and batches of test_learner_shapes_gpu.py that are meant to catch
    it, and by exactly 0 at the others: from init_params the running mean is 0, up to
    B = 128 the reduce kernel makes one trip, and up to B = 146 a channel fits the
    registers.  (A lost gamma shows everywhere: init_params' gamma is U(0, 1), not 1.)
    One block, fixed seeds."""
    hook, wrong, what, catching = MISTAKES[mistake]
    monkeypatch.setattr(LR, hook, wrong)
    convs, _, n = LR._layout(1, 64)
    means = np.zeros(n, bool)
    for c in convs:
        means[c["mu"]:c["mu"] + c["co"]] = True
    for (start, B), (p, batch, P, G, loss) in correct_steps.items():
        Pw, Gw, _ = LR.forward_backward(p, *batch, 1, 64)
        if what == "grad":
            moved = np.abs(Gw - G).max() / np.abs(G).max() / GPU_GRAD_BAR
        else:
            moved = (np.abs(Pw[means] - P[means]) / (1e-5 + 1e-4 * np.abs(P[means]))).max()
        print("%-50s %-7s B=%3d: %9.3g x the bar" % (mistake, start, B, moved))
        if (start, B) in catching:
            assert moved >= 10.0, (mistake, start, B, moved)
        else:
            assert moved == 0.0, (mistake, start, B, moved)
            assert np.array_equal(Pw, P) and np.array_equal(Gw, G)
