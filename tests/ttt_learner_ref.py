"""TEST INFRASTRUCTURE ONLY (the checker, never the product): a numpy float64
restatement of the reference training step for the TicTacToe net
(model/tictactoe.rs:50-81 under model/mod.rs:128-141), the step that
oracle/learner_ref.py restates for Connect4, on a 3x3 board with a 9-way head:

  * forward in train mode: stem conv3x3(3->64)+BN+ReLU, blocks
    relu(x + BN(conv(relu(BN(conv(x)))))), policy head conv(64->32)+BN+ReLU,
    flatten (NCHW, c*9 + cell), linear 288->9; value head conv(64->3)+BN+ReLU,
    flatten, linear 27->1, tanh.  BatchNorm: batch mean and biased variance over
    (B, 3, 3); running stats r <- 0.9 r + 0.1 stat with the unbiased variance.
  * loss = -(log_softmax(p) * pi).sum() / B + mean((v - z)^2)
  * backward, then Adam (beta 0.9/0.999, eps 1e-8, lr 1e-3, no weight decay).

Parameters are the flat construction-order vector of spai_ttt_net_init_params.
Pinned against PyTorch CPU fp32 (tests/golden/learner_ttt_1x64.npz, made by
tests/golden/gen_ttt_learner_golden.py) in tests/test_ttt_learner_cpu.py.
Same interface as oracle/learner_ref.py: train_step, train, masks=, diag=.
"""
import numpy as np

ROWS, COLS, CELLS, ACTIONS, HIDDEN = 3, 3, 9, 9, 64


def _layout(blocks, hidden=HIDDEN):
    """offsets of every tensor in the flat parameter vector"""
    convs, off = [], 0

    def conv(ci, co):
        nonlocal off
        c = dict(ci=ci, co=co, w=off)
        off += co * ci * 9
        c["b"] = off
        off += co
        c["g"], c["be"], c["mu"], c["var"] = off, off + co, off + 2 * co, off + 3 * co
        off += 4 * co
        convs.append(c)

    conv(3, hidden)
    for _ in range(2 * blocks):
        conv(hidden, hidden)
    conv(hidden, 32)
    lin = {"pw": off}
    off += ACTIONS * 32 * CELLS
    lin["pb"] = off
    off += ACTIONS
    conv(hidden, 3)
    lin["vw"] = off
    off += 3 * CELLS
    lin["vb"] = off
    off += 1
    return convs, lin, off


def _im2col(x):
    """[B][C][3][3] -> [B*9][C*9], column order (ci, kh, kw) = w.reshape(co, ci*9)"""
    B, C = x.shape[:2]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    cols = np.empty((B, C, 9, ROWS, COLS), x.dtype)
    for t in range(9):
        kh, kw = divmod(t, 3)
        cols[:, :, t] = xp[:, :, kh:kh + ROWS, kw:kw + COLS]
    return cols.transpose(0, 3, 4, 1, 2).reshape(B * CELLS, C * 9)


def _col2im(dcols, B, C):
    d = dcols.reshape(B, ROWS, COLS, C, 9).transpose(0, 3, 4, 1, 2)
    dxp = np.zeros((B, C, ROWS + 2, COLS + 2), dcols.dtype)
    for t in range(9):
        kh, kw = divmod(t, 3)
        dxp[:, :, kh:kh + ROWS, kw:kw + COLS] += d[:, :, t]
    return dxp[:, :, 1:-1, 1:-1]


def train_step(params, adam_m, adam_v, step, x, pi, z, blocks, hidden=HIDDEN, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8,
               momentum=0.1, bn_eps=1e-5, masks=None, diag=None):
    """one optimizer step; returns (new params, m, v, loss[3], grads) — all float64.

    masks: optional per-conv-layer boolean [B][co][3][3] ReLU masks to use instead of
    (pre-activation > 0) — e.g. the device step's own (post-ReLU activation > 0), so
    that a pre-activation within rounding of 0 takes the same side of the kink in
    both.  diag: optional dict that receives the pre-activations ("pre", per layer)."""
    P, G, loss = forward_backward(params, x, pi, z, blocks, hidden, momentum, bn_eps, masks, diag)
    P, m, vv = adam(P, G, adam_m, adam_v, step, lr, b1, b2, eps)
    return P, m, vv, loss, G


def adam(P, G, adam_m, adam_v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """Adam (running statistics have zero gradient, so their moments stay 0 and they are not moved)"""
    m = b1 * np.asarray(adam_m, np.float64) + (1 - b1) * G
    vv = b2 * np.asarray(adam_v, np.float64) + (1 - b2) * G * G
    t = step + 1
    P = P - (lr / (1 - b1 ** t)) * m / (np.sqrt(vv) / np.sqrt(1 - b2 ** t) + eps)
    return P, m, vv


def forward_backward(params, x, pi, z, blocks, hidden=HIDDEN, momentum=0.1, bn_eps=1e-5, masks=None, diag=None):
    """train-mode forward + backward of one batch; returns (params with the BN running
    statistics updated, gradients, loss[3]) — float64"""
    convs, lin, n = _layout(blocks, hidden)
    P = np.asarray(params, np.float64).copy()
    assert len(P) == n
    G = np.zeros(n)
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    x = x.reshape(B, 3, ROWS, COLS)
    cache = [None] * len(convs)

    def conv_bn_act(l, inp, res=None):
        c = convs[l]
        ci, co = c["ci"], c["co"]
        W = P[c["w"]:c["w"] + co * ci * 9].reshape(co, ci * 9)
        cols = _im2col(inp)
        zz = (cols @ W.T + P[c["b"]:c["b"] + co]).reshape(B, ROWS, COLS, co).transpose(0, 3, 1, 2)
        mu = zz.mean((0, 2, 3))
        var = zz.var((0, 2, 3))
        nn_ = B * CELLS
        P[c["mu"]:c["mu"] + co] = (1 - momentum) * P[c["mu"]:c["mu"] + co] + momentum * mu
        P[c["var"]:c["var"] + co] = (1 - momentum) * P[c["var"]:c["var"] + co] + momentum * var * nn_ / (nn_ - 1)
        inv = 1.0 / np.sqrt(var + bn_eps)
        xhat = (zz - mu[None, :, None, None]) * inv[None, :, None, None]
        y = P[c["g"]:c["g"] + co][None, :, None, None] * xhat + P[c["be"]:c["be"] + co][None, :, None, None]
        if res is not None:
            y = y + res
        mask = (y > 0.0) if masks is None else np.asarray(masks[l], bool).reshape(y.shape)
        a = np.where(mask, y, 0.0)
        if diag is not None:
            diag.setdefault("pre", [None] * len(convs))[l] = y
        cache[l] = dict(cols=cols, W=W, xhat=xhat, inv=inv, a=a, m=mask)
        return a

    h = conv_bn_act(0, x)
    for k in range(blocks):
        r1 = conv_bn_act(1 + 2 * k, h)
        h = conv_bn_act(2 + 2 * k, r1, res=h)
    npol, nval = len(convs) - 2, len(convs) - 1
    rp = conv_bn_act(npol, h).reshape(B, -1)
    rv = conv_bn_act(nval, h).reshape(B, -1)
    Wp = P[lin["pw"]:lin["pw"] + ACTIONS * 32 * CELLS].reshape(ACTIONS, -1)
    Wv = P[lin["vw"]:lin["vw"] + 3 * CELLS].reshape(1, -1)
    logits = rp @ Wp.T + P[lin["pb"]:lin["pb"] + ACTIONS]
    pre = (rv @ Wv.T + P[lin["vb"]:lin["vb"] + 1]).reshape(-1)
    v = np.tanh(pre)
    lse = np.log(np.exp(logits - logits.max(1, keepdims=True)).sum(1)) + logits.max(1)
    logsm = logits - lse[:, None]
    pi = np.asarray(pi, np.float64).reshape(B, ACTIONS)
    zz_ = np.asarray(z, np.float64).reshape(-1)
    lp = -(logsm * pi).sum() / B
    lv = ((v - zz_) ** 2).mean()
    # backward
    dlogits = (np.exp(logsm) * pi.sum(1, keepdims=True) - pi) / B
    dpre = 2.0 * (v - zz_) / B * (1.0 - v * v)
    G[lin["pw"]:lin["pw"] + Wp.size] = (dlogits.T @ rp).reshape(-1)
    G[lin["pb"]:lin["pb"] + ACTIONS] = dlogits.sum(0)
    G[lin["vw"]:lin["vw"] + Wv.size] = (dpre[:, None].T @ rv).reshape(-1)
    G[lin["vb"]] = dpre.sum()

    def bn_conv_bwd(l, da, want_dx=True):
        c, cc = convs[l], cache[l]
        co, ci = c["co"], c["ci"]
        dy = da * cc["m"]
        xhat, inv = cc["xhat"], cc["inv"]
        nn_ = B * CELLS
        sb = dy.sum((0, 2, 3))
        sg = (dy * xhat).sum((0, 2, 3))
        G[c["be"]:c["be"] + co] = sb
        G[c["g"]:c["g"] + co] = sg
        gam = P[c["g"]:c["g"] + co]  # gamma is not changed by the forward
        dz = (gam * inv / nn_)[None, :, None, None] * (nn_ * dy - sb[None, :, None, None] - xhat * sg[None, :, None, None])
        dzf = dz.transpose(0, 2, 3, 1).reshape(B * CELLS, co)
        G[c["w"]:c["w"] + co * ci * 9] = (dzf.T @ cc["cols"]).reshape(-1)
        G[c["b"]:c["b"] + co] = dzf.sum(0)
        if not want_dx:
            return None
        return _col2im(dzf @ cc["W"], B, ci)

    dh = bn_conv_bwd(npol, (dlogits @ Wp).reshape(B, 32, ROWS, COLS))
    dh = dh + bn_conv_bwd(nval, (dpre[:, None] @ Wv).reshape(B, 3, ROWS, COLS))
    for k in reversed(range(blocks)):
        l1, l2 = 1 + 2 * k, 2 + 2 * k
        dt = dh * cache[l2]["m"]
        dr1 = bn_conv_bwd(l2, dt)
        dh = dt + bn_conv_bwd(l1, dr1)
    bn_conv_bwd(0, dh, want_dx=False)
    return P, G, np.array([lp + lv, lp, lv])


def train(params, batches, blocks, hidden=HIDDEN, **kw):
    """run train_step over [(x, pi, z), ...]; returns params, losses, grads of each step"""
    n = len(params)
    m, v = np.zeros(n), np.zeros(n)
    P = np.asarray(params, np.float64)
    losses, grads = [], []
    for k, (x, pi, z) in enumerate(batches):
        P, m, v, loss, g = train_step(P, m, v, k, x, pi, z, blocks, hidden, **kw)
        losses.append(loss)
        grads.append(g)
    return P, np.array(losses), grads


# ------------------------------------------------------------------ inputs shared by the golden and the tests
LINES = [0o7, 0o70, 0o700, 0o111, 0o222, 0o444, 0o421, 0o124]


def encode_moves(moves):
    """get_encoding (tictactoe.rs:199-216) of the position after `moves` from the
    empty board: the player to move's cells, the opponent's, the empty ones"""
    m = [0, 0]
    for k, c in enumerate(moves):
        m[k % 2] |= 1 << c
    mine, theirs = (m[0], m[1]) if len(moves) % 2 == 0 else (m[1], m[0])
    e = np.zeros(27, np.float32)
    for c in range(9):
        e[c] = (mine >> c) & 1
        e[9 + c] = (theirs >> c) & 1
        e[18 + c] = 1 - (((mine | theirs) >> c) & 1)
    return e


def random_games(n, rng):
    """n move lists of random legal play (0..7 plies) that leave the game ongoing,
    longest first (so the games still moving at ply k are a prefix of the list)"""
    out = []
    while len(out) < n:
        m, moves = [0, 0], []
        for k in range(int(rng.integers(0, 8))):
            free = [c for c in range(9) if not ((m[0] | m[1]) >> c) & 1]
            c = int(rng.choice(free))
            m[k % 2] |= 1 << c
            moves.append(c)
            if any((m[k % 2] & l) == l for l in LINES):
                moves = None
                break
        if moves is not None:
            out.append(moves)
    return sorted(out, key=len, reverse=True)


def make_batches(B, steps, seed):
    """(games, batches): steps x B positions of random legal play, random normalised pi,
    z in {-1, 0, 1}; batch k holds the positions of games[k*B:(k+1)*B] in a fixed shuffle"""
    rng = np.random.default_rng(seed)
    games = random_games(B * steps, rng)
    order = rng.permutation(B * steps)
    x = np.array([encode_moves(g) for g in games])[order]
    pi = rng.random((B * steps, 9)).astype(np.float32) ** 2
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice(np.array([-1, 0, 1], np.float32), B * steps)
    return games, order, [(x[k * B:(k + 1) * B], pi[k * B:(k + 1) * B], z[k * B:(k + 1) * B]) for k in range(steps)]


# ------------------------------------------------------------------ checks shared by the learner tests
def learner_masks(blocks, g_refs, rel=3e-3):
    """(well, running): parameters whose Adam updates are well conditioned at every
    step given (|grad| above rel * max|grad|, ten times the tests' gradient tolerance,
    so its sign is certain) and the BN running statistics.  Conv biases feeding a
    BatchNorm have a mathematically zero gradient: in fp32 it is rounding noise that
    Adam's g/(|g|+eps) turns into steps of up to lr, so those entries (and any entry
    whose gradient is that small at some step) are only bounded by lr.  The
    structure of test_oracle_golden.learner_masks, on this net's layout."""
    convs, lin, n = _layout(blocks)
    running = np.zeros(n, bool)
    for c in convs:
        running[c["mu"]:c["mu"] + c["co"]] = True
        running[c["var"]:c["var"] + c["co"]] = True
    well = ~running
    for g in g_refs:
        well &= np.abs(g) > rel * np.abs(g).max()
    return well, running


def check_learner_params(P, P_ref, g_refs, blocks, steps, lr=1e-3, tol=2e-5):
    """test_oracle_golden.check_learner_params on this net's layout.  g_refs: reference
    gradients of every step, or of step 1 only (then, for steps > 1, the bound holds
    for 99.9 % of the step-1 well-conditioned entries)"""
    well, running = learner_masks(blocks, g_refs)
    # BN running stats: exact functions of the batch statistics at step 1; later steps
    # inherit the pre-BN bias noise (a bias shifts the batch mean one-for-one)
    np.testing.assert_allclose(P[running], P_ref[running], rtol=1e-4, atol=1e-5 if steps == 1 else lr * steps)
    err = np.abs(P[well] - P_ref[well])
    if len(g_refs) >= steps:
        assert err.max() <= tol * steps, err.max()
    else:
        assert np.quantile(err, 0.999) <= tol * steps, np.quantile(err, 0.999)
    assert np.abs(P - P_ref).max() <= 2 * lr * steps + 1e-5                          # Adam step bound


def torch_net(params, blocks, momentum=0.1, bn_eps=1e-5):
    """the net in PyTorch CPU fp32 from the flat parameters (train mode; BatchNorm's
    momentum and eps as given); returns (forward(x) -> logits, value; the parameter
    tensors in flat order incl. running stats)"""
    import torch
    import torch.nn.functional as F
    convs, lin, n = _layout(blocks)
    p = torch.tensor(np.asarray(params, np.float32))
    T = []   # (tensor, offset) in flat order

    def leaf(off, shape, grad=True):
        t = p[off:off + int(np.prod(shape))].reshape(shape).clone().requires_grad_(grad)
        T.append((t, off))
        return t

    L = []
    for c in convs:
        L.append(dict(w=leaf(c["w"], (c["co"], c["ci"], 3, 3)), b=leaf(c["b"], (c["co"],)), g=leaf(c["g"], (c["co"],)),
                      be=leaf(c["be"], (c["co"],)), mu=leaf(c["mu"], (c["co"],), False),
                      var=leaf(c["var"], (c["co"],), False)))
    pw, pb = leaf(lin["pw"], (ACTIONS, 32 * CELLS)), leaf(lin["pb"], (ACTIONS,))
    vw, vb = leaf(lin["vw"], (1, 3 * CELLS)), leaf(lin["vb"], (1,))

    def cba(l, x, res=None):
        q = L[l]
        y = F.batch_norm(F.conv2d(x, q["w"], q["b"], padding=1), q["mu"], q["var"], q["g"], q["be"], True, momentum, bn_eps)
        return F.relu(y if res is None else y + res)

    def forward(x):
        h = cba(0, x)
        for k in range(blocks):
            h = cba(2 + 2 * k, cba(1 + 2 * k, h), res=h)
        rp = cba(len(L) - 2, h).flatten(1)
        rv = cba(len(L) - 1, h).flatten(1)
        return F.linear(rp, pw, pb), torch.tanh(F.linear(rv, vw, vb)).reshape(-1)

    return forward, T, n


def torch_train(params, batches, blocks, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, momentum=0.1, bn_eps=1e-5):
    """PyTorch CPU fp32: the same steps (torch.optim.Adam and BatchNorm at the given
    settings, the defaults being torch's); returns per step (loss[3], grads, params) as
    float32 arrays"""
    import torch
    forward, T, n = torch_net(params, blocks, momentum, bn_eps)
    opt = torch.optim.Adam([t for t, _ in T if t.requires_grad], lr=lr, betas=(b1, b2), eps=eps)
    out = []

    def flat(get):
        a = np.zeros(n, np.float32)
        for t, off in T:
            v = get(t)
            if v is not None:
                a[off:off + t.numel()] = v.detach().numpy().ravel()
        return a

    for x, pi, z in batches:
        x = torch.tensor(np.asarray(x, np.float32).reshape(-1, 3, ROWS, COLS))
        pi, z = torch.tensor(np.asarray(pi, np.float32)), torch.tensor(np.asarray(z, np.float32))
        logits, v = forward(x)
        lp = -(torch.log_softmax(logits, 1) * pi).sum() / x.shape[0]
        lv = ((v - z) ** 2).mean()
        opt.zero_grad()
        (lp + lv).backward()
        g = flat(lambda t: t.grad)
        opt.step()
        out.append((np.array([(lp + lv).item(), lp.item(), lv.item()], np.float32), g, flat(lambda t: t)))
    return out


def torch_fp32_distance(p0, batches, blocks, **kw):
    """chess_learner_ref.torch_fp32_distance for this net: how far PyTorch CPU fp32 lies
    from the restatement on the same steps at the settings kw (train's keywords): (loss,
    relative, worst step; gradient / max|g| at step 1; well-conditioned parameters,
    absolute, last step; running statistics, absolute, last step)"""
    P_ref, ref_losses, ref_grads = train(p0, batches, blocks, **kw)
    got = torch_train(p0, batches, blocks, **kw)
    el = max(np.abs(g[0] - r).max() / np.abs(r).max() for g, r in zip(got, ref_losses))
    eg = np.abs(got[0][1] - ref_grads[0]).max() / np.abs(ref_grads[0]).max()
    well, running = learner_masks(blocks, ref_grads)
    P = got[-1][2]
    return el, eg, np.abs(P[well] - P_ref[well]).max(), np.abs(P[running] - P_ref[running]).max()
