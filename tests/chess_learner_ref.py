"""TEST INFRASTRUCTURE ONLY (the checker, never the product): a numpy float64
restatement of the reference training step for the chess net
(model/chess.rs:48-70 under model/mod.rs:128-141), the sibling of
tests/ttt_learner_ref.py and oracle/learner_ref.py on an 8x8 board:

  * forward in train mode: stem conv3x3(19->256)+BN+ReLU, blocks
    relu(x + BN(conv(relu(BN(conv(x)))))); policy head conv1x1(256->256)+bias,
    ReLU, conv1x1(256->73)+bias, flattened NCHW (channel*64 + cell) into 4672
    logits; value head conv1x1(256->1)+bias, ReLU, linear 64->256, ReLU, linear
    256->1, tanh.  The heads have no BatchNorm.  BatchNorm: batch mean and biased
    variance over (B, 8, 8); running stats r <- 0.9 r + 0.1 stat with the
    unbiased variance.
  * loss = -(log_softmax(p) * pi).sum() / B + mean((v - z)^2)
  * backward, then Adam (beta 0.9/0.999, eps 1e-8, lr 1e-3, no weight decay).

Parameters are the flat vector of oracle/chessref.py::net_param_shapes
(= spai_chess_net_init_params).  Pinned against PyTorch float64 autograd and
chessref.net_forward in tests/test_chess_learner_cpu.py.  Same interface as
tests/ttt_learner_ref.py: train_step, train, masks=, diag=.

Activation layers (masks=, diag["pre"]): 0 .. 2*blocks the trunk convs
[B][256][8][8]; 2*blocks+1 the first policy conv [B][256][8][8]; 2*blocks+2 the
value conv [B][64]; 2*blocks+3 the first value linear [B][256].
"""
import numpy as np

ROWS, COLS, CELLS, PLANES, HIDDEN, POLC, ACTIONS = 8, 8, 64, 19, 256, 73, 4672


def _layout(blocks, hidden=HIDDEN):
    """(trunk convs, head offsets, size): offsets of every tensor in the flat parameter vector"""
    convs, off = [], 0

    def take(n):
        nonlocal off
        o = off
        off += n
        return o

    def conv(ci, co):
        c = dict(ci=ci, co=co, w=take(co * ci * 9), b=take(co))
        c["g"], c["be"], c["mu"], c["var"] = take(co), take(co), take(co), take(co)
        convs.append(c)

    conv(PLANES, hidden)
    for _ in range(2 * blocks):
        conv(hidden, hidden)
    head = dict(p1w=take(256 * hidden), p1b=take(256), p2w=take(POLC * 256), p2b=take(POLC), vw=take(hidden),
                vb=take(1), l1w=take(256 * CELLS), l1b=take(256), l2w=take(256), l2b=take(1))
    return convs, head, off


HEAD_SHAPES = dict(p1w=(256, HIDDEN), p1b=(256,), p2w=(POLC, 256), p2b=(POLC,), vw=(1, HIDDEN), vb=(1,),
                   l1w=(256, CELLS), l1b=(256,), l2w=(1, 256), l2b=(1,))


def _im2col(x):
    """[B][C][8][8] -> [B*64][C*9], column order (ci, kh, kw) = w.reshape(co, ci*9)"""
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


# hooks that tests/test_chess_learner_cpu.py replaces to plant a device kernel's possible faults
def _conv_cols(x):
    """the conv's gathered operand"""
    return _im2col(x)


def _head_bias(b):
    """the bias a head conv adds"""
    return b


def _bn_running_mean(old, mu, momentum):
    return (1 - momentum) * old + momentum * mu


def adam(P, G, adam_m, adam_v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """Adam (running statistics have zero gradient, so their moments stay 0 and they are not moved)"""
    m = b1 * np.asarray(adam_m, np.float64) + (1 - b1) * G
    vv = b2 * np.asarray(adam_v, np.float64) + (1 - b2) * G * G
    t = step + 1
    P = P - (lr / (1 - b1 ** t)) * m / (np.sqrt(vv) / np.sqrt(1 - b2 ** t) + eps)
    return P, m, vv


def train_step(params, adam_m, adam_v, step, x, pi, z, blocks, hidden=HIDDEN, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8,
               momentum=0.1, bn_eps=1e-5, masks=None, diag=None):
    """one optimizer step; returns (new params, m, v, loss[3], grads) — all float64.

    masks: optional per-layer boolean ReLU masks to use instead of (pre-activation > 0)
    — e.g. the device step's own (post-ReLU activation > 0).  diag: optional dict that
    receives the pre-activations ("pre", per layer)."""
    P, G, loss = forward_backward(params, x, pi, z, blocks, hidden, momentum, bn_eps, masks, diag)
    P, m, vv = adam(P, G, adam_m, adam_v, step, lr, b1, b2, eps)
    return P, m, vv, loss, G


def forward_backward(params, x, pi, z, blocks, hidden=HIDDEN, momentum=0.1, bn_eps=1e-5, masks=None, diag=None):
    """train-mode forward + backward of one batch; returns (params with the BN running
    statistics updated, gradients, loss[3]) — float64"""
    convs, hd, n = _layout(blocks, hidden)
    P = np.asarray(params, np.float64).copy()
    assert len(P) == n
    G = np.zeros(n)
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    x = x.reshape(B, PLANES, ROWS, COLS)
    nt = len(convs)
    cache = [None] * nt
    pre_all = [None] * (nt + 3)

    def H(name):
        shp = HEAD_SHAPES[name]
        return P[hd[name]:hd[name] + int(np.prod(shp))].reshape(shp)

    def setG(name, val):
        G[hd[name]:hd[name] + val.size] = val.reshape(-1)

    def relu(l, y):
        if masks is None:
            mask = y > 0.0
        elif l == nt:   # given as [B][256][8][8], used as rows (sample, cell)
            mask = np.asarray(masks[l], bool).reshape(B, 256, CELLS).transpose(0, 2, 1).reshape(y.shape)
        else:
            mask = np.asarray(masks[l], bool).reshape(y.shape)
        pre_all[l] = y
        return np.where(mask, y, 0.0), mask

    def conv_bn_act(l, inp, res=None):
        c = convs[l]
        ci, co = c["ci"], c["co"]
        W = P[c["w"]:c["w"] + co * ci * 9].reshape(co, ci * 9)
        cols = _conv_cols(inp)
        zz = (cols @ W.T + P[c["b"]:c["b"] + co]).reshape(B, ROWS, COLS, co).transpose(0, 3, 1, 2)
        mu = zz.mean((0, 2, 3))
        var = zz.var((0, 2, 3))
        nn_ = B * CELLS
        P[c["mu"]:c["mu"] + co] = _bn_running_mean(P[c["mu"]:c["mu"] + co], mu, momentum)
        P[c["var"]:c["var"] + co] = (1 - momentum) * P[c["var"]:c["var"] + co] + momentum * var * nn_ / (nn_ - 1)
        inv = 1.0 / np.sqrt(var + bn_eps)
        xhat = (zz - mu[None, :, None, None]) * inv[None, :, None, None]
        y = P[c["g"]:c["g"] + co][None, :, None, None] * xhat + P[c["be"]:c["be"] + co][None, :, None, None]
        if res is not None:
            y = y + res
        a, mask = relu(l, y)
        cache[l] = dict(cols=cols, W=W, xhat=xhat, inv=inv, a=a, m=mask)
        return a

    h = conv_bn_act(0, x)
    for k in range(blocks):
        r1 = conv_bn_act(1 + 2 * k, h)
        h = conv_bn_act(2 + 2 * k, r1, res=h)
    hf = h.transpose(0, 2, 3, 1).reshape(B * CELLS, hidden)         # rows (sample, cell)
    # policy head
    ap1, mp1 = relu(nt, hf @ H("p1w").T + _head_bias(H("p1b")))     # [B*64][256]
    lg = ap1 @ H("p2w").T + _head_bias(H("p2b"))                    # [B*64][73]
    logits = lg.reshape(B, CELLS, POLC).transpose(0, 2, 1).reshape(B, ACTIONS)
    # value head
    vc, mvc = relu(nt + 1, (hf @ H("vw").T + _head_bias(H("vb"))).reshape(B, CELLS))
    h1, mh1 = relu(nt + 2, vc @ H("l1w").T + H("l1b"))
    v = np.tanh((h1 @ H("l2w").T + H("l2b")).reshape(-1))
    pre_all[nt] = pre_all[nt].reshape(B, ROWS, COLS, 256).transpose(0, 3, 1, 2)
    if diag is not None:
        diag["pre"] = pre_all
        diag["logits"], diag["value"] = logits, v
    mx = logits.max(1, keepdims=True)
    logsm = logits - (np.log(np.exp(logits - mx).sum(1, keepdims=True)) + mx)
    pi = np.asarray(pi, np.float64).reshape(B, ACTIONS)
    zz_ = np.asarray(z, np.float64).reshape(-1)
    lp = -(logsm * pi).sum() / B
    lv = ((v - zz_) ** 2).mean()
    # backward: value head
    dpre = 2.0 * (v - zz_) / B * (1.0 - v * v)
    setG("l2w", dpre[None, :] @ h1)
    setG("l2b", dpre.sum(keepdims=True))
    dh1 = (dpre[:, None] * H("l2w")) * mh1
    setG("l1w", dh1.T @ vc)
    setG("l1b", dh1.sum(0))
    dvc = ((dh1 @ H("l1w")) * mvc).reshape(B * CELLS, 1)
    setG("vw", dvc.T @ hf)
    setG("vb", dvc.sum(keepdims=True))
    dhf = dvc @ H("vw")
    # policy head
    dlogits = (np.exp(logsm) * pi.sum(1, keepdims=True) - pi) / B
    dlg = dlogits.reshape(B, POLC, CELLS).transpose(0, 2, 1).reshape(B * CELLS, POLC)
    setG("p2w", dlg.T @ ap1)
    setG("p2b", dlg.sum(0))
    dzp1 = (dlg @ H("p2w")) * mp1
    setG("p1w", dzp1.T @ hf)
    setG("p1b", dzp1.sum(0))
    dhf = dhf + dzp1 @ H("p1w")
    dh = dhf.reshape(B, ROWS, COLS, hidden).transpose(0, 3, 1, 2)

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

    for k in reversed(range(blocks)):
        l1, l2 = 1 + 2 * k, 2 + 2 * k
        dt = dh * cache[l2]["m"]
        dr1 = bn_conv_bwd(l2, dt)
        dh = dt + bn_conv_bwd(l1, dr1)
    bn_conv_bwd(0, dh, want_dx=False)
    return P, G, np.array([lp + lv, lp, lv])


def eval_forward(params, blocks, x, hidden=HIDDEN, bn_eps=1e-5):
    """Net::forward(x, train=false) with this module's own arithmetic: the running
    statistics normalise; -> logits [B][4672], value [B]"""
    convs, hd, n = _layout(blocks, hidden)
    P = np.asarray(params, np.float64)
    x = np.asarray(x, np.float64).reshape(-1, PLANES, ROWS, COLS)
    B = x.shape[0]

    def H(name):
        shp = HEAD_SHAPES[name]
        return P[hd[name]:hd[name] + int(np.prod(shp))].reshape(shp)

    def cba(l, inp, res=None):
        c = convs[l]
        ci, co = c["ci"], c["co"]
        W = P[c["w"]:c["w"] + co * ci * 9].reshape(co, ci * 9)
        zz = (_conv_cols(inp) @ W.T + P[c["b"]:c["b"] + co]).reshape(B, ROWS, COLS, co).transpose(0, 3, 1, 2)
        s = P[c["g"]:c["g"] + co] / np.sqrt(P[c["var"]:c["var"] + co] + bn_eps)
        y = (zz - P[c["mu"]:c["mu"] + co][None, :, None, None]) * s[None, :, None, None] + \
            P[c["be"]:c["be"] + co][None, :, None, None]
        return np.maximum(y if res is None else y + res, 0.0)

    h = cba(0, x)
    for k in range(blocks):
        h = cba(2 + 2 * k, cba(1 + 2 * k, h), res=h)
    hf = h.transpose(0, 2, 3, 1).reshape(B * CELLS, hidden)
    ap1 = np.maximum(hf @ H("p1w").T + _head_bias(H("p1b")), 0.0)
    logits = (ap1 @ H("p2w").T + _head_bias(H("p2b"))).reshape(B, CELLS, POLC).transpose(0, 2, 1).reshape(B, ACTIONS)
    vc = np.maximum((hf @ H("vw").T + _head_bias(H("vb"))).reshape(B, CELLS), 0.0)
    h1 = np.maximum(vc @ H("l1w").T + H("l1b"), 0.0)
    return logits, np.tanh((h1 @ H("l2w").T + H("l2b")).reshape(-1))


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


# ------------------------------------------------------------------ inputs shared by the tests
def random_games(n, rng, max_plies=24):
    """n move lists of random legal play from the start position (0..max_plies plies,
    through oracle/chessref.py on the CPU) that leave the game ongoing, longest first
    (so the games still moving at ply k are a prefix of the list)"""
    import chessref
    out = []
    while len(out) < n:
        s, moves = chessref.ChessState(), []
        for _ in range(int(rng.integers(0, max_plies + 1))):
            legal = s.valid_actions()
            m = int(legal[int(rng.integers(0, len(legal)))])
            moves.append(m)
            s = s.next_state(m)
            if s.status != 0:
                moves = None
                break
        if moves is not None:
            out.append(moves)
    return sorted(out, key=len, reverse=True)


def play(moves):
    """the oracle state after `moves` from the start position"""
    import chessref
    s = chessref.ChessState()
    for m in moves:
        s = s.next_state(m)
    return s


def make_batches(B, steps, seed, max_plies=24):
    """(games, order, batches): steps x B positions of random legal play (so planes
    16-18, the counters, are not binary); pi random and normalised over each position's
    legal moves at policy_index(side, move), zero elsewhere; z in {-1, 0, 1}; batch k
    holds the positions of games[k*B:(k+1)*B] in a fixed shuffle"""
    import chessref
    rng = np.random.default_rng(seed)
    n = B * steps
    games = random_games(n, rng, max_plies)
    order = rng.permutation(n)
    x = np.zeros((n, PLANES * CELLS), np.float32)
    pi = np.zeros((n, ACTIONS), np.float32)
    for i, g in enumerate(games):
        s = play(g)
        x[i] = s.encoding().reshape(-1)
        idx = np.array([chessref.policy_index(s.side, m) for m in s.valid_actions()])
        assert len(np.unique(idx)) == len(idx)
        w = rng.random(len(idx)) ** 2 + 1e-3
        pi[i, idx] = (w / w.sum()).astype(np.float32)
    chessref.arena_reset()
    x, pi = x[order], pi[order]
    z = rng.choice(np.array([-1, 0, 1], np.float32), n)
    return games, order, [(x[k * B:(k + 1) * B], pi[k * B:(k + 1) * B], z[k * B:(k + 1) * B]) for k in range(steps)]


# ------------------------------------------------------------------ checks shared by the learner tests
def learner_masks(blocks, g_refs, rel=3e-3):
    """(well, running): as ttt_learner_ref.learner_masks on this net's layout.  Conv
    biases feeding a BatchNorm have a mathematically zero gradient, so they (and every
    entry whose gradient is below rel * max|g| at some step) are only bounded by lr."""
    convs, hd, n = _layout(blocks)
    running = np.zeros(n, bool)
    for c in convs:
        running[c["mu"]:c["mu"] + c["co"]] = True
        running[c["var"]:c["var"] + c["co"]] = True
    well = ~running
    for g in g_refs:
        well &= np.abs(g) > rel * np.abs(g).max()
    return well, running


def check_learner_params(P, P_ref, g_refs, blocks, steps, lr=1e-3, tol=2e-5, run_atol=None):
    """ttt_learner_ref.check_learner_params on this net's layout.  run_atol: the absolute
    bar of the running statistics (default 1e-5 at step 1, lr * steps later)"""
    well, running = learner_masks(blocks, g_refs)
    if run_atol is None:
        run_atol = 1e-5 if steps == 1 else lr * steps
    np.testing.assert_allclose(P[running], P_ref[running], rtol=1e-4, atol=run_atol)
    err = np.abs(P[well] - P_ref[well])
    if len(g_refs) >= steps:
        assert err.max() <= tol * steps, err.max()
    else:
        assert np.quantile(err, 0.999) <= tol * steps, np.quantile(err, 0.999)
    assert np.abs(P - P_ref).max() <= 2 * lr * steps + 1e-5                          # Adam step bound


def torch_net(params, blocks, dtype=None, momentum=0.1, bn_eps=1e-5):
    """the net in PyTorch on the CPU from the flat parameters (train mode; BatchNorm's
    momentum and eps as given); returns
    (forward(x) -> logits, value; the parameter tensors in flat order incl. running stats)"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    convs, hd, n = _layout(blocks)
    p = torch.tensor(np.asarray(params, np.float64), dtype=dtype)
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
    Hd = {}
    for name in ("p1w", "p1b", "p2w", "p2b", "vw", "vb", "l1w", "l1b", "l2w", "l2b"):
        shp = HEAD_SHAPES[name]
        if name in ("p1w", "p2w", "vw"):
            shp = shp + (1, 1)
        Hd[name] = leaf(hd[name], shp)

    def cba(l, x, res=None):
        q = L[l]
        y = F.batch_norm(F.conv2d(x, q["w"], q["b"], padding=1), q["mu"], q["var"], q["g"], q["be"], True, momentum, bn_eps)
        return F.relu(y if res is None else y + res)

    def forward(x):
        h = cba(0, x)
        for k in range(blocks):
            h = cba(2 + 2 * k, cba(1 + 2 * k, h), res=h)
        pol = F.conv2d(F.relu(F.conv2d(h, Hd["p1w"], Hd["p1b"])), Hd["p2w"], Hd["p2b"]).flatten(1)
        val = F.relu(F.conv2d(h, Hd["vw"], Hd["vb"])).flatten(1)
        val = torch.tanh(F.linear(F.relu(F.linear(val, Hd["l1w"], Hd["l1b"])), Hd["l2w"], Hd["l2b"]))
        return pol, val.reshape(-1)

    return forward, T, n


def torch_train(params, batches, blocks, lr=1e-3, dtype=None, b1=0.9, b2=0.999, eps=1e-8, momentum=0.1, bn_eps=1e-5):
    """PyTorch CPU autograd (float64 by default): the same steps (torch.optim.Adam and
    BatchNorm at the given settings, the defaults being torch's); returns per step
    (loss[3], grads, params) as float64 arrays"""
    import torch
    dtype = dtype or torch.float64
    forward, T, n = torch_net(params, blocks, dtype, momentum, bn_eps)
    opt = torch.optim.Adam([t for t, _ in T if t.requires_grad], lr=lr, betas=(b1, b2), eps=eps)
    out = []

    def flat(get):
        a = np.zeros(n, np.float64)
        for t, off in T:
            v = get(t)
            if v is not None:
                a[off:off + t.numel()] = v.detach().numpy().ravel()
        return a

    for x, pi, z in batches:
        x = torch.tensor(np.asarray(x, np.float64).reshape(-1, PLANES, ROWS, COLS), dtype=dtype)
        pi = torch.tensor(np.asarray(pi, np.float64), dtype=dtype)
        z = torch.tensor(np.asarray(z, np.float64), dtype=dtype)
        logits, v = forward(x)
        lp = -(torch.log_softmax(logits, 1) * pi).sum() / x.shape[0]
        lv = ((v - z) ** 2).mean()
        opt.zero_grad()
        (lp + lv).backward()
        g = flat(lambda t: t.grad)
        opt.step()
        out.append((np.array([(lp + lv).item(), lp.item(), lv.item()]), g, flat(lambda t: t)))
    return out


def torch_fp32_distance(p0, batches, blocks, **kw):
    """how far PyTorch CPU fp32 lies from this restatement on the same steps at the
    settings kw (train's keywords; none: the defaults): (loss,
    relative, worst step; gradient / max|g| at step 1, the step whose gradient the GPU
    test checks; well-conditioned parameters, absolute, last step; running statistics,
    absolute, last step) — the measurement behind the bars of
    tests/test_chess_learner_gpu.py"""
    import torch
    P_ref, ref_losses, ref_grads = train(p0, batches, blocks, **kw)
    got = torch_train(p0, batches, blocks, dtype=torch.float32, **kw)
    el = max(np.abs(g[0] - r).max() / np.abs(r).max() for g, r in zip(got, ref_losses))
    eg = np.abs(got[0][1] - ref_grads[0]).max() / np.abs(ref_grads[0]).max()
    well, running = learner_masks(blocks, ref_grads)
    P = got[-1][2]
    return el, eg, np.abs(P[well] - P_ref[well]).max(), np.abs(P[running] - P_ref[running]).max()
