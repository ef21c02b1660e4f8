"""TEST INFRASTRUCTURE ONLY (the checker, never the product): the chess train step
of tests/chess_learner_ref.py restated in float64 with the bf16 compute type's
rounding points: every operand of every conv GEMM
(forward, data gradient, weight gradient; trunk and policy head) goes through
`round`; everything else works on the unrounded values.

Two forms:

  * step(): the whole step.  With round = identity it is
    chess_learner_ref.forward_backward (pinned to PyTorch float64 there).  With mm =
    one of F32_ORDERS and store = to_f32 it is a stand-in for a device: fp32 sums
    in some order, fp32 tensors in memory; `fault` plants a device's possible faults.
  * check_local(): the layer-local form.  Every GEMM is recomputed from the DEVICE's
    own tensors (its activations, its captured gradients), so a rounding flip in
    one layer cannot propagate into the comparison of the next; returns
    {name: (error, bar)}.

Rounding: float64 -> float32 (nearest) -> bf16 (nearest even), the device's
v_cvt_pk_bf16_f32 on its fp32 tensor.
"""
import numpy as np

from chess_learner_ref import _col2im, _im2col, _layout, adam, make_batches  # noqa: F401  (re-exported)

ROWS, COLS, CELLS, PLANES, HIDDEN, POLC, ACTIONS = 8, 8, 64, 19, 256, 73, 4672
HEAD_SHAPES = dict(p1w=(256, HIDDEN), p1b=(256,), p2w=(POLC, 256), p2b=(POLC,), vw=(1, HIDDEN), vb=(1,),
                   l1w=(256, CELLS), l1b=(256,), l2w=(1, 256), l2b=(1,))


# ------------------------------------------------------------------ rounding
def identity(x):
    return np.asarray(x, np.float64)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)


def _from_bits(u):
    return (u & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_round(x):
    """nearest even"""
    u = _bits(x)
    return _from_bits(u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1)))


def bf16_trunc(x):
    """toward zero: a planted fault"""
    return _from_bits(_bits(x))


def to_f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


# ------------------------------------------------------------------ GEMMs: float64, or fp32 sums in three orders
def mm64(a, b):
    return a @ b


def _mm32(a, b):
    return (np.asarray(a, np.float32) @ np.asarray(b, np.float32)).astype(np.float64)


def _mm32_chunks(a, b, k=144):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for i in range(0, a.shape[1], k):
        acc = acc + a[:, i:i + k] @ b[i:i + k]
    return acc.astype(np.float64)


def _mm32_reversed(a, b):
    return _mm32(np.ascontiguousarray(a[:, ::-1]), np.ascontiguousarray(b[::-1]))


F32_ORDERS = (_mm32, _mm32_chunks, _mm32_reversed)


# ------------------------------------------------------------------ layers
def _rows(t):
    """[B][C][8][8] -> rows (sample, cell) x C"""
    B, C = t.shape[:2]
    return t.reshape(B, C, CELLS).transpose(0, 2, 1).reshape(B * CELLS, C)


def _nchw(r, B):
    return r.reshape(B, ROWS, COLS, -1).transpose(0, 3, 1, 2)


def conv3_fwd(inp, W, b, round, mm, drop_tap=None):
    """inp [B][ci][8][8], W [co][ci*9] -> z [B][co][8][8] = conv(round(inp), round(W)) + b"""
    B = inp.shape[0]
    cols = _im2col(round(inp))
    if drop_tap is not None:
        cols = cols.copy()
        cols.reshape(B * CELLS, -1, 9)[:, :, drop_tap] = 0.0
    return _nchw(mm(cols, round(W).T) + b, B)


def conv3_dgrad(dz, W, ci, round, mm):
    B = dz.shape[0]
    return _col2im(mm(round(_rows(dz)), round(W)), B, ci)


def conv3_wgrad(dz, inp, round, mm):
    return mm(round(_rows(dz)).T, _im2col(round(inp)))


def bn_train(zz, gamma, beta, res, bn_eps):
    mu = zz.mean((0, 2, 3))
    var = zz.var((0, 2, 3))
    inv = 1.0 / np.sqrt(var + bn_eps)
    xhat = (zz - mu[None, :, None, None]) * inv[None, :, None, None]
    y = gamma[None, :, None, None] * xhat + beta[None, :, None, None]
    if res is not None:
        y = y + res
    return y, mu, var, xhat, inv


def bn_bwd(dy, xhat, inv, gamma):
    nn_ = dy.shape[0] * CELLS
    sb = dy.sum((0, 2, 3))
    sg = (dy * xhat).sum((0, 2, 3))
    bc = lambda v: v[None, :, None, None]   # noqa: E731
    dz = bc(gamma * inv / nn_) * (nn_ * dy - bc(sb) - xhat * bc(sg))
    return dz, sg, sb


def _heads(P, hd):
    return {k: P[hd[k]:hd[k] + int(np.prod(s))].reshape(s) for k, s in HEAD_SHAPES.items()}


def _softmax_loss(logits, pi, B):
    mx = logits.max(1, keepdims=True)
    logsm = logits - (np.log(np.exp(logits - mx).sum(1, keepdims=True)) + mx)
    return -(logsm * pi).sum() / B, (np.exp(logsm) * pi.sum(1, keepdims=True) - pi) / B


def _value_head(H, hf, zt, B, vc_mask=None, h1_mask=None, vc_given=None, h1_given=None):
    """the value head in float64 on unrounded tensors: forward, loss, gradients.
    *_given: use these activations (a device's) downstream instead of the head's own"""
    vc_pre = (hf @ H["vw"].T + H["vb"]).reshape(B, CELLS)
    mvc = vc_pre > 0 if vc_mask is None else vc_mask
    vc = np.where(mvc, vc_pre, 0.0) if vc_given is None else vc_given
    h1_pre = vc @ H["l1w"].T + H["l1b"]
    mh1 = h1_pre > 0 if h1_mask is None else h1_mask
    h1 = np.where(mh1, h1_pre, 0.0) if h1_given is None else h1_given
    v = np.tanh((h1 @ H["l2w"].T + H["l2b"]).reshape(-1))
    lv = ((v - zt) ** 2).mean()
    dpre = 2.0 * (v - zt) / B * (1.0 - v * v)
    g = dict(l2w=dpre[None, :] @ h1, l2b=dpre.sum(keepdims=True))
    dh1 = (dpre[:, None] * H["l2w"]) * mh1
    g["l1w"], g["l1b"] = dh1.T @ vc, dh1.sum(0)
    dvc = ((dh1 @ H["l1w"]) * mvc).reshape(B * CELLS, 1)
    g["vw"], g["vb"] = dvc.T @ hf, dvc.sum(keepdims=True)
    return dict(vc_pre=vc_pre, h1_pre=h1_pre, vc=vc, h1=h1, v=v, lv=lv, g=g, dhf=dvc @ H["vw"])


# ------------------------------------------------------------------ the whole step
def step(params, x, pi, z, blocks, round=identity, mm=mm64, store=identity, fault=None, gemm_params=None,
         wgrad_round=None, momentum=0.1, bn_eps=1e-5):
    """train-mode forward + backward of one batch.  Returns a record: P (the parameters
    with the running statistics updated), G, loss[3], and the tensors a device exposes:
    a (per trunk conv), ap1, vc, h1, logits, dz (per trunk conv), dp1, dlogits; plus pre.

    fault: None, "residual_bf16" (the residual add reads the rounded copy),
    "bn_bwd_rounded_z" (BatchNorm backward is fed the rounded pre-BN output),
    "corner_tap" (the forward convs drop tap 0).  wgrad_round: the rounding the
    weight gradient applies to dz instead of `round` (a fault).  gemm_params: the
    parameters the GEMMs read their weights from instead of `params` (a stale shadow)."""
    convs, hd, n = _layout(blocks)
    P = np.asarray(params, np.float64).copy()
    Pw = P if gemm_params is None else np.asarray(gemm_params, np.float64)
    assert len(P) == n
    G = np.zeros(n)
    B = len(x)
    x4 = np.asarray(x, np.float64).reshape(B, PLANES, ROWS, COLS)
    pi = np.asarray(pi, np.float64).reshape(B, ACTIONS)
    zt = np.asarray(z, np.float64).reshape(-1)
    nt = len(convs)
    wround = round if wgrad_round is None else wgrad_round
    drop = 0 if fault == "corner_tap" else None
    W = [Pw[c["w"]:c["w"] + c["co"] * c["ci"] * 9].reshape(c["co"], c["ci"] * 9) for c in convs]
    H, Hw = _heads(P, hd), _heads(Pw, hd)
    a, pre, cache, dzs = [None] * nt, [None] * nt, [None] * nt, [None] * nt

    def fwd(l, inp, res=None):
        c = convs[l]
        co = c["co"]
        zz = store(conv3_fwd(inp, W[l], P[c["b"]:c["b"] + co], round, mm, drop))
        if res is not None and fault == "residual_bf16":
            res = round(res)
        y, mu, var, xhat, inv = bn_train(zz, P[c["g"]:c["g"] + co], P[c["be"]:c["be"] + co], res, bn_eps)
        nn_ = B * CELLS
        P[c["mu"]:c["mu"] + co] = (1 - momentum) * P[c["mu"]:c["mu"] + co] + momentum * mu
        P[c["var"]:c["var"] + co] = (1 - momentum) * P[c["var"]:c["var"] + co] + momentum * var * nn_ / (nn_ - 1)
        if fault == "bn_bwd_rounded_z":
            xhat = (round(zz) - mu[None, :, None, None]) * inv[None, :, None, None]
        pre[l] = y
        a[l] = store(np.maximum(y, 0.0))
        cache[l] = dict(inp=inp, xhat=xhat, inv=inv, m=y > 0)
        return a[l]

    h = fwd(0, x4)
    for k in range(blocks):
        h = fwd(2 + 2 * k, fwd(1 + 2 * k, h), res=h)
    hf = _rows(h)
    p1_pre = mm(round(hf), round(Hw["p1w"]).T) + H["p1b"]
    mp1 = p1_pre > 0
    ap1 = store(np.where(mp1, p1_pre, 0.0))
    logits = store(_nchw(mm(round(ap1), round(Hw["p2w"]).T) + H["p2b"], B).reshape(B, ACTIONS))
    vh = _value_head(H, hf, zt, B)
    lp, dlogits = _softmax_loss(logits, pi, B)
    dlogits = store(dlogits)
    for k, v in vh["g"].items():
        G[hd[k]:hd[k] + v.size] = v.reshape(-1)
    dlg = _rows(dlogits.reshape(B, POLC, ROWS, COLS))
    G[hd["p2w"]:hd["p2w"] + POLC * 256] = mm(wround(dlg).T, round(ap1)).reshape(-1)
    G[hd["p2b"]:hd["p2b"] + POLC] = dlg.sum(0)
    dp1 = store(mm(round(dlg), round(Hw["p2w"])) * mp1)
    G[hd["p1w"]:hd["p1w"] + 256 * HIDDEN] = mm(wround(dp1).T, round(hf)).reshape(-1)
    G[hd["p1b"]:hd["p1b"] + 256] = dp1.sum(0)
    dh = _nchw(vh["dhf"] + mm(round(dp1), round(Hw["p1w"])), B)

    def bwd(l, da, want_dx=True):
        c, cc = convs[l], cache[l]
        co, ci = c["co"], c["ci"]
        dz, sg, sb = bn_bwd(da * cc["m"], cc["xhat"], cc["inv"], P[c["g"]:c["g"] + co])
        dz = dzs[l] = store(dz)
        G[c["g"]:c["g"] + co], G[c["be"]:c["be"] + co] = sg, sb
        G[c["b"]:c["b"] + co] = dz.sum((0, 2, 3))
        G[c["w"]:c["w"] + co * ci * 9] = mm(wround(_rows(dz)).T, _im2col(round(cc["inp"]))).reshape(-1)
        return conv3_dgrad(dz, W[l], ci, round, mm) if want_dx else None

    for k in reversed(range(blocks)):
        l1, l2 = 1 + 2 * k, 2 + 2 * k
        dt = dh * cache[l2]["m"]
        dh = dt + bwd(l1, store(bwd(l2, dt)))
    bwd(0, dh, want_dx=False)
    return dict(P=P, G=G, loss=np.array([lp + vh["lv"], lp, vh["lv"]]), a=a, pre=pre, ap1=_nchw(ap1, B),
                p1_pre=_nchw(p1_pre, B), vc=vh["vc"], h1=vh["h1"], logits=logits, dz=dzs, dp1=_nchw(dp1, B),
                dlogits=dlogits, value=vh["v"])


def train(params, batches, blocks, lr=1e-3, stale_at=None, **kw):
    """step() + Adam over [(x, pi, z), ...] -> (params, records).  stale_at: the step
    (0-based) whose GEMMs read the previous step's weights (a stale shadow)"""
    P = np.asarray(params, np.float64)
    m, v = np.zeros(len(P)), np.zeros(len(P))
    recs, prev = [], P
    for k, (x, pi, z) in enumerate(batches):
        rec = step(P, x, pi, z, blocks, gemm_params=prev if k == stale_at else None, **kw)
        rec["P0"] = P
        prev = P
        P, m, v = adam(rec["P"], rec["G"], m, v, k, lr)
        rec["P1"] = P
        recs.append(rec)
    return P, recs


# ------------------------------------------------------------------ the layer-local form
A_BAR, G_BAR = 1e-4, 3e-4     # the fp32 learner tests' bars: activations / flips, gradients
RUN_RTOL, RUN_ATOL = 1e-4, 1e-5
U32 = 2.0 ** -24              # fp32 unit roundoff


def zero_bias_bound(dy, zz, xhat, inv, gamma, dz, sg, sb):
    """per channel: how far from 0 an fp32 BatchNorm backward can leave the gradient of a
    conv bias that feeds a BatchNorm.  In exact arithmetic it is 0: sum dz = k (n sum dy -
    n sb - sg sum xhat), k = gamma invstd / n, with sb = sum dy and sum xhat = 0.  In
    fp32 (a kernel that sums a channel's n values as ceil(n / 256) sequential adds per
    thread and a tree of 8 levels, so d = ceil(n / 256) + 8 roundings deep; xhat =
    fl(fl(z - mean) invstd); dz = fl(k fl(fl(fl(n dy) - sb) - fl(xhat sg))), no
    contraction), to first order in u = 2^-24:

      |sb - sum dy|       <= d u sum|dy|
      |sum xhat|          <= invstd (d u sum|z| + u n |mean|) + 2 u sum|xhat|
                             (the computed mean's error, then xhat's two roundings)
      dz's own roundings  <= 4 u k (|n dy| + |sb| + |xhat sg|) per element
      the sum of dz       <= d u sum|dz|

    The bound is the sum of these, doubled for the second-order terms and for reading
    the quantities from this float64 recomputation and not from the device.  It comes
    from the number format alone; nothing of a device's output enters it."""
    ax = (0, 2, 3)
    n = dy.shape[0] * CELLS
    d = -(-n // 256) + 8
    k = np.abs(gamma * inv / n)
    bc = lambda v: v[None, :, None, None]   # noqa: E731
    e_sb = d * U32 * np.abs(dy).sum(ax)
    e_xh = inv * (d * U32 * np.abs(zz).sum(ax) + U32 * n * np.abs(zz.mean(ax))) + 2 * U32 * np.abs(xhat).sum(ax)
    e_dz = 4 * U32 * (n * np.abs(dy) + bc(np.abs(sb)) + np.abs(xhat * bc(sg))).sum(ax)
    return 2 * (k * (n * e_sb + np.abs(sg) * e_xh + e_dz) + d * U32 * np.abs(dz).sum(ax))


def check_local(p0, x, pi, z, blocks, dev, round=bf16_round, mm=mm64, momentum=0.1, bn_eps=1e-5):
    """every layer of one step recomputed in float64 from the device's own tensors,
    GEMM operands through `round`.  dev: a (per trunk conv [B][256][8][8]), ap1, vc
    [B][64], h1 [B][256], logits [B][4672], dz (per trunk conv), dp1, dlogits, G, P1
    (the parameters after the step: the running statistics are read), loss[3].
    Bars: A_BAR, G_BAR, RUN_* (the fp32 learner tests'), and zero_bias_bound for the conv
    biases' gradients ("zero_bias<l>": error = the worst channel's |g| / bound, bar 1).
    Returns {name: (error, bar)}; a check holds when error <= bar."""
    convs, hd, n = _layout(blocks)
    P = np.asarray(p0, np.float64)
    B = len(x)
    x4 = np.asarray(x, np.float64).reshape(B, PLANES, ROWS, COLS)
    pi = np.asarray(pi, np.float64).reshape(B, ACTIONS)
    zt = np.asarray(z, np.float64).reshape(-1)
    nt = len(convs)
    f = lambda t, shape=None: np.asarray(t, np.float64).reshape(shape if shape else np.shape(t))   # noqa: E731
    act = (B, HIDDEN, ROWS, COLS)
    a = [f(t, act) for t in dev["a"]]
    dzd = [f(t, act) for t in dev["dz"]]
    ap1, dp1 = f(dev["ap1"], act), f(dev["dp1"], act)
    vc, h1 = f(dev["vc"], (B, CELLS)), f(dev["h1"], (B, 256))
    logits, dlogits = f(dev["logits"], (B, ACTIONS)), f(dev["dlogits"], (B, ACTIONS))
    Gd, P1 = f(dev["G"]), f(dev["P1"])
    W = [P[c["w"]:c["w"] + c["co"] * c["ci"] * 9].reshape(c["co"], c["ci"] * 9) for c in convs]
    H = _heads(P, hd)
    out, G = {}, np.zeros(n)

    def put(name, got, ref, rel, scale=None):
        out[name] = (float(np.abs(got - ref).max()), rel * float(np.abs(ref).max() if scale is None else scale))

    def put_act(name, got, y):
        """a device activation against the pre-activation y under the device's own mask"""
        mask = got > 0
        s = float(np.abs(y).max())
        out[name] = (float(np.abs(got - np.where(mask, y, 0.0)).max()), A_BAR * s)
        diff = mask != (y > 0)
        out[name + ".flips"] = (float(np.abs(y[diff]).max()) if diff.any() else 0.0, A_BAR * s)
        return mask

    def put_close(name, got, ref, rtol, atol):
        out[name] = (float((np.abs(got - ref) - rtol * np.abs(ref)).max()), atol)

    # forward
    cache = [None] * nt
    for l, c in enumerate(convs):
        co = c["co"]
        inp = x4 if l == 0 else a[l - 1]
        res = a[l - 2] if l >= 2 and l % 2 == 0 else None
        zz = conv3_fwd(inp, W[l], P[c["b"]:c["b"] + co], round, mm)
        y, mu, var, xhat, inv = bn_train(zz, P[c["g"]:c["g"] + co], P[c["be"]:c["be"] + co], res, bn_eps)
        mask = put_act("a%d" % l, a[l], y)
        nn_ = B * CELLS
        put_close("run_mu%d" % l, P1[c["mu"]:c["mu"] + co], (1 - momentum) * P[c["mu"]:c["mu"] + co] + momentum * mu,
                  RUN_RTOL, RUN_ATOL)
        put_close("run_var%d" % l, P1[c["var"]:c["var"] + co],
                  (1 - momentum) * P[c["var"]:c["var"] + co] + momentum * var * nn_ / (nn_ - 1), RUN_RTOL, RUN_ATOL)
        cache[l] = dict(inp=inp, zz=zz, xhat=xhat, inv=inv, m=mask)
    hf = _rows(a[nt - 1])
    ap1r = _rows(ap1)
    mp1 = _rows(put_act("ap1", ap1, _nchw(mm(round(hf), round(H["p1w"]).T) + H["p1b"], B)))
    put("logits", logits, _nchw(mm(round(ap1r), round(H["p2w"]).T) + H["p2b"], B).reshape(B, ACTIONS), A_BAR)
    vh = _value_head(H, hf, zt, B, vc_mask=vc > 0, h1_mask=h1 > 0, vc_given=vc, h1_given=h1)
    put_act("vc", vc, vh["vc_pre"])
    put_act("h1", h1, vh["h1_pre"])
    lp, dlogits_ref = _softmax_loss(logits, pi, B)
    put_close("loss", f(dev["loss"]), np.array([lp + vh["lv"], lp, vh["lv"]]), 1e-4, 1e-5)
    # backward
    put("dlogits", dlogits, dlogits_ref, G_BAR)
    for k, v in vh["g"].items():
        G[hd[k]:hd[k] + v.size] = v.reshape(-1)
    dlg, dp1r = _rows(dlogits.reshape(B, POLC, ROWS, COLS)), _rows(dp1)
    G[hd["p2w"]:hd["p2w"] + POLC * 256] = mm(round(dlg).T, round(ap1r)).reshape(-1)
    G[hd["p2b"]:hd["p2b"] + POLC] = dlg.sum(0)
    put("dp1", dp1r, mm(round(dlg), round(H["p2w"])) * mp1, G_BAR)
    G[hd["p1w"]:hd["p1w"] + 256 * HIDDEN] = mm(round(dp1r).T, round(hf)).reshape(-1)
    G[hd["p1b"]:hd["p1b"] + 256] = dp1r.sum(0)
    dh = _nchw(vh["dhf"] + mm(round(dp1r), round(H["p1w"])), B)

    def bwd(l, da, want_dx=True):
        c, cc = convs[l], cache[l]
        co, ci = c["co"], c["ci"]
        dz_ref, sg, sb = bn_bwd(da * cc["m"], cc["xhat"], cc["inv"], P[c["g"]:c["g"] + co])
        put("dz%d" % l, dzd[l], dz_ref, G_BAR)
        # the conv bias feeds a BatchNorm: its gradient is 0 up to fp32 rounding, per channel
        bound = zero_bias_bound(da * cc["m"], cc["zz"], cc["xhat"], cc["inv"], P[c["g"]:c["g"] + co], dz_ref, sg, sb)
        out["zero_bias%d" % l] = (float((np.abs(Gd[c["b"]:c["b"] + co]) / bound).max()), 1.0)
        G[c["g"]:c["g"] + co], G[c["be"]:c["be"] + co] = sg, sb
        G[c["b"]:c["b"] + co] = dzd[l].sum((0, 2, 3))
        G[c["w"]:c["w"] + co * ci * 9] = conv3_wgrad(dzd[l], cc["inp"], round, mm).reshape(-1)
        return conv3_dgrad(dzd[l], W[l], ci, round, mm) if want_dx else None

    for k in reversed(range(blocks)):
        l1, l2 = 1 + 2 * k, 2 + 2 * k
        dt = dh * cache[l2]["m"]        # the skip path: unrounded
        dh = dt + bwd(l1, bwd(l2, dt))
    bwd(0, dh, want_dx=False)
    gmax = float(np.abs(G).max())
    for l, c in enumerate(convs):
        nw = c["co"] * c["ci"] * 9
        put("g_w%d" % l, Gd[c["w"]:c["w"] + nw], G[c["w"]:c["w"] + nw], G_BAR)
        for k in ("b", "g", "be"):
            put("g_%s%d" % (k, l), Gd[c[k]:c[k] + c["co"]], G[c[k]:c[k] + c["co"]], G_BAR, gmax)
    for k, s in HEAD_SHAPES.items():
        m = int(np.prod(s))
        put("g_" + k, Gd[hd[k]:hd[k] + m], G[hd[k]:hd[k] + m], G_BAR, None if k in ("p1w", "p2w") else gmax)
    return out


def failures(checks, factor=1.0):
    """the checks whose error exceeds factor x bar"""
    return {k: v for k, v in checks.items() if not v[0] <= factor * v[1]}


def device_record(rec):
    """a step() record as check_local's `dev` (the stand-in device of the CPU tests)"""
    return dict(a=rec["a"], ap1=rec["ap1"], vc=rec["vc"], h1=rec["h1"], logits=rec["logits"], dz=rec["dz"],
                dp1=rec["dp1"], dlogits=rec["dlogits"], G=rec["G"], P1=rec["P1"] if "P1" in rec else rec["P"],
                loss=rec["loss"])
