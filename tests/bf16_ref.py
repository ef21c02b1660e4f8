"""Reference restatements of the two fused bf16 forwards (net_c4.hip k_forward,
chess_net.hip k_chess_forward) in numpy float64, with the kernels' quantisation
points ("Quantisation points of the fused forwards"), plus the
parameter builders the net tests share.

Connect4 (and, with other dims, the TicTacToe net: same architecture):
  * BN folded in fp32 exactly as fold(): scale = g / sqrtf(var + 1e-5f),
    w' = w * scale, b' = (b - mu) * scale + beta;
  * folded weights -> bf16 (round to nearest even, f2bf); biases stay fp32;
  * every conv: fp32 sum starting from the bias (+ the bf16 block input for the
    second conv of a block) -> bf16 -> ReLU;
  * head features relu(bf16); the two linears on bf16 weights, fp32 sums, the
    fp32 bias added last; tanh on the value; softmax, then the legal-move mask.
Chess:
  * fold in double (conv_bn / pack_conv): sc = g / sqrt((double)var + 1e-5),
    w' = (float)(w * sc) -> bf16, b' = (float)((b - mu) * sc + beta);
  * input planes -> bf16; trunk as above; p1 and p2 (1x1) on bf16 weights, the
    p1 output -> bf16 -> ReLU, the p2 output (the logits) fp32;
  * value head in fp32 on the bf16 trunk output: v_w, l1_w, l2_w unrounded.

Options of both forwards:
  quant=False      the plain float64 net (no rounding anywhere);
  acc=np.float32   fp32 accumulation in chunks of `chunk` K indices, the K order
                   permuted by `korder` (a seed): "another fp32 summation order";
  mutate=[...]     deliberately wrong references, to prove a test is sensitive:
                     ("drop_tap", layer, cell, tap)   one 3x3 term of one output cell
                     ("zero_bias", layer, channel)    one channel's folded bias
                     ("swap_cells", layer, c1, c2)    two cells of a layer's output
  exact=True       assert that nothing rounds: the fold reproduces the intended
                   dyadic values, every pre-rounding activation is a bf16 number
                   and every sum's |terms| stay below 2^24 units of their common
                   LSB (so any fp32 summation order gives the same bits).
Layer names: Connect4 "stem", "res0" .. "res{2*blocks-1}", "head" (32 policy + 3
value channels); chess "stem", "res{i}", "p1", "p2", "v".
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = np.float32(1e-5)
# running variance of the exact-arithmetic nets: var + 1e-5f == 1.0f in fp32, so the
# folded scale is gamma itself
EXACT_VAR = np.float32(np.float32(1) - np.float32(1e-5))
assert np.float32(EXACT_VAR + EPS32) == np.float32(1)
ULP_TOL = dict(rtol=0, atol=2e-7)   # tanhf against float64 tanh (tests/test_gpu_fp32.py)


# ---------------------------------------------------------------- bf16
def bf16_bits(a):
    """f2bf of net_c4.hip / chess_net.hip on a float32 array: round to nearest even;
    inf stays, a NaN keeps its sign and top payload bits and is quietened."""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    special = (u & 0x7F800000) == 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    spc = (u >> 16) | np.where(u & 0xFFFF, 0x40, 0).astype(np.uint64)
    return np.where(special, spc, rne).astype(np.uint16)


def bf16_round(a):
    """a -> the nearest bf16 numbers, as float64.  A float64 input goes through fp32
    first, as the device's fp32 accumulators do."""
    bits = bf16_bits(np.asarray(a, F64).astype(F32))
    return (bits.astype(np.uint32) << 16).view(F32).astype(F64)


def _lsb(*arrays):
    """the largest power of two that divides every non-zero value of the arrays"""
    e = 1 << 20
    for a in arrays:
        v = np.asarray(a, F64).ravel()
        v = v[v != 0]
        if v.size == 0:
            continue
        assert np.all(np.isfinite(v))
        m, ex = np.frexp(v)
        M = np.abs(m * 2.0 ** 53).astype(np.int64)
        tz = np.log2((M & -M).astype(F64)).astype(np.int64)
        e = min(e, int((ex - 53 + tz).min()))
    return 2.0 ** e if e != (1 << 20) else 1.0


# ---------------------------------------------------------------- layouts
def _conv_bn(L, name, ci, co):
    L += [(name + ".w", (co, ci, 3, 3)), (name + ".b", (co,)), (name + ".g", (co,)), (name + ".be", (co,)),
          (name + ".mu", (co,)), (name + ".var", (co,))]


def c4_layout(blocks, hidden=64, dims=(3, 6, 7, 7)):
    """flat parameter order of the Connect4 / TicTacToe net (spai_net_num_params)"""
    C, H, W, A = dims
    L = []
    _conv_bn(L, "stem", C, hidden)
    for i in range(2 * blocks):
        _conv_bn(L, "res%d" % i, hidden, hidden)
    _conv_bn(L, "pol", hidden, 32)
    L += [("pol_lin.w", (A, 32 * H * W)), ("pol_lin.b", (A,))]
    _conv_bn(L, "val", hidden, 3)
    L += [("val_lin.w", (1, 3 * H * W)), ("val_lin.b", (1,))]
    return L


def chess_layout(blocks, hidden=256):
    """flat parameter order of the chess net (chessref.net_param_shapes)"""
    L = []
    _conv_bn(L, "stem", 19, hidden)
    for i in range(2 * blocks):
        _conv_bn(L, "res%d" % i, hidden, hidden)
    L += [("p1.w", (256, hidden, 1, 1)), ("p1.b", (256,)), ("p2.w", (73, 256, 1, 1)), ("p2.b", (73,)),
          ("v.w", (1, hidden, 1, 1)), ("v.b", (1,)), ("l1.w", (256, 64)), ("l1.b", (256,)),
          ("l2.w", (1, 256)), ("l2.b", (1,))]
    return L


def layout_size(layout):
    return sum(int(np.prod(s)) for _, s in layout)


def unflatten(params, layout):
    """name -> view of the flat vector"""
    params = np.asarray(params)
    out, off = {}, 0
    for name, shp in layout:
        n = int(np.prod(shp))
        out[name] = params[off:off + n].reshape(shp)
        off += n
    assert off == params.size, (off, params.size)
    return out


def flatten(d, layout):
    return np.concatenate([np.asarray(d[name], F32).reshape(-1) for name, _ in layout]).astype(F32)


_LINEAR_BIASES = ("pol_lin.b", "val_lin.b", "l1.b", "l2.b")


def trained_like(params, layout, seed):
    """A deterministic function of an init_params vector that looks like a trained
    net where the init is degenerate: every conv bias (the chess 1x1 convs' too), BN
    beta and running mean becomes +-U(0.1, 0.3), the running variance log-uniform in
    [0.5, 2], gamma U(0.5, 1.5) with every 11th channel negated.  Weights and the
    linear biases (already non-zero at init) are kept."""
    rng = np.random.default_rng(seed)
    out = np.array(params, F32, copy=True)
    d = unflatten(out, layout)
    for name, shp in layout:
        n = int(np.prod(shp))
        kind = name.split(".")[1]
        if (kind == "b" and name not in _LINEAR_BIASES) or kind in ("be", "mu"):
            d[name][...] = (rng.uniform(0.1, 0.3, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
        elif kind == "var":
            d[name][...] = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n)).astype(F32)
        elif kind == "g":
            g = rng.uniform(0.5, 1.5, n)
            g[5::11] *= -1.0
            d[name][...] = g.astype(F32)
    return out


# ---------------------------------------------------------------- the arithmetic
class _Ctx:
    def __init__(self, quant, acc, korder, chunk, mutate, exact, cache=None):
        self.quant, self.acc, self.korder, self.chunk, self.exact = quant, np.dtype(acc), korder, chunk, exact
        # cache: a dict that an unmutated run fills with every layer's output (and the folded
        # weights) and that mutated runs of the same net and inputs resume from
        self.cache, self.dirty = cache, False
        if mutate and isinstance(mutate[0], str):
            mutate = [mutate]
        self.mutate = [tuple(m) for m in (mutate or ())]
        for m in self.mutate:
            assert m[0] in ("drop_tap", "zero_bias", "swap_cells"), m
        self.used = set()
        self.max_act = 0.0     # largest |pre-rounding activation| (reported by the exactness tests)
        self.max_units = 0.0   # largest sum of |terms| in units of the terms' LSB

    def mut(self, kind, layer):
        out = [m for m in self.mutate if m[0] == kind and m[1] == layer]
        self.used.update(out)
        return out

    def done(self):
        assert self.used == set(self.mutate), "mutation names no layer of this net: %r" % (set(self.mutate) - self.used,)

    def order(self, K, layer):
        if self.korder is None:
            return np.arange(K)
        return np.random.default_rng([self.korder, K, sum(map(ord, layer))]).permutation(K)

    def gemm(self, layer, P2, W2, bias, res=None, bias_last=False):
        """P2 [M][K] x W2 [K][co] + bias (+ res [M][co])"""
        bias = np.asarray(bias, F64)
        if self.exact:
            absum = np.abs(P2) @ np.abs(W2) + np.abs(bias)
            if res is not None:
                absum = absum + np.abs(res)
            unit = min(_lsb(P2) * _lsb(W2), _lsb(bias), _lsb(res) if res is not None else 1.0)
            units = float(absum.max()) / unit
            assert units < 2.0 ** 24, "%s: sum of |terms| = %g units of 2^%d: an fp32 order could round" % (
                layer, units, int(np.log2(unit)))
            self.max_units = max(self.max_units, units)
        if self.acc == np.dtype(F64):
            out = P2 @ W2 + bias
            return out + res if res is not None else out
        M, K = P2.shape
        idx = self.order(K, layer)
        out = np.zeros((M, W2.shape[1]), F32) if bias_last else np.broadcast_to(bias.astype(F32), (M, W2.shape[1]))
        for s in range(0, K, self.chunk):
            j = idx[s:s + self.chunk]
            out = (out.astype(F64) + P2[:, j] @ W2[j]).astype(F32)
        if res is not None:
            out = (out.astype(F64) + res).astype(F32)
        if bias_last:
            out = (out.astype(F64) + bias.astype(F32)).astype(F32)
        return out.astype(F64)

    def conv(self, layer, a, hw, w, b, res=None, relu=True, round_out=True):
        """a [N][cells][ci], w [co][ci][k][k] and b [co] as the kernel holds them
        -> [N][cells][co]; cell = row * W + col, tap = (dh + 1) * 3 + (dw + 1)"""
        H, W = hw
        N, cells, ci = a.shape
        co, k = w.shape[0], w.shape[2]
        mutated = any(m[1] == layer for m in self.mutate)
        if self.cache is not None and self.mutate and not self.dirty and not mutated:
            return self.cache[layer]   # upstream of every mutation
        self.dirty = self.dirty or mutated
        w, b = np.asarray(w, F64), np.array(b, F64)
        for m in self.mut("zero_bias", layer):
            b[m[2]] = 0.0
        drops = self.mut("drop_tap", layer)
        if not w.any():   # an all-zero conv: the bias (the identity-trunk nets have many)
            pre = np.broadcast_to(b, (N, cells, co)) + (res if res is not None else 0.0)
        else:
            p = k // 2
            ap = np.zeros((N, H + 2 * p, W + 2 * p, ci))
            ap[:, p:p + H, p:p + W] = a.reshape(N, H, W, ci)
            P = np.stack([ap[:, dy:dy + H, dx:dx + W] for dy in range(k) for dx in range(k)], 3)
            P = P.reshape(N, cells, k * k, ci)
            for m in drops:
                P[:, m[2], m[3], :] = 0.0
            W2 = w.transpose(2, 3, 1, 0).reshape(k * k * ci, co)
            r2 = res.reshape(N * cells, co) if res is not None else None
            pre = self.gemm(layer, P.reshape(N * cells, k * k * ci), W2, b, r2).reshape(N, cells, co)
        if self.quant and round_out:
            q = bf16_round(pre)
            if self.exact:
                assert np.array_equal(q, pre), "%s: a pre-rounding activation is no bf16 number (max |act| %g)" % (
                    layer, np.abs(pre).max())
                self.max_act = max(self.max_act, float(np.abs(pre).max()))
            pre = q
        out = np.maximum(pre, 0.0) if relu else np.array(pre)
        for m in self.mut("swap_cells", layer):
            out = np.array(out)
            out[:, [m[2], m[3]]] = out[:, [m[3], m[2]]]
        if self.cache is not None and not self.mutate:
            self.cache[layer] = out
        return out


def _fold32(p, name, ctx):
    """fold() of net_c4.hip: fp32 throughout"""
    w, b, g, be, mu, var = (np.asarray(p[name + s], F32) for s in (".w", ".b", ".g", ".be", ".mu", ".var"))
    scale = (g / np.sqrt(var + EPS32)).astype(F32)
    wf = (w * scale[:, None, None, None]).astype(F32) if w.any() else w
    bf = ((b - mu).astype(F32) * scale).astype(F32)
    bf = (bf + be).astype(F32)
    if ctx.exact:
        assert np.array_equal(scale, g), "%s: var + eps != 1, the scale is not gamma" % name
        _assert_fold_exact(name, w, b, g, be, mu, wf, bf)
    return wf.astype(F64), bf.astype(F64)


def _fold64(p, name, ctx, to_f32):
    """conv_bn of chess_net.hip: double, the results stored as fp32 (to_f32), or the
    plain float64 fold of the unquantised nets"""
    w, b, g, be, mu, var = (np.asarray(p[name + s], F32).astype(F64) for s in (".w", ".b", ".g", ".be", ".mu", ".var"))
    sc = g / np.sqrt(var + 1e-5)
    wf = w * sc[:, None, None, None] if w.any() else w
    bf = (b - mu) * sc + be
    if to_f32:
        wf, bf = wf.astype(F32).astype(F64), bf.astype(F32).astype(F64)
    if ctx.exact:
        _assert_fold_exact(name, w, b, g, be, mu, wf, bf)
    return wf, bf


def _assert_fold_exact(name, w, b, g, be, mu, wf, bf):
    w, b, g, be, mu = (np.asarray(v, F64) for v in (w, b, g, be, mu))
    assert np.array_equal(wf, w * g[:, None, None, None]), "%s: folded weights are not w * gamma" % name
    assert np.array_equal(bf, (b - mu) * g + be), "%s: folded bias is not (b - mu) * gamma + beta" % name
    assert np.array_equal(bf16_round(wf), wf), "%s: folded weights are no bf16 numbers" % name


def _q(ctx, a):
    return bf16_round(a) if ctx.quant else np.asarray(a, F64)


def _memo(cache, fold):
    """the folded, rounded (weights, bias) of a layer, kept in the cache between runs"""
    def get(ctx, name):
        key = ("fold", name)
        if cache is not None and key in cache:
            return cache[key]
        w, b = fold(name)
        w = _q(ctx, w)
        if cache is not None:
            cache[key] = (w, b)
        return w, b
    return get


def c4_forward(params, blocks, x, quant=True, acc=F64, korder=None, chunk=32, mutate=(), exact=False,
               dims=(3, 6, 7, 7), hidden=64, info=None, cache=None):
    """x [N][C][H][W] -> logits [N][A], value [N] (float64 arrays)"""
    C, H, W, A = dims
    ctx = _Ctx(quant, acc, korder, chunk, mutate, exact, cache)
    p = unflatten(np.asarray(params, F32), c4_layout(blocks, hidden, dims))
    fold = _memo(cache, (lambda n: _fold32(p, n, ctx)) if quant else (lambda n: _fold64(p, n, ctx, False)))
    x = np.asarray(x, F64).reshape(-1, C, H * W)
    N, hw = x.shape[0], (H, W)
    a = _q(ctx, x.transpose(0, 2, 1))
    if exact:
        assert np.array_equal(a, x.transpose(0, 2, 1))
    a = ctx.conv("stem", a, hw, *fold(ctx, "stem"))
    for i in range(blocks):
        y = ctx.conv("res%d" % (2 * i), a, hw, *fold(ctx, "res%d" % (2 * i)))
        a = ctx.conv("res%d" % (2 * i + 1), y, hw, *fold(ctx, "res%d" % (2 * i + 1)), res=a)
    (pw, pb), (vw, vb) = fold(ctx, "pol"), fold(ctx, "val")
    h = ctx.conv("head", a, hw, np.concatenate([pw, vw]), np.concatenate([pb, vb]))
    hp = h[:, :, :32].transpose(0, 2, 1).reshape(N, -1)   # the reference's flatten: channel * cells + cell
    hv = h[:, :, 32:].transpose(0, 2, 1).reshape(N, -1)
    lw, vlw = _q(ctx, p["pol_lin.w"]), _q(ctx, p["val_lin.w"])
    if exact:
        assert np.array_equal(lw, p["pol_lin.w"]) and np.array_equal(vlw, p["val_lin.w"])
    logits = ctx.gemm("pol_lin", hp, lw.T, p["pol_lin.b"], bias_last=True)
    v = ctx.gemm("val_lin", hv, vlw.T, p["val_lin.b"], bias_last=True)
    if exact:
        assert np.array_equal(logits.astype(F32).astype(F64), logits)
    ctx.done()
    if info is not None:
        info.update(max_act=ctx.max_act, max_units=ctx.max_units, pre_tanh=v[:, 0])
    return logits, np.tanh(v[:, 0])


def chess_forward(params, blocks, x, quant=True, acc=F64, korder=None, chunk=32, mutate=(), exact=False, info=None,
                  cache=None):
    """x [N][19][8][8] -> logits [N][4672] (channel * 64 + cell), value [N]"""
    ctx = _Ctx(quant, acc, korder, chunk, mutate, exact, cache)
    p = unflatten(np.asarray(params, F32), chess_layout(blocks))
    fold = _memo(cache, lambda n: _fold64(p, n, ctx, quant))
    x = np.asarray(x, F64).reshape(-1, 19, 64)
    N, hw = x.shape[0], (8, 8)
    a = _q(ctx, x.transpose(0, 2, 1))
    if exact:
        assert np.array_equal(a, x.transpose(0, 2, 1))
    a = ctx.conv("stem", a, hw, *fold(ctx, "stem"))
    for i in range(blocks):
        y = ctx.conv("res%d" % (2 * i), a, hw, *fold(ctx, "res%d" % (2 * i)))
        a = ctx.conv("res%d" % (2 * i + 1), y, hw, *fold(ctx, "res%d" % (2 * i + 1)), res=a)
    w1, w2 = _q(ctx, p["p1.w"]), _q(ctx, p["p2.w"])
    if exact:
        assert np.array_equal(w1, p["p1.w"]) and np.array_equal(w2, p["p2.w"])
    p1 = ctx.conv("p1", a, hw, w1, p["p1.b"])
    lg = ctx.conv("p2", p1, hw, w2, p["p2.b"], relu=False, round_out=False)
    logits = lg.transpose(0, 2, 1).reshape(N, 73 * 64)
    vc = ctx.conv("v", a, hw, p["v.w"], p["v.b"], round_out=False)[:, :, 0]   # fp32 weights, no rounding
    h = np.maximum(ctx.gemm("l1", vc, np.asarray(p["l1.w"], F64).T, p["l1.b"]), 0.0)
    v = ctx.gemm("l2", h, np.asarray(p["l2.w"], F64).T, p["l2.b"])
    if exact:
        assert np.array_equal(logits.astype(F32).astype(F64), logits)
    ctx.done()
    if info is not None:
        info.update(max_act=ctx.max_act, max_units=ctx.max_units, pre_tanh=v[:, 0])
    return logits, np.tanh(v[:, 0])


# ---------------------------------------------------------------- Connect4 positions and predict
def c4_random_states(n, max_plies, seed):
    """(x, o, n, 0) after random column drops (bit col * 7 + row, row 0 at the bottom;
    a four in a row is not looked for: the net does not care).  Full columns occur."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bb, height = [0, 0], [0] * 7
        plies = int(rng.integers(0, max_plies + 1))
        for ply in range(plies):
            cols = [c for c in range(7) if height[c] < 6]
            c = cols[int(rng.integers(len(cols)))]
            bb[ply & 1] |= 1 << (c * 7 + height[c])
            height[c] += 1
        out.append((bb[0], bb[1], plies, 0))
    return out


def c4_encode(states):
    """the reference's encoding (connect_four.rs:242-259): planes [mine, theirs, empty]"""
    x = np.zeros((len(states), 3, 6, 7), F32)
    for i, (bx, bo, n, _) in enumerate(states):
        mine, theirs = (bx, bo) if n % 2 == 0 else (bo, bx)
        for r in range(6):
            for c in range(7):
                bit = 1 << (c * 7 + r)
                x[i, 0 if mine & bit else 1 if theirs & bit else 2, r, c] = 1.0
    return x


def c4_legal(states):
    return np.array([[((bx | bo) >> (7 * a + 5)) & 1 == 0 for a in range(7)] for bx, bo, _, _ in states])


def softmax_mask(logits, legal):
    """Model::predict in float64: softmax, mask, renormalise"""
    z = np.asarray(logits, F64)
    e = np.exp(z - z.max(1, keepdims=True))
    m = e / e.sum(1, keepdims=True) * legal
    return m / m.sum(1, keepdims=True)


# ---------------------------------------------------------------- exact-arithmetic nets
TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def tap_on_board(cell, tap, H, W):
    dh, dw = TAPS[tap]
    return 0 <= cell // W + dh < H and 0 <= cell % W + dw < W


def _blank(layout):
    d = {name: np.zeros(shp, F32) for name, shp in layout}
    for name in d:
        if name.endswith(".g"):
            d[name][...] = 1.0
        elif name.endswith(".var"):
            d[name][...] = EXACT_VAR
    return d


def _shift(d, name, tap, rng, ci_used=None):
    """conv `name` := output channel co takes input channel perm[co] at `tap`, sign
    +1, or -1 with bias 1 (1 - x on 0/1 inputs: ReLU keeps it)"""
    w = d[name + ".w"]
    co, ci = w.shape[:2]
    ci_used = ci if ci_used is None else ci_used
    perm = (rng.permutation(max(co, ci_used)) % ci_used)[:co]
    neg = rng.random(co) < 0.4
    w[...] = 0.0
    w[np.arange(co), perm, tap // 3, tap % 3] = np.where(neg, -1.0, 1.0)
    d[name + ".b"][...] = np.where(neg, 1.0, 0.0)


def _centre_identity(d, name):
    w = d[name + ".w"]
    w[...] = 0.0
    w[np.arange(w.shape[0]), np.arange(w.shape[0]), 1, 1] = 1.0


def _ternary(rng, shape, density=2.0 / 3.0):
    """{-1, 0, +1}, the signs equally likely"""
    return (rng.choice([-1.0, 1.0], shape) * (rng.random(shape) < density)).astype(F32)


def _c4_lift_stem(d, C=3):
    """the stem lifts the input planes into distinct 0/1/2-valued channels: channel c
    = plane c % 3 at tap (c // 3) % 9; channels 27..53 negated (1 - x); channels
    54.. add the next plane's centre tap"""
    w, b = d["stem.w"], d["stem.b"]
    for c in range(w.shape[0]):
        t = (c // 3) % 9
        w[c, c % C, t // 3, t % 3] = -1.0 if 27 <= c < 54 else 1.0
        if 27 <= c < 54:
            b[c] = 1.0
        if c >= 54:
            w[c, (c + 1) % C, 1, 1] += 1.0


def _c4_select_head(d, hidden=64):
    """head conv := centre-tap selections of 35 distinct trunk channels"""
    for c in range(32):
        d["pol.w"][c, (c * 37 + 5) % hidden, 1, 1] = 1.0
    for c in range(3):
        d["val.w"][c, ((32 + c) * 37 + 5) % hidden, 1, 1] = 1.0


def _c4_linears(d, rng, pol_shift=10, val_shift=9):
    """integer weights, the 7 (or 1) of a (channel, cell) feature distinct from every
    other feature's, scaled by a power of two so that softmax and tanh stay sensitive"""
    A, K = d["pol_lin.w"].shape
    while True:
        w = rng.integers(-127, 128, (A, K))
        if len({tuple(c) for c in w.T}) == K:
            break
    d["pol_lin.w"][...] = w * 2.0 ** -pol_shift
    d["pol_lin.b"][...] = rng.integers(-8, 9, A) / 8.0
    kv = d["val_lin.w"].shape[1]
    d["val_lin.w"][0] = (rng.permutation(kv) - kv // 2) * 2.0 ** -val_shift
    d["val_lin.b"][0] = 0.25


C4_SHIFT_LAYERS = {   # probe name -> (blocks, probed layer)
    "stem": (0, "stem"), "block_conv1": (1, "res0"), "block_conv2": (2, "res3"),
    "deep_first": (6, "res0"), "deep_middle": (6, "res5"), "deep_last": (6, "res11"), "head": (1, "head")}


def c4_shift_probe(which, tap, seed=0):
    """-> (params, blocks, probed layer).  An identity trunk (all-zero convs) around
    one conv that is a pure shift by `tap` with a channel permutation and signs."""
    blocks, layer = C4_SHIFT_LAYERS[which]
    rng = np.random.default_rng([seed, tap, sum(map(ord, which))])
    layout = c4_layout(blocks)
    d = _blank(layout)
    if layer == "stem":
        _shift(d, "stem", tap, rng)
    else:
        _c4_lift_stem(d)
    if layer == "head":
        _shift(d, "pol", tap, rng)
        _shift(d, "val", tap, rng)
    else:
        _c4_select_head(d)
    if layer.startswith("res"):
        i = int(layer[3:])
        _shift(d, layer, tap, rng)
        _centre_identity(d, "res%d" % (i ^ 1))   # the block's other conv passes it on
    _c4_linears(d, rng)
    return flatten(d, layout), blocks, layer


C4_DENSE_KINDS = ("stem", "conv1", "conv2", "head", "linears")


def c4_dense_probe(kind, seed=0):
    """-> (params, blocks, probed layer or None).  One layer kind with dense ternary
    weights over every (co, ci, tap); the layers after it only select."""
    blocks = {"stem": 0, "conv1": 1, "conv2": 1, "head": 0, "linears": 0}[kind]
    rng = np.random.default_rng([seed, sum(map(ord, kind))])
    layout = c4_layout(blocks)
    d = _blank(layout)
    layer = {"stem": "stem", "conv1": "res0", "conv2": "res1", "head": "head", "linears": None}[kind]
    if kind == "stem":
        d["stem.w"][...] = _ternary(rng, d["stem.w"].shape)
        d["stem.b"][...] = rng.integers(-2, 3, 64)
    else:
        _c4_lift_stem(d)
    if kind in ("conv1", "conv2"):
        d[layer + ".w"][...] = _ternary(rng, d[layer + ".w"].shape)
        d[layer + ".b"][...] = rng.integers(-2, 3, 64)
        _centre_identity(d, "res1" if kind == "conv1" else "res0")
    if kind == "head":
        d["pol.w"][...] = _ternary(rng, d["pol.w"].shape)
        d["val.w"][...] = _ternary(rng, d["val.w"].shape)
        d["pol.b"][...] = rng.integers(-2, 3, 32)
    else:
        _c4_select_head(d)
    if kind == "linears":
        d["pol_lin.w"][...] = _ternary(rng, d["pol_lin.w"].shape) * 2.0 ** -4
        d["val_lin.w"][...] = _ternary(rng, d["val_lin.w"].shape) * 2.0 ** -3
        d["pol_lin.b"][...] = rng.integers(-8, 9, 7) / 8.0
    else:
        _c4_linears(d, rng, pol_shift=13 if kind != "stem" else 12, val_shift=11)
    return flatten(d, layout), blocks, layer


def _fold_layer(d, name, rng, density, gammas, frac, cover=True, off_in=()):
    """sparse ternary weights under non-trivial dyadic BN / bias parameters, different in
    every channel and layer, built so that every channel's folded bias shows downstream:
    * a tenth of the output channels have no weights, their bias alone decides the ReLU
      (some positive, some negative);
    * the others read the input channels in turn at random taps with a folded weight of
      +|gamma| (so a live input opens them), plus the sparse ternary terms;
    * the folded bias is +(frac |gamma| + frac k), k = 1..2, or, for a quarter of the
      channels with |gamma| >= 1, the small negative -(frac |gamma| + frac);
    * conv bias, running mean and beta are all non-zero: b - mu = +-frac, and beta has the
      sign of (b - mu) gamma (the double-precision fold of the chess net then still gives
      the intended fp32 number)."""
    w = d[name + ".w"]
    co, ci = w.shape[:2]
    g = rng.choice(gammas, co)
    w[...] = _ternary(rng, w.shape, density)
    dead = rng.random(co) < 0.1
    dead[:2] = [True, False]
    w[dead] = 0.0
    live, perm = np.flatnonzero(~dead), rng.permutation(ci)
    for c in range(max(len(live), ci) if cover else len(live)):
        t = int(rng.integers(9))
        w[live[c % len(live)], perm[c % ci], t // 3, t % 3] = np.sign(g[live[c % len(live)]])
    neg = np.where(dead, rng.random(co) < 0.5, (rng.random(co) < 0.25) & (np.abs(g) >= 1))
    neg[0] = True
    for o in live:   # a channel that reads nothing but constant zeros (off_in) gets a positive bias
        if not np.delete(w[o], list(off_in), 0).any():
            neg[o] = False
    fb = np.where(neg, -(frac * np.abs(g) + frac), frac * np.abs(g) + frac * rng.integers(1, 3, co))
    bm = np.sign(fb) * np.sign(g) * frac             # b - mu
    mu = bm * rng.choice([1.0, 2.0, -2.0, -3.0], co)
    d[name + ".g"][...] = g
    d[name + ".mu"][...] = mu
    d[name + ".b"][...] = mu + bm
    d[name + ".be"][...] = fb - bm * g
    assert np.all(d[name + ".b"] != 0) and np.all(mu != 0) and np.all(d[name + ".be"] * bm * g > 0)
    return np.flatnonzero(dead & neg)   # the channels that are zero whatever the input


# seeds at which every channel's folded bias is seen in the outputs (tests/test_bf16_ref_cpu.py
# checks it): with sparse weights a few channels of most nets feed only closed ReLUs
FOLD_SEEDS = {("c4", 0): 0, ("c4", 1): 3, ("c4", 2): 12, ("chess", 0): 0, ("chess", 1): 1}


def c4_fold_probe(blocks, seed=None):
    """-> (params, blocks).  Every conv with non-zero dyadic conv bias, beta, mean and a
    gamma in {+-1, +-2, 0.5}.  With blocks the activations need 7 integer bits, so there
    the parameters are multiples of 1/2 and no gamma is 0.5 (one fraction bit, not two),
    and the head's gammas are +-1."""
    seed = FOLD_SEEDS[("c4", blocks)] if seed is None else seed
    rng = np.random.default_rng([seed, blocks, 77])
    layout = c4_layout(blocks)
    d = _blank(layout)
    half = [0.5] if blocks == 0 else []
    frac = 0.25 if blocks == 0 else 0.5
    two = [2.0, -2.0] if blocks == 0 else []
    off = trunk = _fold_layer(d, "stem", rng, 0.08, [1.0, -1.0, 2.0, -2.0] + 2 * half, 0.5)
    for i in range(2 * blocks):
        off = _fold_layer(d, "res%d" % i, rng, 0.002 if blocks < 2 else 0.001,
                          [1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -2.0 if blocks < 2 else -1.0], frac, off_in=off)
        if i & 1:   # the block's output is zero where its input and its second conv both are
            off = trunk = np.intersect1d(off, trunk)
    _fold_layer(d, "pol", rng, 0.004, [1.0, -1.0] + two + half, frac, off_in=off)
    _fold_layer(d, "val", rng, 0.008, [1.0, -1.0] + two[1:] + half, frac, cover=False, off_in=off)   # (pol reads every channel)
    _c4_linears(d, rng, pol_shift=13, val_shift=11)
    return flatten(d, layout), blocks


# ---- chess
def _chess_lift_stem(d):
    """channel c = plane c % 19 at tap (c // 19) % 9; channels 128.. negated (1 - x)"""
    w, b = d["stem.w"], d["stem.b"]
    for c in range(w.shape[0]):
        t = (c // 19) % 9
        w[c, c % 19, t // 3, t % 3] = -1.0 if c >= 128 else 1.0
        if c >= 128:
            b[c] = 1.0


def _chess_heads(d, rng, select=True):
    """p1 := a signed channel permutation (the trunk's channels stay distinguishable),
    p2 := small integers distinct per (policy channel, p1 channel) column, biases
    non-zero; the value head on dyadic fp32 weights"""
    if select:
        perm = rng.permutation(256)
        d["p1.w"][np.arange(256), perm, 0, 0] = 1.0
        d["p1.b"][...] = rng.integers(0, 3, 256)
    while True:
        w = rng.integers(-7, 8, (73, 256))
        if len({tuple(c) for c in w.T}) == 256:
            break
    d["p2.w"][:, :, 0, 0] = w * 2.0 ** -4
    d["p2.b"][...] = rng.integers(-8, 9, 73) / 8.0
    d["v.w"][0, :, 0, 0] = rng.choice([-3, -2, -1, 1, 2, 3], 256) / 16.0
    d["v.b"][0] = 0.5
    d["l1.w"][...] = rng.integers(-3, 4, (256, 64)) / 16.0
    d["l1.b"][...] = rng.integers(-4, 5, 256) / 8.0
    d["l2.w"][...] = rng.integers(-3, 4, (1, 256)) / 64.0
    d["l2.b"][0] = -0.125


CHESS_SHIFT_LAYERS = {
    "stem": (0, "stem"), "block_conv1": (1, "res0"), "block_conv2": (2, "res3"),
    "deep_first": (6, "res0"), "deep_middle": (6, "res5"), "deep_last": (6, "res11"),
    "deep20_middle": (20, "res20")}


def chess_shift_probe(which, tap, seed=0):
    blocks, layer = CHESS_SHIFT_LAYERS[which]
    rng = np.random.default_rng([seed, tap, sum(map(ord, which)), 5])
    layout = chess_layout(blocks)
    d = _blank(layout)
    if layer == "stem":
        _shift(d, "stem", tap, rng)
    else:
        _chess_lift_stem(d)
        _shift(d, layer, tap, rng)
        _centre_identity(d, "res%d" % (int(layer[3:]) ^ 1))
    _chess_heads(d, rng)
    return flatten(d, layout), blocks, layer


CHESS_DENSE_KINDS = ("stem", "conv1", "conv2", "p1", "p2", "value")


def chess_dense_probe(kind, seed=0):
    blocks = 1 if kind in ("conv1", "conv2") else 0
    rng = np.random.default_rng([seed, sum(map(ord, kind)), 6])
    layout = chess_layout(blocks)
    d = _blank(layout)
    layer = {"stem": "stem", "conv1": "res0", "conv2": "res1", "p1": "p1", "p2": "p2", "value": "v"}[kind]
    if kind == "stem":
        d["stem.w"][...] = _ternary(rng, d["stem.w"].shape)
        d["stem.b"][...] = rng.integers(-2, 3, 256)
    else:
        _chess_lift_stem(d)
    if kind in ("conv1", "conv2"):
        d[layer + ".w"][...] = _ternary(rng, d[layer + ".w"].shape)
        d[layer + ".b"][...] = rng.integers(-2, 3, 256)
        _centre_identity(d, "res1" if kind == "conv1" else "res0")
    _chess_heads(d, rng, select=kind != "p1")
    if kind == "p1":
        d["p1.w"][...] = _ternary(rng, d["p1.w"].shape)
        d["p1.b"][...] = rng.integers(-2, 3, 256)
    if kind == "p2":
        d["p2.w"][...] = _ternary(rng, d["p2.w"].shape)
    if kind == "value":
        d["v.w"][...] = _ternary(rng, d["v.w"].shape) / 8.0
        d["l1.w"][...] = _ternary(rng, d["l1.w"].shape) / 8.0
        d["l2.w"][...] = _ternary(rng, d["l2.w"].shape) / 16.0
    if kind in ("stem", "conv1", "conv2"):   # large trunk outputs: keep tanh off saturation
        d["v.w"][...] /= 16.0
    return flatten(d, layout), blocks, layer


def chess_fold_probe(blocks, seed=None):
    seed = FOLD_SEEDS[("chess", blocks)] if seed is None else seed
    rng = np.random.default_rng([seed, blocks, 78])
    layout = chess_layout(blocks)
    d = _blank(layout)
    off = trunk = _fold_layer(d, "stem", rng, 0.02, [1.0, -1.0, 2.0, -2.0, 0.5, 0.5], 0.5)
    for i in range(2 * blocks):
        off = _fold_layer(d, "res%d" % i, rng, 0.0005, [1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -2.0], 0.25, off_in=off)
        if i & 1:
            off = trunk = np.intersect1d(off, trunk)
    _chess_heads(d, rng)
    # the 1x1 convs' biases: none zero (p1's not below -1/2: a trunk channel that is 1 here and
    # 0 without its bias must still open the p1 channel that selects it)
    b = rng.integers(-2, 9, 256)
    d["p1.b"][...] = np.where(b == 0, 1, b) / 4.0
    sel = np.argmax(d["p1.w"][:, :, 0, 0], 1)            # a p1 channel that selects a constant-zero trunk
    fix = np.isin(sel, off)                               # channel shows its bias only if that is positive
    d["p1.b"][fix] = np.abs(d["p1.b"][fix])
    b = rng.integers(-8, 9, 73)
    d["p2.b"][...] = np.where(b == 0, 1, b) / 8.0
    # the trunk's large constant channels would close the value conv's ReLU everywhere (v_b
    # would not show): v_b := minus the median of the value conv's sums on the probe inputs
    params = flatten(d, layout)
    cache = {}
    chess_forward(params, blocks, chess_probe_inputs()[:3], cache=cache)
    trunk_out = cache["res%d" % (2 * blocks - 1)] if blocks else cache["stem"]
    med = np.median(trunk_out @ d["v.w"][0, :, 0, 0].astype(F64))
    d["v.b"][0] = -np.round(2 * med) / 2 + 0.5
    return flatten(d, layout), blocks


def binary_planes(n, planes, H, W, seed, density=0.5):
    """0/1 inputs; every cell is set in some position and plane"""
    x = (np.random.default_rng(seed).random((n, planes, H, W)) < density).astype(F32)
    assert x.any((0, 1)).all()
    return x


# ---------------------------------------------------------------- the inputs the exact probes share
C4_PREDICT_UNIQUE = 61   # prime: tiled over a batch, every position meets every slot of every group size


def c4_probe_inputs():
    """-> (x [24 + 61][3][6][7], states): 24 arbitrary 0/1 plane sets (forward only) and
    the encodings of 61 positions (forward and predict)"""
    states = c4_random_states(C4_PREDICT_UNIQUE, 36, seed=11)
    x = np.concatenate([binary_planes(24, 3, 6, 7, seed=12), c4_encode(states)])
    return x, states


def chess_probe_inputs(n=5):
    return binary_planes(n, 19, 8, 8, seed=13)


# ---------------------------------------------------------------- the bound of the trained-parameter tests
def spread_bound(forward, params, blocks, x, korders=(1, 2, 3), chunk=1, **kw):
    """(The fp32 emulations add one product at a time, chunk = 1, in a permuted K order: the
    plain sequential fp32 sum; the chess tests take chunks of 4 over their K = 2304, for time.  Chunks of 32 that are summed exactly inside understate the
    noise of the short sums, the 126-feature value linear above all.)
    The device is one more fp32 summation order of the sums this module restates, so
    its distance from the fp64-accumulated emulation is a draw from the distribution of
    the distances of other fp32 orders; bf16 rounding flips are rare and discrete, the
    maximum heavy-tailed, hence 4 x the largest of three.
    -> dict(logits, value: the fp64-accumulated emulation; spread_l, spread_v; bound_l =
    4 spread_l; bound_v = 4 spread_v + 2e-7, tanhf's own error; cache)"""
    cache = {}
    lg, v = forward(params, blocks, x, cache=cache, **kw)
    sl = sv = 0.0
    for k in korders:
        l2, v2 = forward(params, blocks, x, acc=F32, korder=k, chunk=chunk, **kw)
        sl, sv = max(sl, float(np.abs(l2 - lg).max())), max(sv, float(np.abs(v2 - v).max()))
    return dict(logits=lg, value=v, spread_l=sl, spread_v=sv, bound_l=4 * sl, bound_v=4 * sv + ULP_TOL["atol"],
                cache=cache)


def trained_cases(blocks, ref):
    """the two subtly wrong kernels the bound must resolve: the corner tap of the last
    trunk conv (the stem without blocks) dropped at the corner cell; that conv's largest
    folded bias zeroed.  (The largest, because a tolerance cannot see every channel: at
    two blocks the median channel's bias moves the logits by about twice the bound, the
    smallest by less than it.  Every channel's bias is pinned by the exact fold probes.)"""
    layer = "res%d" % (2 * blocks - 1) if blocks else "stem"
    ch = int(np.argmax(np.abs(ref["cache"][("fold", layer)][1])))
    return [("drop_tap", layer, 0, 8), ("zero_bias", layer, ch)]


def mutation_effects(forward, params, blocks, x, ref, cases, **kw):
    """max |dlogit| of each mutated reference"""
    return [float(np.abs(forward(params, blocks, x, mutate=m, cache=ref["cache"], **kw)[0] - ref["logits"]).max())
            for m in cases]


def check_bound_conditions(forward, params, blocks, x, ref, **kw):
    """the two conditions on the bound, from the reference alone -> the effects"""
    eff = mutation_effects(forward, params, blocks, x, ref, trained_cases(blocks, ref), **kw)
    old_bar = 3e-2 * max(1.0, float(np.abs(ref["logits"]).max()))
    assert ref["spread_l"] > 0
    assert ref["bound_l"] <= min(eff) / 3, (ref["bound_l"], eff)
    assert ref["bound_l"] < old_bar, (ref["bound_l"], old_bar)
    return eff


# ---------------------------------------------------------------- the probe registry (CPU and GPU tests)
TAP_CENTRE = 4
C4_PROBES = ([("shift", w) for w in C4_SHIFT_LAYERS] + [("dense", k) for k in C4_DENSE_KINDS] +
             [("fold", b) for b in (0, 1, 2)])
CHESS_PROBES = ([("shift", w) for w in CHESS_SHIFT_LAYERS] + [("dense", k) for k in CHESS_DENSE_KINDS] +
                [("fold", b) for b in (0, 1)])


def probe_nets(game, family, which):
    """-> [(tap or None, params, blocks, probed layer or None)]: the nets of one probe
    (a shift probe is nine nets, one per tap)"""
    c4 = game == "c4"
    if family == "shift":
        return [(t,) + (c4_shift_probe if c4 else chess_shift_probe)(which, t) for t in range(9)]
    if family == "dense":
        return [(None,) + (c4_dense_probe if c4 else chess_dense_probe)(which)]
    return [(None,) + (c4_fold_probe if c4 else chess_fold_probe)(which) + (None,)]


def probe_id(p):
    return "%s-%s" % p
