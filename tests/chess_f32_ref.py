"""The fp32 chess net (csrc/chess_net_f32.hip, ChessNet(dtype="f32")) restated in
numpy float32, in the kernel's own summation order, so that every logit and the
value's pre-activation can be compared bit for bit.

The order (include/spai.h, spai_chess_net_create_dtype):
  3x3 convs   each output starts at the conv bias; then the products are added
              input channel ascending, kernel row, kernel column, with separate
              multiply and add; an off-board tap is skipped
  BatchNorm   ((x - mean) * inv) * gamma + beta, inv = 1 / sqrt(var + 1e-5) in float32
  residual    relu(h + bn(conv(...))), the block input as the left operand
  heads       conv1x1 and linear outputs: the bias first, then the input index ascending

It is vectorised over the outputs and loops over (ci, ky, kx): every statement is
  acc = acc + w[:, ci, ky, kx] * x_shifted
on float32 arrays, so every product and every sum rounds to float32 exactly as on
the device.  It runs none of the device's code and none of chessref.net_forward's
(float64, one matmul).

order="desc" sums the input channels (and the head inputs) descending instead: a
second fp32 order, used only to measure the spread between two fp32 summation
orders, the unit of the CPU test's bounds.

fault: one deliberate error, for the tests that show the yardstick reacts
  ("drop_tap", layer)      tap (ky, kx) = (0, 0) of that trunk conv left out
  ("zero_bias", layer)     that trunk conv's bias lost
  ("swap_cells", layer)    cells 9 and 10 of that trunk conv's output exchanged
  ("bn_mean_beta", layer)  that conv's BN mean and beta exchanged
  ("no_residual", block)   that block's residual left out
with layer 0 the stem and layer 1 + i trunk conv i.
"""
import numpy as np

import chessref as ch

F32 = np.float32
EPS = F32(1e-5)


def relu(v):
    return np.where(v < 0, F32(0), v)   # the kernel's `v < 0 ? 0 : v`


def _chan_order(n, order):
    return range(n) if order == "asc" else range(n - 1, -1, -1)


def conv3x3(x, w, b, order="asc", drop_tap=None):
    """x [n][ci][8][8], w [co][ci][3][3], b [co] -> [n][co][8][8], float32 throughout"""
    n, ci = x.shape[:2]
    co = w.shape[0]
    acc = np.empty((n, co, 8, 8), F32)
    acc[...] = b[None, :, None, None]
    for i in _chan_order(ci, order):
        for ky in range(3):
            for kx in range(3):
                if drop_tap == (ky, kx):
                    continue
                dy, dx = ky - 1, kx - 1
                y0, y1, x0, x1 = max(0, -dy), min(8, 8 - dy), max(0, -dx), min(8, 8 - dx)
                prod = w[None, :, i, ky, kx, None, None] * x[:, i, None, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                assert prod.dtype == F32
                a = acc[:, :, y0:y1, x0:x1]
                np.add(a, prod, out=a)
    return acc


def dense(x, w, b, order="asc"):
    """x [n][k][...], w [o][k], b [o] -> [n][o][...]: the bias first, then k in order"""
    n, k = x.shape[:2]
    tail = x.shape[2:]
    ex = (None,) * len(tail)
    acc = np.empty((n, w.shape[0]) + tail, F32)
    acc[...] = b[(None, slice(None)) + ex]
    for i in _chan_order(k, order):
        prod = w[(None, slice(None), i) + ex] * x[:, i, None]
        assert prod.dtype == F32
        np.add(acc, prod, out=acc)
    return acc


def bn(x, g, b, m, v):
    inv = F32(1.0) / np.sqrt(v + EPS)
    assert inv.dtype == F32
    e = (slice(None), None, None)
    return ((x - m[e]) * inv[e]) * g[e] + b[e]


def forward(params, blocks, x, order="asc", fault=None):
    """-> logits [n][4672] float32, the value's pre-activation [n] float32 (value = tanh of it)"""
    P = ch.unpack_params(np.asarray(params, F32), blocks)
    x = np.ascontiguousarray(x, F32).reshape(-1, 19, 8, 8)
    it = iter(P)
    fk, fa = fault if fault else (None, None)

    def nxt():
        return next(it)[1]

    def conv_bn(h, layer):
        w, b, (g, be, mu, var) = nxt(), nxt(), nxt()
        if fk == "zero_bias" and fa == layer:
            b = np.zeros_like(b)
        if fk == "bn_mean_beta" and fa == layer:
            be, mu = mu, be
        y = bn(conv3x3(h, w, b, order, (0, 0) if fk == "drop_tap" and fa == layer else None), g, be, mu, var)
        if fk == "swap_cells" and fa == layer:
            y = y.reshape(y.shape[0], -1, 64).copy()
            y[:, :, [9, 10]] = y[:, :, [10, 9]]
            y = y.reshape(-1, y.shape[1], 8, 8)
        return y

    h = relu(conv_bn(x, 0))
    for blk in range(blocks):
        y = relu(conv_bn(h, 1 + 2 * blk))
        y = conv_bn(y, 2 + 2 * blk)
        h = relu(y if fk == "no_residual" and fa == blk else h + y)
    hf = h.reshape(h.shape[0], 256, 64)
    w, b = nxt(), nxt()
    p = relu(dense(hf, w.reshape(256, 256), b, order))
    w, b = nxt(), nxt()
    logits = dense(p, w.reshape(73, 256), b, order).reshape(-1, 73 * 64)
    w, b = nxt(), nxt()
    v = relu(dense(hf, w.reshape(1, 256), b, order))[:, 0, :]       # [n][64]
    w1, b1, w2, b2 = nxt(), nxt(), nxt(), nxt()
    v = relu(dense(v, w1, b1, order))                                # [n][256]
    vpre = dense(v, w2, b2, order)[:, 0]
    assert logits.dtype == F32 and vpre.dtype == F32
    return logits, vpre


def value_of(vpre):
    """tanh in float64, rounded to float32: what the device's tanhf is held against"""
    return np.tanh(np.asarray(vpre, np.float64)).astype(F32)


def trained_like(params, blocks, seed):
    """non-identity BatchNorm (and conv biases): bf16_ref.trained_like on the chess layout"""
    import bf16_ref as R
    return R.trained_like(np.asarray(params, F32), R.chess_layout(blocks), seed)
