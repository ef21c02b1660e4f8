"""tests/chess_f32_ref.py, the float32 restatement that the fp32 chess net
(ChessNet(dtype="f32")) is held against bit for bit, anchored on the CPU: it runs
no device code, so it has to be shown to be the chess net, and to react to the
errors a forward kernel can make.

The unit of every bound is the spread: the largest difference, over the logits and
the value's pre-activation, between the restatement's order and a second float32
order (input channels descending), computed here on the same inputs.  Two correct
fp32 forwards differ by about one spread; the bound is 4 x spread.

Measured (6 positions of tests/golden/chess_net_b1.npz, 1 block, init seed 7):
  init parameters      spread 1.0e-6 at max |logit| 1.26;
                       against chessref.net_forward (float64) 0.80 x spread,
                       against the libtorch logits of the fixture 0.88 x spread,
                       value against libtorch 8.4e-8
  trained-like (BN and conv biases overwritten, seed 61)
                       spread 5.7e-6 at max |logit| 3.66; against float64 0.70 x spread
  faults               the smallest effect is planes 17 / 18 rounded to bf16: 62 x and
                       238 x spread (trained-like), 103 x and 567 x (init); every other
                       fault moves a logit by more than 1e5 x spread
"""
import ctypes as C
import os

import numpy as np
import pytest

import chess_f32_ref as F
import chessref as ch
from bf16_ref import bf16_round
from conftest import GOLDEN

BLOCKS, SEED, TRAINED_SEED = 1, 7, 61
BOUND = 4.0   # x spread


def init_params(blocks, seed):
    """spai_chess_net_init_params is host-only: no device needed"""
    import spai
    L = spai.lib()
    n = C.c_size_t()
    L.spai_chess_net_num_params.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    L.spai_chess_net_init_params.argtypes = [C.c_int, C.c_uint64, C.c_void_p]
    assert L.spai_chess_net_num_params(blocks, C.byref(n)) == 0
    p = np.zeros(n.value, np.float32)
    assert L.spai_chess_net_init_params(blocks, seed, p.ctypes.data_as(C.c_void_p)) == 0
    return p


def diff(a, b):
    """largest |difference| over logits and value pre-activation of two forwards"""
    return max(float(np.abs(a[0].astype(np.float64) - b[0]).max()), float(np.abs(a[1].astype(np.float64) - b[1]).max()))


@pytest.fixture(scope="module")
def G():
    g = np.load(os.path.join(GOLDEN, "chess_net_b1.npz"))
    assert int(g["blocks"]) == BLOCKS and int(g["seed"]) == SEED
    x = g["x"]
    out = dict(x=x, golden=(g["logits"], g["value"]))
    init = init_params(BLOCKS, SEED)
    for name, p in (("init", init), ("trained", F.trained_like(init, BLOCKS, TRAINED_SEED))):
        asc = F.forward(p, BLOCKS, x)
        desc = F.forward(p, BLOCKS, x, order="desc")
        out[name] = dict(params=p, asc=asc, spread=diff(asc, desc))
        print(f"{name}: spread {out[name]['spread']:.3g} at max |logit| {np.abs(asc[0]).max():.3g}")
    return out


def f64_pre(params, x):
    """chessref.net_forward's logits and value; the value as its pre-activation"""
    lg, v = ch.net_forward(params, BLOCKS, x)
    return lg, np.arctanh(v)


def test_anchored_to_float64_and_libtorch(G):
    d = G["init"]
    assert 0 < d["spread"] < 1e-5
    r64 = diff(d["asc"], f64_pre(d["params"], G["x"])) / d["spread"]
    lg, v = G["golden"]
    rlt = float(np.abs(d["asc"][0].astype(np.float64) - lg).max()) / d["spread"]
    rv = float(np.abs(F.value_of(d["asc"][1]).astype(np.float64) - v).max()) / d["spread"]
    print(f"init: float64 {r64:.2f} x spread, libtorch logits {rlt:.2f} x, libtorch value {rv:.2f} x")
    assert r64 <= BOUND and rlt <= BOUND and rv <= BOUND, (r64, rlt, rv)


def test_trained_like_parameters(G):
    """init_params' BatchNorm is the identity and its conv biases are zero: only these
    parameters can show a wrong BN order, a swapped mean and variance or a lost bias"""
    d = G["trained"]
    p, q = d["params"], G["init"]["params"]
    for (kind, a), (_, b) in zip(ch.unpack_params(p, BLOCKS), ch.unpack_params(q, BLOCKS)):
        if kind == "bn":
            g, be, mu, var = a
            assert (var > 0).all() and all(not np.array_equal(u, w) for u, w in zip(a, b))
            assert np.abs(mu).min() > 0 and np.abs(be).min() > 0 and (g < 0).any()
    r64 = diff(d["asc"], f64_pre(p, G["x"])) / d["spread"]
    print(f"trained-like: float64 {r64:.2f} x spread")
    assert r64 <= BOUND, r64


FAULTS = [("drop_tap", 2), ("zero_bias", 2), ("swap_cells", 2), ("swap_planes", None), ("bn_mean_beta", 0),
          ("bn_mean_beta", 2), ("no_residual", 0), ("bf16_plane", 17), ("bf16_plane", 18)]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f"{f[0]}-{f[1]}")
def test_the_yardstick_reacts(G, fault):
    d = G["trained"]
    x = G["x"]
    kind, arg = fault
    if kind == "swap_planes":
        x2 = x.copy()
        x2[:, [0, 6]] = x[:, [6, 0]]           # my pawns <-> their pawns
        got = F.forward(d["params"], BLOCKS, x2)
    elif kind == "bf16_plane":
        x2 = x.copy()
        x2[:, arg] = bf16_round(x[:, arg]).astype(np.float32)
        assert not np.array_equal(x2[:, arg], x[:, arg])   # the fixture's fractions are no bf16 numbers
        got = F.forward(d["params"], BLOCKS, x2)
    else:
        got = F.forward(d["params"], BLOCKS, x, fault=fault)
    r = diff(got, d["asc"]) / d["spread"]
    print(f"{kind} {arg}: {r:.3g} x spread")
    assert r > BOUND, r


def test_abi():
    import spai
    L = spai.lib()
    for s in ("spai_chess_net_create_dtype", "spai_chess_net_dtype"):
        assert s in spai.SYMBOLS and hasattr(L, s), s
    # host-side argument checks, no device needed
    L.spai_chess_net_dtype.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    d = C.c_int()
    assert L.spai_chess_net_dtype(None, C.byref(d)) == -1
    import spai_chess as sc
    sc.lib()
    assert sc.ChessNet.DTYPES == {"bf16": 0, "f32": 1}
    with pytest.raises(ValueError):
        sc.ChessNet(None, 1, np.zeros(1, np.float32), dtype="fp16")
