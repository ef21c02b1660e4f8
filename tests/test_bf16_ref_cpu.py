"""CPU checks of tests/bf16_ref.py, the reference the GPU net tests compare the
fused bf16 forwards with (test_net_exact_gpu.py, test_net_trained_params_gpu.py):

* its bf16 rounding is torch's;
* without quantisation it is the PyTorch net of gen_golden.py / gen_chess_golden.py
  on trained-like parameters (non-identity BatchNorm statistics, non-zero conv
  biases), and so are the CPU oracles: the oracles' BN path away from mean 0 / var 1;
* every exact-arithmetic probe passes its own exactness asserts on the inputs the
  GPU tests use (nothing rounds, any fp32 summation order gives the same bits);
* every probe reacts to the mutation it is there to catch: each tap at each cell,
  each channel's bias, a cell swap;
* the bound of the trained-parameter tests (4 x the spread of fp32 summation
  orders) is at most a third of what a dropped corner tap or a zeroed bias moves,
  and below the old 3e-2 bar.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import bf16_ref as R

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


# ---------------------------------------------------------------- bf16 rounding
def _bits32(u):
    return np.array(u, np.uint32).view(np.float32)


def test_bf16_round_matches_torch():
    import torch
    rng = np.random.default_rng(0)
    hi = rng.integers(0, 1 << 16, 4096).astype(np.uint32) << 16
    parts = [
        (rng.standard_normal(20000) * np.exp(rng.uniform(-30, 30, 20000))).astype(np.float32),
        rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),   # any bit pattern
        _bits32(hi | 0x8000), _bits32(hi | 0x7FFF), _bits32(hi | 0x8001),                      # ties, just below / above
        _bits32(rng.integers(0, 1 << 23, 4096).astype(np.uint32) | (rng.integers(0, 2, 4096).astype(np.uint32) << 31)),
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 3.4028235e38, -3.4028235e38, 3.3895314e38,
                  1e-45, -1e-45, 1.0, 1.00390625, 1.01171875], np.float32),
        _bits32([0x7F800001, 0xFF800001, 0x7FC00000, 0x7FBFFFFF, 0x7F7F8000, 0x7F7F7FFF]),
    ]
    a = np.concatenate(parts)
    mine = R.bf16_bits(a)
    ref = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(a)
    assert nan.sum() > 100 and (~nan).sum() > 40000
    np.testing.assert_array_equal(mine[~nan], ref[~nan])
    # NaN: torch returns the canonical quiet NaN, f2bf keeps the sign and the top payload
    # bits and sets the quiet bit when the payload sat in the low half: both are NaNs
    for b in (mine[nan], ref[nan]):
        assert np.all((b & 0x7F80) == 0x7F80) and np.all(b & 0x7F)
    # the value form used by the forwards
    v = R.bf16_round(a[~nan])
    np.testing.assert_array_equal(v.astype(np.float32), torch.from_numpy(a[~nan]).to(torch.bfloat16).float().numpy())


# ---------------------------------------------------------------- plain reference vs PyTorch and the oracles
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "trained_like_nets.npz"))


def _close(a, ref, tol, what):
    err = float(np.abs(np.asarray(a, np.float64) - ref).max())
    bar = tol * max(1.0, float(np.abs(ref).max()))
    print("%s: max |d| %.3g (bar %.3g)" % (what, err, bar))
    assert err <= bar, (what, err, bar)


# fp32 nets against float64: an fp32 sum of K terms of size ~a is off by ~sqrt(K) * 6e-8 * a,
# five to seven layers deep, on logits of a few units: a few 1e-6; 2e-5 relative to the
# largest logit is the bar (the oracle and PyTorch are both fp32)
F32_VS_F64 = 2e-5


@pytest.mark.parametrize("net", ["c4", "ttt"])
def test_plain_reference_vs_torch_and_oracle(oracle, fixture, net):
    import gen_golden as G
    import gen_trained_like_golden as GT
    blocks = GT.NETS[net][0]
    dims = GT.C4_DIMS if net == "c4" else GT.TTT_DIMS
    game = oracle.GAME_CONNECT4 if net == "c4" else oracle.GAME_TICTACTOE
    p, x = GT.net_params(net), fixture[net + "_x"]
    d = R.unflatten(p, R.c4_layout(blocks, 64, dims))
    for name, v in d.items():   # trained-like: no identity statistics left
        kind = name.split(".")[1]
        if kind in ("be", "mu") or (kind == "b" and "lin" not in name):
            assert np.all(np.abs(v) >= 0.1)
        if kind == "var":
            assert np.abs(v - 1.0).mean() > 0.1 and v.min() >= 0.5 and v.max() <= 2.0
        if kind == "g":
            assert ((v < 0).any() or v.size <= 5) and np.all(np.abs(v) >= 0.5)
    lg, v = R.c4_forward(p, blocks, x, quant=False, dims=dims)
    _close(fixture[net + "_logits"], lg, F32_VS_F64, net + " fixture logits")
    _close(fixture[net + "_value"], v, F32_VS_F64, net + " fixture value")
    tl, tv, _ = G.torch_forward(p, dims, blocks, 64, x)
    _close(tl, lg, F32_VS_F64, net + " torch logits")
    _close(tv, v, F32_VS_F64, net + " torch value")
    ol, ov = oracle.Net(game, blocks, 64, p).forward(x.reshape(len(x), -1))
    _close(ol, lg, F32_VS_F64, net + " oracle logits")
    _close(ov, v, F32_VS_F64, net + " oracle value")


def test_plain_chess_reference_vs_torch_and_oracle(fixture):
    import chessref
    import gen_chess_golden as GC
    import gen_trained_like_golden as GT
    blocks = GT.NETS["chess"][0]
    p, x = GT.net_params("chess"), fixture["chess_x"]
    d = R.unflatten(p, R.chess_layout(blocks))
    for name in ("p1.b", "p2.b", "v.b", "stem.b", "res1.mu"):
        assert np.all(np.abs(d[name]) >= 0.1)
    lg, v = R.chess_forward(p, blocks, x, quant=False)
    _close(fixture["chess_logits"], lg, F32_VS_F64, "chess fixture logits")
    _close(fixture["chess_value"], v, F32_VS_F64, "chess fixture value")
    tl, tv = GC.torch_forward(p, blocks, x)
    _close(tl, lg, F32_VS_F64, "chess torch logits")
    _close(tv, v, F32_VS_F64, "chess torch value")
    ol, ov = chessref.net_forward(p, blocks, x)   # float64 itself
    _close(ol, lg, 1e-12, "chessref logits")
    _close(ov, v, 1e-12, "chessref value")


def test_c4_encode_matches_oracle(oracle):
    """the helper's bitboard -> planes encoding is the oracle's (predict runs on
    bitboards, the reference on planes)"""
    for bx, bo, n, _ in R.c4_random_states(40, 36, seed=3):
        st = oracle.C4State()
        oracle.lib().or_c4_init(oracle.C.byref(st))
        for col in range(7):
            for row in range(6):
                b = 1 << (col * 7 + row)
                st.board[row][col] = oracle.X if bx & b else oracle.O if bo & b else 0
        st.num_actions_played = n
        st.current_player = oracle.X if n % 2 == 0 else oracle.O
        enc = np.asarray(oracle.C4(st).encoding(), np.float32).reshape(3, 6, 7)
        assert np.array_equal(enc, R.c4_encode([(bx, bo, n, 0)])[0])


# ---------------------------------------------------------------- exact probes
@pytest.fixture(scope="module")
def c4_in():
    return R.c4_probe_inputs()


@pytest.fixture(scope="module")
def chess_in():
    return R.chess_probe_inputs()


def test_probe_inputs(c4_in, chess_in):
    x, states = c4_in
    assert len(states) == R.C4_PREDICT_UNIQUE and x.shape == (24 + len(states), 3, 6, 7)
    assert set(np.unique(x)) == {0.0, 1.0} and x.any((0, 1)).all() and chess_in.any((0, 1)).all()
    enc = x[24:]
    assert np.array_equal(enc.sum(1), np.ones((len(states), 6, 7)))   # mine / theirs / empty
    legal = R.c4_legal(states)
    assert (~legal).any() and legal.any(1).all()                      # full columns occur, no full board
    assert np.array_equal(legal, enc[:, 2, 5, :] == 1)                 # a column is open iff its top cell is empty


@pytest.mark.parametrize("probe", R.C4_PROBES, ids=R.probe_id)
def test_c4_probe_is_exact(c4_in, probe):
    x, _ = c4_in
    for tap, params, blocks, layer in R.probe_nets("c4", *probe):
        info, cache = {}, {}
        lg, v = R.c4_forward(params, blocks, x, exact=True, info=info, cache=cache)
        if tap in (None, 0, 4, 8):   # any fp32 order: permuted, chunked fp32 accumulation gives the same bits
            l2, v2 = R.c4_forward(params, blocks, x, acc=np.float32, korder=5, chunk=8, cache=cache)
            assert np.array_equal(lg, l2) and np.array_equal(v, v2)
        assert len(np.unique(lg)) > lg.size // 8 and np.abs(lg).max() < 64    # softmax stays sensitive
        assert np.abs(info["pre_tanh"]).max() < 6 and np.ptp(info["pre_tanh"]) > 0.25
        print(probe, tap, "max |act| %g, max sum of |terms| %g units" % (info["max_act"], info["max_units"]))


@pytest.mark.parametrize("probe", R.CHESS_PROBES, ids=R.probe_id)
def test_chess_probe_is_exact(chess_in, probe):
    for tap, params, blocks, layer in R.probe_nets("chess", *probe):
        info, cache = {}, {}
        lg, v = R.chess_forward(params, blocks, chess_in, exact=True, info=info, cache=cache)
        if tap in (None, 4):   # any fp32 order gives the same bits
            l2, v2 = R.chess_forward(params, blocks, chess_in, acc=np.float32, korder=5, chunk=16, cache=cache)
            assert np.array_equal(lg, l2) and np.array_equal(v, v2)
        assert np.abs(info["pre_tanh"]).max() < 6 and np.ptp(info["pre_tanh"]) > 0.01
        print(probe, tap, "max |act| %g, max sum of |terms| %g units" % (info["max_act"], info["max_units"]))


# ---------------------------------------------------------------- mutation checks
def _reacts(forward, params, blocks, x, base, cache, m):
    info = {}
    lg, _ = forward(params, blocks, x, mutate=m, cache=cache, info=info)
    return not (np.array_equal(lg, base[0]) and np.array_equal(info["pre_tanh"], base[1]))


def _mutation_check(game, probe, x):
    forward = R.c4_forward if game == "c4" else R.chess_forward
    H, W = (6, 7) if game == "c4" else (8, 8)
    cells = H * W
    family = probe[0]
    n_mut = 0
    for tap, params, blocks, layer in R.probe_nets(game, *probe):
        cache, info = {}, {}
        lg, _ = forward(params, blocks, x, cache=cache, info=info)
        base = (lg, info["pre_tanh"])

        def reacts(m):
            return _reacts(forward, params, blocks, x, base, cache, m)
        if family in ("shift", "dense") and layer is not None:
            k1 = layer in ("p1", "p2", "v")   # 1x1 convs: the one tap
            taps = [0] if k1 else [tap] if family == "shift" else range(9)
            for t in taps:
                for cell in range(cells):
                    if k1 or R.tap_on_board(cell, t, H, W):
                        assert reacts(("drop_tap", layer, cell, t)), (probe, "tap", t, "cell", cell)
                        n_mut += 1
        swap_layer = layer if layer is not None else "head" if game == "c4" else "p1"
        # (two interior cells; a border cell with an interior one)
        assert reacts(("swap_cells", swap_layer, W + 1, W + 2)) and reacts(("swap_cells", swap_layer, 1, cells - 2 - W))
        if family == "fold":
            layers = ["stem"] + ["res%d" % i for i in range(2 * blocks)] + (["head"] if game == "c4" else ["p1", "p2", "v"])
            dead = live_bias_only = 0
            for L in layers:
                if L == "head":
                    w = np.concatenate([cache[("fold", "pol")][0], cache[("fold", "val")][0]])
                    b = np.concatenate([cache[("fold", "pol")][1], cache[("fold", "val")][1]])
                elif L in ("p1", "p2", "v"):
                    d = R.unflatten(params, R.chess_layout(blocks))
                    w, b = d[L + ".w"], d[L + ".b"]
                else:
                    w, b = cache[("fold", L)]
                assert np.all(b != 0), (probe, L)
                for c in range(len(b)):
                    bias_only = not w[c].any()
                    if bias_only and b[c] < 0 and L != "p2":   # relu(b) = relu(0): zeroing cannot show; a
                        dead += 1                               # wrong positive bias there would
                        continue
                    live_bias_only += bias_only
                    assert reacts(("zero_bias", L, c)), (probe, L, "channel", c)
                    n_mut += 1
            assert dead > 0 and live_bias_only > 0   # channels whose bias alone decides the ReLU, both ways
    print(probe, n_mut, "mutations, all seen")


@pytest.mark.parametrize("probe", R.C4_PROBES, ids=R.probe_id)
def test_c4_probe_reacts_to_mutations(c4_in, probe):
    x, _ = c4_in
    _mutation_check("c4", probe, x if probe[0] == "fold" else np.concatenate([x[:6], x[24:30]]))


@pytest.mark.parametrize("probe", R.CHESS_PROBES, ids=R.probe_id)
def test_chess_probe_reacts_to_mutations(chess_in, probe):
    _mutation_check("chess", probe, chess_in[:3] if probe[0] == "fold" else chess_in[:2])


def test_mutation_must_name_a_layer():
    params, blocks, _ = R.c4_dense_probe("stem")
    with pytest.raises(AssertionError):
        R.c4_forward(params, blocks, R.c4_probe_inputs()[0][:2], mutate=("zero_bias", "res7", 0))


# ---------------------------------------------------------------- the trained-parameter bound
def trained_c4_params(oracle, blocks):
    return R.trained_like(oracle.init_params(oracle.GAME_CONNECT4, blocks, 64, 50 + blocks), R.c4_layout(blocks),
                          60 + blocks)


def trained_chess_params(blocks):
    import spai_chess
    return R.trained_like(spai_chess.init_params(blocks, 50 + blocks), R.chess_layout(blocks), 60 + blocks)


@pytest.mark.parametrize("blocks", [0, 1, 2])
def test_c4_trained_bound_conditions(oracle, fixture, blocks):
    p, x = trained_c4_params(oracle, blocks), fixture["c4_x"]
    ref = R.spread_bound(R.c4_forward, p, blocks, x)
    eff = R.check_bound_conditions(R.c4_forward, p, blocks, x, ref)
    print("c4 %d blocks: spread %.3g, bound %.3g, effects %s, old bar %.3g" % (
        blocks, ref["spread_l"], ref["bound_l"], np.round(eff, 4), 3e-2 * max(1.0, np.abs(ref["logits"]).max())))


@pytest.mark.parametrize("blocks", [0, 1])
def test_chess_trained_bound_conditions(fixture, blocks):
    p, x = trained_chess_params(blocks), fixture["chess_x"]
    ref = R.spread_bound(R.chess_forward, p, blocks, x, chunk=4)
    eff = R.check_bound_conditions(R.chess_forward, p, blocks, x, ref)
    print("chess %d blocks: spread %.3g, bound %.3g, effects %s, old bar %.3g" % (
        blocks, ref["spread_l"], ref["bound_l"], np.round(eff, 4), 3e-2 * max(1.0, np.abs(ref["logits"]).max())))
