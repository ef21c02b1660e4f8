#!/usr/bin/env python3
"""Generate tests/golden/trained_like_nets.npz: the Connect4, TicTacToe and chess
nets in PyTorch CPU fp32 (the torch_forward functions of gen_golden.py and
gen_chess_golden.py) on trained-like parameters -- non-zero conv biases, BN
beta and running mean, running variance != 1, some negative gammas
(tests/bf16_ref.py trained_like) -- where every other fixture has the init's
identity statistics.

Runs in the build container only (needs torch CPU, the oracle library and
libspai.so for the host-only chess parameter init).  The fixture stores the
inputs, logits and values; the tests regenerate the parameters from the seeds
in NETS through trained_like.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "self-play-ai_amd")]

import bf16_ref as R  # noqa: E402

# net -> (blocks, init seed, trained_like seed, positions, position seed)
NETS = {"c4": (2, 21, 31, 32, 41), "ttt": (2, 22, 32, 32, 42), "chess": (1, 23, 33, 4, 43)}
C4_DIMS, TTT_DIMS = (3, 6, 7, 7), (3, 3, 3, 9)


def net_params(net):
    """the trained-like parameter vector of a fixture net (used by the tests too)"""
    blocks, seed, tl_seed = NETS[net][:3]
    if net == "chess":
        import spai_chess
        return R.trained_like(spai_chess.init_params(blocks, seed), R.chess_layout(blocks), tl_seed)
    import oracle
    game, dims = (oracle.GAME_CONNECT4, C4_DIMS) if net == "c4" else (oracle.GAME_TICTACTOE, TTT_DIMS)
    return R.trained_like(oracle.init_params(game, blocks, 64, seed), R.c4_layout(blocks, 64, dims), tl_seed)


def positions(net):
    import gen_golden as G
    n, seed = NETS[net][3:]
    rng = random.Random(seed)
    if net == "chess":
        import gen_chess_golden as GC
        return GC.positions(n, seed)
    cls = G.C4 if net == "c4" else G.TTT
    out = []
    while len(out) < n:
        s = cls()
        for _ in range(rng.randrange(0, 30 if net == "c4" else 7)):
            if s.status != G.ONGOING:
                break
            s = s.next_state(rng.choice(s.valid()))
        if s.status == G.ONGOING:
            out.append(s.encoding())
    return np.stack(out).astype(np.float32)


def main():
    import torch
    import gen_chess_golden as GC
    import gen_golden as G
    torch.set_num_threads(8)
    out = {}
    for net in ("c4", "ttt"):
        blocks = NETS[net][0]
        x = positions(net)
        lg, v, _ = G.torch_forward(net_params(net), C4_DIMS if net == "c4" else TTT_DIMS, blocks, 64, x)
        out.update({net + "_x": x, net + "_logits": lg, net + "_value": v})
    x = positions("chess")
    lg, v = GC.torch_forward(net_params("chess"), NETS["chess"][0], x)
    out.update(chess_x=x, chess_logits=lg, chess_value=v)
    np.savez_compressed(os.path.join(HERE, "trained_like_nets.npz"), **out)
    print("wrote trained_like_nets.npz", {k: a.shape for k, a in out.items()})


if __name__ == "__main__":
    main()
