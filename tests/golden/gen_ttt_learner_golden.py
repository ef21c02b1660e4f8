"""Golden of the TicTacToe train step: PyTorch CPU fp32 (autograd + torch.optim.Adam)
on the net built from the flat parameters, 1x64, B = 32, 3 steps.  Writes
learner_ttt_1x64.npz (inputs, losses, step-1 gradients, parameters after step 1)
and learner_ttt_1x64_step3.npz (parameters after step 3).  The initial
parameters come from the seed (spai_ttt.init_params), not from the file.

    python tests/golden/gen_ttt_learner_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "self-play-ai_amd")):
    sys.path.insert(0, p)

BLOCKS, HIDDEN, SEED, B, K = 1, 64, 21, 32, 3


def main():
    import torch
    import spai_ttt
    import ttt_learner_ref as LR
    torch.manual_seed(0)
    torch.set_num_threads(1)
    p0 = spai_ttt.init_params(BLOCKS, SEED)
    _, _, batches = LR.make_batches(B, K, SEED)
    s, pi, z = (np.array([b[i] for b in batches]) for i in range(3))
    steps = LR.torch_train(p0, batches, BLOCKS)
    np.savez(os.path.join(HERE, "learner_ttt_1x64.npz"), meta=np.array([BLOCKS, HIDDEN, SEED, B, K]), states=s,
             policies=pi, values=z, loss=np.array([st[0] for st in steps]), grads1=steps[0][1], params1=steps[0][2])
    np.savez(os.path.join(HERE, "learner_ttt_1x64_step3.npz"), params3=steps[K - 1][2])
    print("loss", [st[0] for st in steps])


if __name__ == "__main__":
    main()
