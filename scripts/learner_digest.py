"""SHA-256 digests of what the three device learners compute from fixed seeds (a
record for comparing two builds of the library to the bit, not a test).

  TicTacToe  blocks 2: two train_batch steps of 17, then train(n=70, batch=32, epochs=2)
  chess      blocks 1: two train_batch steps of 5, then train(n=9, batch=4, epochs=2)
  Connect4   blocks 1, hidden 64: train(n=70, batch=32, epochs=2)

After every call the digest covers the raw bytes of the returned loss, grads() and
params().  Prints one JSON object; run it once per build (SPAI_LIB selects the
library) and compare the outputs: apart from "commit" they must be identical.

usage: [SPAI_LIB=path/libspai.so] python scripts/learner_digest.py [--commit HASH] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle"), os.path.join(REPO, "self-play-ai_amd")):
    sys.path.insert(0, p)


def digest(loss, L):
    h = hashlib.sha256()
    for a in (loss, L.grads(), L.params()):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


def run(L, steps, epoch_set):
    """digests after each train_batch of `steps` and after train(*epoch_set, batch, epochs)"""
    out = {}
    for k, (x, pi, z) in enumerate(steps):
        out[f"train_batch_{k}"] = digest(L.train_batch(x, pi, z), L)
    (x, pi, z), batch, epochs = epoch_set
    out["train"] = digest(L.train(x, pi, z, epochs=epochs, batch=batch, seed=9), L)
    L.close()
    return out


def tictactoe():
    import spai_ttt as st
    import ttt_learner_ref as LR
    eng = st.TTTEngine(num_searches=1, max_trees=1)
    out = run(st.TTTLearner(eng, 2, st.init_params(2, 5)), LR.make_batches(17, 2, 17)[2],
              (LR.make_batches(70, 1, 70)[2][0], 32, 2))
    eng.close()
    return out


def chess():
    import chess_learner_ref as LR
    import spai_chess as sc
    eng = sc.ChessEngine(num_searches=1, max_trees=1, max_moves=64)
    out = run(sc.ChessLearner(eng, 1, sc.init_params(1, 5)), LR.make_batches(5, 2, 5)[2],
              (LR.make_batches(9, 1, 9)[2][0], 4, 2))
    eng.close()
    return out


def connect4():
    import spai
    n, rng = 70, np.random.default_rng(70)
    cells = rng.integers(0, 3, (n, 42))   # any one-hot planes do: the step does not check reachability
    x = (cells[:, None, :] == np.arange(3)[None, :, None]).astype(np.float32).reshape(n, 126)
    pi = rng.random((n, 7)).astype(np.float32) ** 2
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    z = rng.choice(np.array([-1, 0, 1], np.float32), n)
    eng = spai.Engine(num_searches=1, max_trees=1)
    out = run(spai.Learner(eng, 1, spai.init_params(1, 64, seed=5)), [], ((x, pi, z), 32, 2))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    rec = dict(commit=commit, tictactoe=tictactoe(), chess=chess(), connect4=connect4())
    text = json.dumps(rec, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
