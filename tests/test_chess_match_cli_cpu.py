"""scripts/chess_match.py's arguments and report line on a faked match result (no device needed)."""
import importlib.util
import json
import math
import os
import sys

import pytest

from conftest import REPO


def _mod():
    spec = importlib.util.spec_from_file_location("chess_match", os.path.join(REPO, "scripts", "chess_match.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_scoring_is_c4_match_s():
    m = _mod()
    c4 = sys.modules["c4_match"]
    assert m.elo_from_counts is c4.elo_from_counts
    assert os.path.samefile(c4.__file__, os.path.join(REPO, "scripts", "c4_match.py"))


def test_arguments():
    ap = _mod().parser()
    d = ap.parse_args(["a.safetensors", "uniform"])
    assert (d.a, d.b, d.games, d.sims_a, d.sims_b, d.blocks, d.opening_plies, d.max_plies, d.seed, d.max_trees,
            d.bench) == ("a.safetensors", "uniform", 64, 400, 400, 20, 2, 512, 0, 1024, False)
    d = ap.parse_args(["init:3", "hash", "--games", "10", "--sims-a", "48", "--sims-b", "8", "--blocks", "1",
                       "--opening-plies", "3", "--max-plies", "40", "--seed", "7", "--max-trees", "8"])
    assert (d.a, d.b, d.games, d.sims_a, d.sims_b, d.blocks, d.opening_plies, d.max_plies, d.seed, d.max_trees) == \
        ("init:3", "hash", 10, 48, 8, 1, 3, 40, 7, 8)
    assert ap.parse_args(["--bench"]).bench
    with pytest.raises(SystemExit):
        _mod().main(["only-one-player"])


class FakeEngine:
    """ChessEngine.match's interface: every call is recorded and answers fixed counts per game"""

    def __init__(self):
        self.calls = []

    def match(self, a, b, n_games, game_id_base=0, opening_plies=2, max_plies=512, seed=0, start=None,
              keep_moves=True):
        self.calls.append(dict(n=n_games, base=game_id_base, opening_plies=opening_plies, max_plies=max_plies,
                               seed=seed, keep_moves=keep_moves))
        first = sum(1 for g in range(n_games) if (game_id_base + g) % 2 == 0)
        second = n_games - first
        # A wins every game it moves first in; the others are drawn, one of them by adjudication
        st = dict(a_wins=[float(first), 0.0], draws=[0.0, float(second)], b_wins=[0.0, 0.0],
                  sims=[100.0 * n_games, 50.0 * n_games], evals=[90.0 * n_games, 45.0 * n_games],
                  adjudicated=1.0, plies=30.0 * n_games, seconds=0.5)
        return [], st


def test_play_sums_calls_and_reports():
    m = _mod()
    eng = FakeEngine()
    out = m.play(eng, ("A",), ("B",), games=10, per_call=4, opening_plies=3, max_plies=40, seed=7)
    assert [(c["n"], c["base"]) for c in eng.calls] == [(4, 0), (4, 4), (2, 8)]
    assert all((c["opening_plies"], c["max_plies"], c["seed"], c["keep_moves"]) == (3, 40, 7, False)
               for c in eng.calls)
    assert out["games"] == 10 and out["a_wins"] == [5.0, 0.0] and out["draws"] == [0.0, 5.0]
    assert out["b_wins"] == [0.0, 0.0] and out["adjudicated"] == 3.0 and out["plies"] == 300.0
    assert out["sims"] == [1000.0, 500.0] and out["evals"] == [900.0, 450.0]
    assert out["seconds"] == 1.5 and out["sims_per_s"] == 1000.0
    assert out["score"] == 0.75 and math.isclose(out["elo"], 400 * math.log10(3))
    assert out["elo_lo"] < out["elo"] < out["elo_hi"]
    json.dumps(out)   # the report is one JSON line


def test_report_of_a_sweep_has_no_finite_elo():
    m = _mod()
    tot = dict(a_wins=[2.0, 2.0], draws=[0.0, 0.0], b_wins=[0.0, 0.0], sims=[1.0, 1.0], evals=[1.0, 1.0],
               adjudicated=0.0, plies=8.0)
    out = m.report(tot, 4, 0.0)
    assert out["score"] == 1.0 and out["elo"] is None and out["sims_per_s"] is None
