"""scripts/c4_match.py's score and Elo arithmetic (no device needed)."""
import importlib.util
import math
import os

from conftest import REPO


def _mod():
    spec = importlib.util.spec_from_file_location("c4_match", os.path.join(REPO, "scripts", "c4_match.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_elo_from_trinomial_counts():
    elo = _mod().elo_from_counts
    even = elo(30, 40, 30)
    assert even["score"] == 0.5 and even["elo"] == 0.0
    assert math.isclose(even["elo_lo"], -even["elo_hi"]) and even["elo_hi"] > 0
    # score 0.75 is 400 log10(3) Elo; draws narrow the interval at the same score
    wins = elo(75, 0, 25)
    drawn = elo(50, 50, 0)
    assert wins["score"] == drawn["score"] == 0.75
    assert math.isclose(wins["elo"], 400 * math.log10(3))
    assert math.isclose(wins["score_se"], math.sqrt(0.75 * 0.25 / 100))
    assert math.isclose(drawn["score_se"], math.sqrt(0.0625 / 100))
    assert drawn["elo_hi"] - drawn["elo_lo"] < wins["elo_hi"] - wins["elo_lo"]
    # a clean sweep has no finite Elo
    sweep = elo(10, 0, 0)
    assert sweep["score"] == 1.0 and sweep["elo"] is None and sweep["elo_hi"] is None
    assert elo(0, 0, 0) is None
