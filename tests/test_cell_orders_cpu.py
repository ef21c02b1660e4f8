"""The fused Connect4 forward's row layouts and skipped taps (net_c4.hip: kCellOrder,
kRowTab, kRowLin, tap_skip), parsed out of the source and checked by brute force
over the 6x7 board, with none of the generator's own code:

  * every group size's rows hold each (position, cell) exactly once, the rest pads;
  * a skipped (group size, tile, tap) has no on-board neighbour in any of its 16
    rows, and the centre tap is never skipped;
  * the (tile, tap) pair counts per wave in the comment block are the recomputed ones
    (the kernel's task plans, restated here);
  * the row tables' B-fragment reads are free of LDS bank conflicts under the
    row & 7 XOR swizzle, counted over the lane groups that serve a ds_read_b128;
  * scripts/gen_cell_orders.py reproduces the committed row tables (S = 2, 3; the
    S >= 4 annealing takes minutes and is not rerun here).
"""
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "self-play-ai_amd", "csrc", "net_c4.hip")
ROWS, COLS, CELLS = 6, 7, 42
PAD = 255
SIZES = range(1, 9)
ROW_TABLE_SIZES = (2, 3)


def _ints(body):
    return [int(v) for v in re.findall(r"-?\d+", body)]


def _parse():
    text = open(SRC).read()

    def table(name):
        m = re.search(r"constexpr u?int8_t %s\[(\d+)\]\[(\d+)\] = \{(.*?)\n\};" % name, text, re.S)
        assert m, name
        body = re.sub(r"//[^\n]*", "", m.group(3))
        rows = [_ints(r) for r in re.findall(r"\{([^{}]*)\}", body)]
        assert len(rows) == int(m.group(1)) and all(len(r) == int(m.group(2)) for r in rows), name
        return rows

    lin = re.search(r"constexpr int8_t kRowLin\[2\]\[2\] = \{(.*?)\};", text)
    lin = _ints(lin.group(1))
    masks = {}
    for S in SIZES:
        m = re.search(r"constexpr uint16_t m%d\[21\] = \{([^}]*)\};" % S, text)
        masks[S] = _ints(m.group(1))
        assert len(masks[S]) == 21
    counts = {}
    for m in re.finditer(r"// S=(\d): [^\n]*?trunk layer (\d+) -> (\d+) \[([\d, ]+)\], head (\d+) -> (\d+)", text):
        counts[int(m.group(1))] = (int(m.group(2)), int(m.group(3)), _ints(m.group(4)), int(m.group(5)), int(m.group(6)))
    return {"order": table("kCellOrder"), "rowtab": table("kRowTab"), "lin": {2: lin[0:2], 3: lin[2:4]},
            "masks": masks, "counts": counts}


@pytest.fixture(scope="module")
def tables():
    return _parse()


def npt(S):
    return (S * CELLS + 15) // 16


def rows_of(tables, S):
    """LDS row -> (position, cell) or None for a pad, for all 16 * npt(S) rows, as the kernel lays them out"""
    n = 16 * npt(S)
    if S in ROW_TABLE_SIZES:
        tab = tables["rowtab"][S - 2]
        assert all(v == PAD for v in tab[n:])
        return [None if v == PAD else (v // CELLS, v % CELLS) for v in tab[:n]]
    if S < 4:   # position-major
        return [(r // CELLS, r % CELLS) if r < S * CELLS else None for r in range(n)]
    order = tables["order"][S]
    return [(r % S, order[r // S]) if r < S * CELLS else None for r in range(n)]


def on_board(cell, tap):
    h, w = divmod(cell, COLS)
    return 0 <= h + tap // 3 - 1 < ROWS and 0 <= w + tap % 3 - 1 < COLS


def plan(W, CT, n):
    """(position tile, co tile) tasks of wave W: Plan<W, CT, NPT> of net_c4.hip at its default knobs"""
    tt = n * CT
    first, nr = tt * W // 4, tt * (W + 1) // 4 - tt * W // 4
    if n <= 8:   # co-major
        return [((first + i) % n, (first + i) // n) for i in range(nr)]
    if CT == 4 and n <= 11:   # pair split
        m, r, pj, ph = n // 2, n % 2, W >> 1, W & 1
        return [(ph * m + i // 2, 2 * pj + (i & 1)) for i in range(2 * m)] + [(n - 1, 2 * pj + ph)] * r
    return [((first + i) // CT, (first + i) % CT) for i in range(nr)]   # position-major


def pairs_per_wave(masks, S, CT):
    kept = [9 - bin(m).count("1") for m in masks]
    return [sum(kept[pt] for pt, _ in plan(W, CT, npt(S))) for W in range(4)]


@pytest.mark.parametrize("S", SIZES)
def test_rows_are_a_bijection(tables, S):
    rows = rows_of(tables, S)
    real = [r for r in rows if r is not None]
    assert sorted(real) == [(s, c) for s in range(S) for c in range(CELLS)]
    assert len(rows) - len(real) == 16 * npt(S) - S * CELLS


@pytest.mark.parametrize("S", SIZES)
def test_skipped_taps_have_no_on_board_neighbour(tables, S):
    rows, masks = rows_of(tables, S), tables["masks"][S]
    assert all(m == 0 for m in masks[npt(S):])
    for t in range(npt(S)):
        assert not (masks[t] >> 4) & 1, "centre tap skipped"
        assert masks[t] < 512
        for tap in range(9):
            if (masks[t] >> tap) & 1:
                for rc in rows[16 * t:16 * t + 16]:
                    assert rc is None or not on_board(rc[1], tap), (S, t, tap, rc)


@pytest.mark.parametrize("S", ROW_TABLE_SIZES)
def test_row_tables_skip_a_sixth(tables, S):
    """S = 3: four tiles drop 3 taps each (12 of 72 pairs); S = 2: three tiles (9 of 54)"""
    skipped = sum(bin(m).count("1") for m in tables["masks"][S])
    assert skipped * 6 == 9 * npt(S)


def test_comment_counts_match(tables):
    none = [0] * 21
    for S in SIZES:
        if S == 1:
            assert S not in tables["counts"]
            continue
        before, after, per, head_before, head_after = tables["counts"][S]
        got = pairs_per_wave(tables["masks"][S], S, 4)
        assert per == got and after == max(got), (S, got)
        assert head_after == max(pairs_per_wave(tables["masks"][S], S, 3))
        if S in ROW_TABLE_SIZES:   # before: the position-major rows, nothing skipped
            assert before == max(pairs_per_wave(none, S, 4))
            assert head_before == max(pairs_per_wave(none, S, 3))


# the 16-lane groups that one ds_read_b128 is served in (lane = row in tile + 16 * K quarter)
_G = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
B128_GROUPS = [g for g in _G] + [[l + 32 for l in g] for g in _G]


@pytest.mark.parametrize("S", ROW_TABLE_SIZES)
def test_row_table_reads_are_conflict_free(tables, S):
    """every kept (tile, tap) B read, both K halves: the 16 lanes of a group hit 16 different 16-B granules of
    the 256-B bank row.  A row's chunk q sits at granule (row & 1) * 8 + (q ^ (row & 7)); an off-board or pad lane
    reads the zero block at the granule of residue (row + a * dh + b * dw) & 7, as make_geo does."""
    rows, masks, (a, b) = rows_of(tables, S), tables["masks"][S], tables["lin"][S]
    row_at = {rc: r for r, rc in enumerate(rows) if rc is not None}
    for t in range(npt(S)):
        for tap in range(9):
            if (masks[t] >> tap) & 1:
                continue
            dh, dw = tap // 3 - 1, tap % 3 - 1
            for half in (0, 1):
                for grp in B128_GROUPS:
                    granules = set()
                    for lane in grp:
                        p, q = 16 * t + (lane & 15), (lane >> 4) + 4 * half
                        rc = rows[p]
                        if rc is not None and on_board(rc[1], tap):
                            r = row_at[(rc[0], rc[1] + dh * COLS + dw)]
                        else:
                            r = (p + a * dh + b * dw) & 7
                        granules.add((r & 1) << 3 | ((q ^ r) & 7))
                    assert len(granules) == 16, (S, t, tap, half)


def test_generator_reproduces_the_row_tables(tables):
    spec = importlib.util.spec_from_file_location("gen_cell_orders", os.path.join(REPO, "scripts", "gen_cell_orders.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for S in ROW_TABLE_SIZES:
        tab, lin, masks = gen.search_rows(S)
        assert tab + [PAD] * (128 - len(tab)) == tables["rowtab"][S - 2]
        assert list(lin) == tables["lin"][S]
        assert masks + [0] * (21 - len(masks)) == tables["masks"][S]
        assert gen.conflicts(tab, S, lin, masks) == 0
