"""Cell orders for the fused Connect4 forward (net_c4.hip): which board cell each
LDS row group holds, per group size S, so that as many 16-row position tiles as
possible have NO on-board neighbour for some 3x3 tap -- those (tile, tap) MFMAs
and their B-fragment reads are skipped (the products would be exact zeros).

For S >= 4 (cell-major groups) LDS row r of a group of S positions holds cell
kCellOrder[S][r / S] of position r % S.  The search maximises the skipped (tile,
tap) pairs while keeping the four waves' MFMA counts balanced under the kernel's
task plans (Plan<W, CT, NPT>: co-major for NPT <= 8, pair split up to 11 tiles,
position-major above), for the trunk convs (CT = 4) and, at a quarter of the
weight, the head conv as it ran when the tables were searched (its own CT = 3
plan; since round 3 the head runs on the trunk plan without co tile 3, so the
trunk term is the one that counts).  At S = 4 the order index's parity must equal
the cell's checkerboard colour (h + w) & 1: a tile then holds row groups 4t..4t+3
whose neighbours for any tap alternate in parity, which keeps the B-fragment reads
bank-conflict free (net_c4.hip make_geo).

S = 2 and 3 (row tables): a cell-major tile would need 8 whole cells of one edge
at S = 2 (the longest edge has 7), and at S = 3 tile boundaries fall inside cells.
There kRowTab[S][r] names the (position, cell) of every LDS row r, or a pad
row, with pads allowed anywhere.  One tile per board edge (S = 3: all four; S = 2:
three) holds only rows of that edge, any positions mixed, and drops that edge's 3
taps: 72 -> 60 (tile, tap) pairs per wave at S = 3, 54 -> 45 at S = 2 (co-major
plan: every wave walks all tiles, so the waves stay balanced).  Bank conflicts: a
ds_read_b128 is served in 16-lane groups that each hold the lanes of two 8-row
"octets" of a tile (rows 4..11 and rows 0..3, 12..15) at different K quarters,
and lanes of different K quarters never share a 16-B granule under the row&7 XOR
swizzle; so a tap's read is conflict-free iff the neighbour rows of each octet are
distinct mod 8.  The search fixes row & 7 = (a*h + b*w + c*s) & 7 for the row of
cell (h, w) of position s: a tap then shifts every row's residue by the constant
a*dh + b*dw, an octet's 8 distinct residues stay distinct, and an off-board
neighbour (or a pad row) reads the zero block at the granule of that shifted
residue.  For each (a, b, c) the rows of one residue are matched to the 2 slots
that each tile has for it (edge tiles take only their edge's rows); kRowLin[S] =
{a, b}.  conflicts() counts what is left by brute force over the hardware's lane
groups: 0 for both sizes.

S = 1 keeps the position-major rows of the identity order (16 consecutive cells
per tile: no tile lies on one board edge, nothing to skip).  Deterministic
(fixed seeds); prints the C++ tables.
    python scripts/gen_cell_orders.py > /tmp/orders.txt
"""
import random

R, C = 6, 7
CELLS = [(h, w) for h in range(R) for w in range(C)]
TAPS = [(dh, dw) for dh in (-1, 0, 1) for dw in (-1, 0, 1)]   # tap index = (dh+1)*3 + (dw+1), as net_c4.hip


def off_board(c, t):
    return not (0 <= c[0] + t[0] < R and 0 <= c[1] + t[1] < C)


def npt(S):
    return (S * 42 + 15) // 16


def plan(W, CT, n):
    """(position tile, co tile) tasks of wave W: net_c4.hip Plan<W, CT, NPT>"""
    mode = 1 if n <= 8 else (2 if CT == 4 and n <= 11 else 0)
    tt = n * CT
    if mode == 2:
        m, r, pj, ph = n // 2, n % 2, W >> 1, W & 1
        return [(ph * m + i // 2, 2 * pj + (i & 1)) if i < 2 * m else (n - 1, 2 * pj + ph) for i in range(2 * m + r)]
    first, nr = tt * W // 4, tt * (W + 1) // 4 - tt * W // 4
    if mode == 1:
        return [((first + i) % n, (first + i) // n) for i in range(nr)]
    return [((first + i) // CT, (first + i) % CT) for i in range(nr)]


def skip_masks(order, S):
    out = []
    for t in range(npt(S)):
        m = 0
        for ti, tap in enumerate(TAPS):
            rows = [r for r in range(16 * t, 16 * t + 16) if r < 42 * S]
            if rows and all(off_board(order[r // S], tap) for r in rows):
                m |= 1 << ti
        out.append(m)
    return out


def cost(order, S, CT=4):
    masks, n = skip_masks(order, S), npt(S)
    per = [sum(sum(1 for ti in range(9) if not (masks[pt] >> ti) & 1) for pt, _ in plan(W, CT, n)) for W in range(4)]
    return max(per), per, masks


def score(order, S):
    return cost(order, S)[0] + 0.25 * cost(order, S, 3)[0]


def colour_ok(o):
    return all(((h + w) & 1) == (i & 1) for i, (h, w) in enumerate(o))


def search(S, iters, seed):
    rnd = random.Random(seed)
    checker = S == 4
    ring = ([(0, w) for w in range(7)] + [(h, 6) for h in range(1, 6)] + [(5, w) for w in range(5, -1, -1)]
            + [(h, 0) for h in range(4, 0, -1)])
    inner = [(h, w) for h in range(1, 5) for w in range(1, 6)]
    best = None
    for start in range(22):
        for d in (1, -1):
            rr = [ring[(start + d * i) % 22] for i in range(22)]
            for split in range(23):
                o = rr[:split] + inner[:10] + rr[split:] + inner[10:]
                if checker:   # re-deal the cells onto the indices of their colour, keeping their relative order
                    black = [x for x in o if not (x[0] + x[1]) & 1]
                    white = [x for x in o if (x[0] + x[1]) & 1]
                    o = [black[i // 2] if i % 2 == 0 else white[i // 2] for i in range(42)]
                c = score(o, S)
                if best is None or c < best[0]:
                    best = (c, o)
    cur, curc = list(best[1]), best[0]
    for _ in range(iters):
        i, j = rnd.randrange(42), rnd.randrange(42)
        if checker and (i & 1) != (j & 1):
            continue
        cur[i], cur[j] = cur[j], cur[i]
        c = score(cur, S)
        if c <= curc:
            curc = c
        else:
            cur[i], cur[j] = cur[j], cur[i]
    return curc, cur


# ---------------------------------------------------------------- row tables (S = 2, 3)
ROW_SIZES = (2, 3)
ROW_SEED = 7
PAD = 255
EDGES = (("bottom", lambda h, w: h == 0), ("top", lambda h, w: h == R - 1),
         ("left", lambda h, w: w == 0), ("right", lambda h, w: w == C - 1))
# the 16-lane groups that serve one ds_read_b128 (lane = column + 16 * K quarter)
B128_GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
B128_GROUPS = B128_GROUPS + tuple([l + 32 for l in grp] for grp in B128_GROUPS)


def row_masks(tab, S):
    """tap_skip masks of a row table: taps whose neighbour is off the board for every non-pad row of the tile"""
    out = []
    for t in range(npt(S)):
        cells = [divmod(code % 42, C) for code in tab[16 * t:16 * t + 16] if code != PAD]
        out.append(sum(1 << ti for ti, tap in enumerate(TAPS) if all(off_board(c, tap) for c in cells)))
    return out


def row_cost(masks, S, CT=4):
    n = npt(S)
    per = [sum(9 - bin(masks[pt]).count("1") for pt, _ in plan(W, CT, n)) for W in range(4)]
    return max(per), per


def conflicts(tab, S, lin, masks):
    """extra LDS passes of the B-fragment reads of all kept (tile, tap) pairs, both K halves (0 = conflict-free)"""
    row_of = {code: r for r, code in enumerate(tab) if code != PAD}
    extra = 0
    for t in range(npt(S)):
        for ti, (dh, dw) in enumerate(TAPS):
            if (masks[t] >> ti) & 1:
                continue
            for half in (0, 1):
                for grp in B128_GROUPS:
                    hit = {}
                    for lane in grp:
                        p, q = 16 * t + (lane & 15), (lane >> 4) + 4 * half
                        code = tab[p]
                        s, (h, w) = code // 42, divmod(code % 42, C)
                        if code != PAD and not off_board((h, w), (dh, dw)):
                            r = row_of[s * 42 + (h + dh) * C + w + dw]
                        else:   # the zero block, at the granule of the row residue a neighbour would have
                            r = (p + lin[0] * dh + lin[1] * dw) & 7
                        granule = (r & 1) << 3 | ((q ^ r) & 7)
                        hit[granule] = hit.get(granule, 0) + 1
                    extra += max(hit.values()) - 1
    return extra


def edge_matching(items, edges):
    """most rows of one residue placed in the edge tiles' 2 slots each: {(edge tile, slot): item}"""
    slot = {}

    def place(it, seen):
        for k, e in enumerate(edges):
            if not EDGES[e][1](it[1], it[2]):
                continue
            for j in range(2):
                if (k, j) in seen:
                    continue
                seen.add((k, j))
                if (k, j) not in slot or place(slot[(k, j)], seen):
                    slot[(k, j)] = it
                    return True
        return False

    for it in items:
        place(it, set())
    return slot


def col_of(res, j):
    """column (row within the tile) with residue res in octet j: rows 4..11, and rows 0..3, 12..15"""
    return 4 + ((res - 4) & 7) if j == 0 else (res if res < 4 else res + 8)


def row_layout(S, edges, lin):
    """rows of every tile as {tile: {col: item}} with edge tile k = tile k, or None if (a, b, c) does not fit"""
    a, b, c = lin
    n, ne = npt(S), len(edges)
    tiles = [dict() for _ in range(n)]
    for res in range(8):
        items = [(s, h, w) for s in range(S) for h in range(R) for w in range(C) if (a * h + b * w + c * s) % 8 == res]
        slot = edge_matching(items, edges)
        rest = [it for it in items if it not in slot.values()]
        if len(rest) > 2 * (n - ne):
            return None
        for (k, j), it in slot.items():
            tiles[k][col_of(res, j)] = it
        for i, it in enumerate(rest):   # two slots per tile, tile by tile
            tiles[ne + i // 2][col_of(res, i % 2)] = it
    return tiles


def search_rows(S, seed=ROW_SEED):
    """(row table, (a, b), masks): the most edge tiles that fit conflict-free, then the fewest (tile, tap) pairs of
    the busiest wave in the trunk plan and the CT = 3 head plan over the edge tiles' places; ties by the seed"""
    import itertools
    rnd = random.Random(seed * 16 + S)
    n = npt(S)
    for ne in (4, 3, 2, 1):
        fits = []
        for edges in itertools.combinations(range(4), ne):
            for lin in itertools.product(range(8), repeat=3):
                tiles = row_layout(S, edges, lin)
                if tiles is not None:
                    fits.append((edges, lin, tiles))
        if fits:
            break
    else:
        raise RuntimeError("no row layout")
    edges, lin, tiles = fits[rnd.randrange(len(fits))]
    best = None
    for where in itertools.combinations(range(n), ne):   # tile indices of the edge tiles
        order = list(where) + [t for t in range(n) if t not in where]   # order[k] = tile index of layout tile k
        tab = [PAD] * (16 * n)
        for k, rows in enumerate(tiles):
            for col, (s, h, w) in rows.items():
                tab[16 * order[k] + col] = s * 42 + h * C + w
        masks = row_masks(tab, S)
        key = (row_cost(masks, S)[0], row_cost(masks, S, 3)[0])
        if best is None or key < best[0]:
            best = (key, tab, masks)
    _, tab, masks = best
    assert sorted(x for x in tab if x != PAD) == list(range(42 * S))
    return tab, lin[:2], masks


def main():
    orders, masks, rows, lins = {}, {}, {}, {}
    for S in range(1, 9):
        if S <= 3:   # no cell order: position-major rows (nothing to skip) or a row table
            orders[S], masks[S] = [h * 7 + w for h, w in CELLS], [0] * npt(S)
            if S not in ROW_SIZES:
                print(f"// S={S}: position-major rows, identity order")
                continue
            rows[S], lins[S], masks[S] = search_rows(S)
            none = [0] * npt(S)
            print(f"// S={S}: row table, max MFMA tile-taps per wave and trunk layer {row_cost(none, S)[0]} -> "
                  f"{row_cost(masks[S], S)[0]} {row_cost(masks[S], S)[1]}, head {row_cost(none, S, 3)[0]} -> "
                  f"{row_cost(masks[S], S, 3)[0]}; B-read bank conflicts {conflicts(rows[S], S, lins[S], masks[S])}")
            continue
        o = min((search(S, 8000, seed) for seed in range(4)), key=lambda x: x[0])[1]
        assert S != 4 or colour_ok(o)
        orders[S] = [h * 7 + w for h, w in o]
        masks[S] = skip_masks(o, S)
        new = cost(o, S)
        print(f"// S={S}: max MFMA tile-taps per wave and trunk layer {cost(CELLS, S)[0]} -> {new[0]} {new[1]}, "
              f"head {cost(CELLS, S, 3)[0]} -> {cost(o, S, 3)[0]}")
    print("constexpr uint8_t kCellOrder[9][42] = {")
    print("    {" + ", ".join(["0"] * 42) + "},")
    for S in range(1, 9):
        print("    {" + ", ".join(map(str, orders[S])) + "},")
    print("};")
    print("constexpr uint8_t kRowTab[2][128] = {   // [S - 2]")
    for S in ROW_SIZES:
        print("    {" + ", ".join(map(str, rows[S] + [PAD] * (128 - len(rows[S])))) + "},")
    print("};")
    print("constexpr int8_t kRowLin[2][2] = {" + ", ".join("{%d, %d}" % tuple(lins[S]) for S in ROW_SIZES) + "};   // [S - 2]")
    print("__host__ __device__ constexpr uint16_t tap_skip(int S, int t) {")
    for S in range(1, 9):
        print(f"    constexpr uint16_t m{S}[21] = {{" + ", ".join(map(str, masks[S] + [0] * (21 - len(masks[S])))) + "};")
    print("    return S == 1 ? m1[t] : S == 2 ? m2[t] : S == 3 ? m3[t] : S == 4 ? m4[t] : S == 5 ? m5[t] : S == 6 ? m6[t]"
          " : S == 7 ? m7[t] : m8[t];")
    print("}")


if __name__ == "__main__":
    main()
