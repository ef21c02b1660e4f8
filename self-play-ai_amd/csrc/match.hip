// match.hip — play() (main.rs:54-135) between two evaluators over many games on
// the device-resident Connect4 search (search.hip): spai_match_run (spai.h "match").
#include <chrono>

#include "philox.h"
#include "search_internal.h"

namespace spai {
// Game g of the call owns trees 2g (player A's) and 2g + 1 (B's).  The games run in
// lockstep, so at every ply the games with A to move and those with B to move are
// two disjoint tree lists: chain 0 searches A's with A's evaluator, chain 1 B's
// with B's, side by side like the two halves of a self-play call.  Tail mode (a
// one-chain schedule) stays off.
namespace {
// the opening of pair `pair`: ply k plays the idx-th legal column, idx from one f32 multiply
__host__ __device__ inline c4::State opening_state(uint64_t seed, uint64_t pair, uint32_t plies, uint8_t *moves) {
    c4::State s{0, 0, 0, c4::kOngoing};
    for (uint32_t k = 0; k < plies; ++k) {
        const uint32_t legal = c4::legal_mask(s.x, s.o, s.status);
        const int n_legal = (int)c4::popc32(legal);
        int idx = (int)(sample_u01_f32(seed, pair, k) * (float)n_legal);
        idx = idx < n_legal - 1 ? idx : n_legal - 1;
        const int a = c4::kth_bit(legal, idx);
        c4::State ns = s;
        (void)c4::next_state(s, a, ns);
        s = ns;
        if (moves) moves[k] = (uint8_t)a;
    }
    return s;
}

// both trees of every game: an empty arena whose root is the position after the opening
__global__ void k_match_start(TreeView T, RootsOut R, uint32_t n_games, uint64_t gid_base, uint64_t seed,
                              uint32_t plies) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_games) return;
    const c4::State s = opening_state(seed, (gid_base + g) / 2, plies, nullptr);
    for (uint32_t t = 2 * g; t < 2 * g + 2; ++t) {
        tree_clear(T, R, t);
        root_position(R, t, s);
    }
}

// The move after a ply's search call, per searched tree t (the mover's; t ^ 1 is the
// opponent's tree of the same game, at the same position): the most-visited root
// child, ties to the last; for a game that goes on, the mover's tree re-rooted at it
// (use_subtree) and the opponent's at the same action's child -- the same index, its
// root being the same position -- or, while that root has no children (before the
// second player's first search), started anew at the new position.  The move step is
// k_advance's (search_internal.h "move step") but for the pick; the pick word without
// a visited child is kPickNone | 2 (the all-zero code of weighted_index_f32).
__global__ void k_match_advance(TreeView T, RootsOut R, const uint32_t *__restrict__ active, uint32_t n_active,
                                const uint32_t *err, const uint32_t *cache_fill, ChainCounts cc, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    move_header(err, cache_fill, cc, n_active, out);
    if (i >= n_active) return;
    const uint32_t t = active[i], opp = t ^ 1u;
    uint32_t *rec = out + 2 + (size_t)i * kMoveRec;
    uint32_t vis[c4::kActions];
    const uint32_t rw = move_load_root(T, t, rec, vis);
    uint32_t best = 0;   // (the visit counts past the children are 0)
    int idx = -1;
#pragma unroll
    for (int k = 0; k < c4::kActions; ++k)
        if (vis[k] >= best && vis[k] > 0) {
            best = vis[k];
            idx = k;
        }
    if (best == 0) {
        rec[kRecPick] = kPickNone | 2u;
        return;
    }
    c4::State cs;
    if (!move_apply(T, R, t, rw, idx, rec, cs)) return;
    const uint32_t ow = T.nodes[(size_t)opp * T.cap + T.root[opp]].w;
    if (ow != kNoChildren) R.root[opp] = (ow & 0xFFFFFFu) + (uint32_t)idx;
    else tree_clear(T, R, opp);
    root_position(R, opp, cs);
}
}  // namespace

int match_run(spai_engine *e, const spai_match_player *a, const spai_match_player *b, uint32_t n_games,
              uint64_t gid_base, const spai_match_config *cfg, spai_match_game *games, spai_match_stats *stats) {
    const auto t_start = std::chrono::steady_clock::now();
    const uint32_t W = 2 * n_games;
    SPAI_TRY(trees_create(e, W));
    EvalCache &C = e->cache;
    hipStream_t st = e->stream;
    // what each player's chain runs, but for its trees of the ply (launch) and its cache view (new_gens)
    Chain side[2] = {{0, 0, a->num_searches, a->eval, a->net, {}}, {0, 0, b->num_searches, b->eval, b->net, {}}};
    const uint32_t stride = std::max(side[0].iters, side[1].iters);
    SPAI_TRY(move_buffers(e, 2 + (size_t)W * kMoveRec + 2 * (size_t)stride));
    // Every return, errors included, leaves the streams idle, the cache without the match's entries and
    // the trees as trees_create leaves them (the host mirrors of the roots are not kept in a match).
    const Quiesce quiesce{e, W};
    // The evaluation cache, on when a net plays: each player's entries carry a
    // generation of their own, so neither is ever served the other's evaluations
    // (one generation when both play the same net).  The table is emptied before the
    // generations are drawn, so no older entry can carry either.
    SPAI_TRY(cache_prepare(e, side[0].kind == SPAI_EVAL_NET || side[1].kind == SPAI_EVAL_NET));
    const bool same_net = side[0].kind == SPAI_EVAL_NET && side[1].kind == SPAI_EVAL_NET && side[0].net == side[1].net;
    auto new_gens = [&]() -> int {
        SPAI_TRY(cache_clear(e));
        for (int h = 0; h < 2; ++h) {
            if (h && !same_net) C.gen = C.gen % 32767u + 1u;
            if (side[h].kind == SPAI_EVAL_NET) side[h].cache = cache_view(e);
        }
        return SPAI_OK;
    };
    if (C.buckets) SPAI_TRY(new_gens());
    const TreeView tv = tree_view(e);
    const RootsOut ro = roots_out(e);
    k_match_start<<<(n_games + 255) / 256, 256, 0, st>>>(tv, ro, n_games, gid_base, cfg->seed, cfg->opening_plies);
    SPAI_HIP(hipGetLastError());
    // the host's record of every game: position, moves, outcome
    std::vector<c4::State> pos(n_games);
    std::vector<spai_match_game> rec_games(n_games);
    for (uint32_t g = 0; g < n_games; ++g) {
        spai_match_game &G = rec_games[g];
        G = spai_match_game{};
        G.game_id = gid_base + g;
        G.a_moves_first = (int8_t)(((gid_base + g) & 1ull) == 0);
        G.n_moves = (uint8_t)cfg->opening_plies;
        pos[g] = opening_state(cfg->seed, (gid_base + g) / 2, cfg->opening_plies, G.moves);
    }
    // a ply's trees: player A's of the live games where A is to move, then B's of the others
    struct Ply {
        std::vector<uint32_t> trees;
        uint32_t cnt[2] = {0, 0};
    } ply[2];
    auto build = [&](const std::vector<uint32_t> &live_games, uint32_t ply_no, Ply &P) {
        P.trees.clear();
        for (uint32_t p = 0; p < 2; ++p) {
            for (uint32_t g : live_games)
                if ((((gid_base + g) ^ ply_no) & 1ull) == p) P.trees.push_back(2 * g + p);
            P.cnt[p] = (uint32_t)P.trees.size() - (p ? P.cnt[0] : 0u);
        }
    };
    auto launch = [&](const Ply &P, uint32_t *dst) -> int {
        if (cache_nearly_full(C)) SPAI_TRY(new_gens());
        const uint32_t na = (uint32_t)P.trees.size();
        side[0].cnt = side[1].off = P.cnt[0];   // (A's trees first)
        side[1].cnt = P.cnt[1];
        SPAI_TRY(chains_launch(e, P.trees.data(), side, 2, 0u, false, false));
        ChainCounts cc{{}, {}, stride};
        for (int h = 0; h < 2; ++h) {
            cc.p[h] = e->batch[h].iter_counts.p;
            cc.n[h] = P.cnt[h] ? side[h].iters : 0u;
        }
        k_match_advance<<<(na + 63) / 64, 64, 0, st>>>(tv, ro, e->active.p, na, e->err.p,
                                                       C.buckets ? C.ctr.p : nullptr, cc, e->move_out.p);
        SPAI_HIP(hipGetLastError());
        const size_t words = 2 + (size_t)na * kMoveRec + 2 * (size_t)stride;
        SPAI_HIP(hipMemcpyAsync(dst, e->move_out.p, words * 4, hipMemcpyDeviceToHost, st));
        return SPAI_OK;
    };
    std::vector<uint32_t> live_games(n_games), next_games;
    for (uint32_t g = 0; g < n_games; ++g) live_games[g] = g;
    std::vector<uint8_t> ended(n_games, 0);
    double sims[2] = {0, 0}, evals[2] = {0, 0};
    uint32_t ply_no = cfg->opening_plies;
    int cur = 0;
    build(live_games, ply_no, ply[0]);
    SPAI_TRY(launch(ply[0], e->h_move[0]));
    while (!live_games.empty()) {
        const Ply &P = ply[cur];
        const uint32_t na = (uint32_t)P.trees.size();
        const uint32_t *mo = e->h_move[cur];
        SPAI_HIP(hipStreamSynchronize(st));
        SPAI_TRY(check_device_errors(e, mo[0]));
        const uint32_t *counts = move_rec(mo, na);
        bool stop = false;
        double net_served = 0, net_fwd = 0;   // the leaves of the players that are nets: the cache's lookups
        for (uint32_t p = 0, i = 0; p < 2; ++p) {
            if (!P.cnt[p]) continue;
            double served = 0, fwd = 0;
            for (uint32_t k = 0; k < P.cnt[p]; ++k, ++i) {
                const uint32_t *rec = move_rec(mo, i);
                served += rec[kRecEvals];
                stop |= (rec[kRecPick] & kPickNone) != 0;
                ended[P.trees[i] / 2] = pick_status(rec[kRecPick]) != c4::kOngoing;
            }
            for (uint32_t j = 0; j < side[p].iters; ++j) fwd += counts[(size_t)p * stride + j];
            sims[p] += (double)P.cnt[p] * side[p].iters;
            evals[p] += served;
            if (side[p].kind == SPAI_EVAL_NET) {
                net_served += served;
                net_fwd += fwd;
            }
        }
        cache_account(e, net_served, net_fwd, mo[1]);
        SPAI_CHECK(!stop, SPAI_ERR_NAN, "no visited root child to play (num_searches = 1 visits none)");
        // the games that go on, in order, search their next ply while the host records this one
        next_games.clear();
        for (uint32_t g : live_games)
            if (!ended[g]) next_games.push_back(g);
        if (!next_games.empty()) {
            build(next_games, ply_no + 1, ply[cur ^ 1]);
            SPAI_TRY(launch(ply[cur ^ 1], e->h_move[cur ^ 1]));
        }
        for (uint32_t i = 0; i < na; ++i) {
            const uint32_t t = P.trees[i], g = t / 2, p = t & 1u;
            const uint32_t *rec = move_rec(mo, i);
            const c4::State rs = pos[g];
            const int mv = pick_action(rec[kRecPick]);
            c4::State cs;
            SPAI_CHECK(root_children(rec[kRecRoot]) == c4::popc32(c4::legal_mask(rs.x, rs.o, rs.status)) &&
                           move_replays(rec, rs, cs),
                       SPAI_ERR_INVALID, "internal: game %u's device move does not replay", g);
            spai_match_game &G = rec_games[g];
            SPAI_CHECK(G.n_moves < c4::kCells, SPAI_ERR_INVALID, "internal: game %u longer than 42 plies", g);
            G.moves[G.n_moves++] = (uint8_t)mv;
            pos[g] = cs;
            if (cs.status == c4::kWon) G.result_a = p == 0 ? 1 : -1;
        }
        live_games.swap(next_games);
        cur ^= 1;
        ++ply_no;
    }
    if (games)
        for (uint32_t g = 0; g < n_games; ++g) games[g] = rec_games[g];
    if (stats) {
        *stats = spai_match_stats{};
        for (const spai_match_game &G : rec_games) {
            const int f = G.a_moves_first ? 0 : 1;
            (G.result_a > 0 ? stats->a_wins : G.result_a < 0 ? stats->b_wins : stats->draws)[f] += 1;
        }
        for (int p = 0; p < 2; ++p) {
            stats->sims[p] = sims[p];
            stats->evals[p] = evals[p];
        }
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
    return SPAI_OK;
}

}  // namespace spai
