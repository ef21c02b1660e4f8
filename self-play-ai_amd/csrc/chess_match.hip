// chess_match.hip — play() (main.rs:54-135, its chess variant) between two
// evaluators over many chess games on the device-resident chess search
// (chess_search.hip): spai_chess_match_run (spai.h "chess match").
//
// Game g of the call owns trees 2g (player A's) and 2g + 1 (B's).  The games run
// in lockstep, so at every ply the games with A to move and those with B to move
// are two disjoint tree lists: chain 0 searches A's trees with A's evaluator on the
// engine's stream, chain 1 B's with B's on the match's own stream and leaf batch.
// A chain's move kernel touches both trees of its games and of no other game, so
// the two streams share nothing within a ply.  Per ply the host enqueues both
// chains -- tree list up, search, move kernel, move records (16 B per game) back,
// all through pinned buffers so that no copy waits for a stream -- and only then
// joins the two streams.
#include <chrono>

#include "chess_search_internal.h"
#include "philox.h"

namespace spai {
namespace chess {
namespace {

// move record flags (rec.y >> 8)
constexpr uint32_t kRecNoVisit = 1;     // no visited root child: nothing to play
constexpr uint32_t kRecRestart = 2;     // the opponent's tree was started anew
constexpr uint32_t kRecMismatch = 4;    // the opponent's child carries another move code (never, by construction)

// Both trees of every game: Tree::with_root_state of the game's position after the
// opening, history included.  One wave per game.  The start position is
// start[pair - pair_base] (empty transposition table) or State::default(); ply k of
// the opening plays the idx-th legal move in MoveGen order, idx from one f32
// multiply of the Philox uniform of (seed, pair, k).
// rec[g] = status | reps << 8, opening move 0 | move 1 << 16, move 2, plies played.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_cmatch_start(TV T, uint32_t n_games, uint64_t gid_base,
                                                                     uint64_t seed, uint32_t plies,
                                                                     const Board *__restrict__ start, uint4 *rec,
                                                                     uint32_t *err) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= n_games) return;
    const uint64_t pair = (gid_base + g) / 2;
    Board b;
    if (start) b = start[pair - gid_base / 2];
    else start_board(b);
    b.status = 0;
    if (plies > T.max_hist) {
        if (lane == 0) atomicOr(err, kErrHist);
        return;
    }
    uint64_t hk[3] = {0, 0, 0};   // list hashes of the opening's positions (plies <= 3)
    uint32_t mk[3] = {0, 0, 0};
    uint32_t played = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        if (k >= plies) break;
        const GenOut g0 = wave_movegen(b, nullptr, lane);
        if (g0.n == 0) break;   // (no game ends within 3 plies of the start position)
        int idx = (int)(sample_u01_f32(seed, pair, k) * (float)g0.n);
        idx = idx < g0.n - 1 ? idx : g0.n - 1;
        int sel = -1;
        (void)wave_movegen(b, lane, [&](int off, int m) {
            if (off == idx) sel = m;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sel = max(sel, __shfl_xor(sel, o, 64));
        hk[k] = g0.hash;
        mk[k] = (uint32_t)sel;
        apply_move(b, sel);
        played = k + 1;
    }
    const GenOut g1 = wave_movegen(b, nullptr, lane);
    uint32_t reps = 1;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) reps += (k < played && hk[k] == g1.hash) ? 1u : 0u;
    b.status = (uint8_t)status_from(g1, reps, b);
    if (lane == 0) {
        for (uint32_t t = 2 * g; t < 2 * g + 2; ++t) {
            uint64_t *h = T.hist + (size_t)t * T.max_hist;
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                if (k < played) h[k] = hk[k];
            tree_one_node(T, t, b, reps, played);
        }
        rec[g] = make_uint4((uint32_t)b.status | (reps << 8), mk[0] | (mk[1] << 16), mk[2], played);
    }
}

// The move after a ply's search, per searched tree t (the mover's; t ^ 1 is the
// opponent's tree of the same game, at the same position), one wave per game:
// the most-visited root child, ties to the last (a wave reduction over at most
// 218 children); the mover's tree re-rooted at it (advance_step, k_cadvance's
// step); the opponent's tree advanced to the same child index -- its root being
// the same position, its children are the same MoveGen list -- or, while that root
// has no children (before the second player's first search), started anew at the
// new position with the mover's history.
// rec[gi] = move | child index << 16, status | flags << 8, reps, root children.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_cmatch_move(TV T, const uint32_t *__restrict__ active,
                                                                    uint32_t n_active, uint4 *rec, uint32_t *err) {
    const int lane = threadIdx.x & 63;
    const uint32_t gi = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (gi >= n_active) return;
    const uint32_t t = active[gi], opp = t ^ 1u;
    const size_t base = tbase(T, t);
    const uint32_t r = T.root[t];
    const uint32_t nch = T.nodes[base + r].w >> 16;
    const uint32_t f = nch ? T.first[base + r] : 0u;
    uint32_t bv = 0;
    int bi = -1;
    for (uint32_t i = lane; i < nch; i += 64) {
        const uint32_t v = T.nodes[base + f + i].x;
        if (v > 0 && v >= bv) {   // later children win ties
            bv = v;
            bi = (int)i;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t ov = __shfl_xor(bv, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (bi < 0) {
        if (lane == 0) rec[gi] = make_uint4(0u, kRecNoVisit << 8, 0u, nch);
        return;
    }
    const uint32_t mv = T.nodes[base + f + (uint32_t)bi].w & 0xFFFFu;
    // the mover's history before the step: what a restarted opponent tree takes over
    const uint32_t hn = T.hist_n[t];
    const uint64_t rh = T.nhash[base + r];
    // the opponent's root before anything moves
    const size_t obase = tbase(T, opp);
    const uint32_t orr = T.root[opp];
    const uint32_t onch = T.nodes[obase + orr].w >> 16;
    const uint32_t ohn = T.hist_n[opp];
    if (onch && ohn >= T.max_hist) {
        if (lane == 0) atomicOr(err, kErrHist);
        return;
    }
    Board b;
    uint32_t reps;
    if (!advance_step(T, t, (uint32_t)bi, lane, err, b, reps)) return;
    uint32_t flags = 0;
    if (onch) {
        const uint32_t child = T.first[obase + orr] + (uint32_t)bi;
        if (onch != nch || (T.nodes[obase + child].w & 0xFFFFu) != mv) flags |= kRecMismatch;
        if (lane == 0) {
            T.hist[(size_t)opp * T.max_hist + ohn] = T.nhash[obase + orr];
            T.hist_n[opp] = ohn + 1;
            T.root[opp] = child;
            T.root_board[opp] = b;
            T.root_reps[opp] = reps;
        }
    } else {
        flags |= kRecRestart;
        const uint64_t *src = T.hist + (size_t)t * T.max_hist;
        uint64_t *dst = T.hist + (size_t)opp * T.max_hist;
        for (uint32_t i = lane; i < hn; i += 64) dst[i] = src[i];   // (entries the step did not write)
        if (lane == 0) {
            dst[hn] = rh;
            tree_one_node(T, opp, b, reps, hn + 1);
        }
    }
    if (lane == 0) rec[gi] = make_uint4(mv | ((uint32_t)bi << 16), (uint32_t)b.status | (flags << 8), reps, nch);
}

// every return of a match, errors included, leaves both streams idle and both error words clear
struct Quiesce {
    spai_chess *e;
    ~Quiesce() {
        MatchBufs &M = e->match;
        (void)hipStreamSynchronize(e->stream);
        if (M.stream) (void)hipStreamSynchronize(M.stream);
        (void)hipMemsetAsync(e->err.p, 0, 4, e->stream);
        if (M.err.p) (void)hipMemsetAsync(M.err.p, 0, 4, e->stream);
        (void)hipStreamSynchronize(e->stream);
    }
};

void free_pinned(MatchBufs &M) {
    for (int p = 0; p < 2; ++p) {
        if (M.h_list[p]) (void)hipHostFree(M.h_list[p]);
        if (M.h_rec[p]) (void)hipHostFree(M.h_rec[p]);
        M.h_list[p] = nullptr;
        M.h_rec[p] = nullptr;
    }
    if (M.h_srec) (void)hipHostFree(M.h_srec);
    M.h_srec = nullptr;
}

int match_buffers(spai_chess *e, uint32_t n_games) {
    MatchBufs &M = e->match;
    if (!M.stream) SPAI_HIP(hipStreamCreateWithFlags(&M.stream, hipStreamNonBlocking));
    if (!M.err.p) {
        SPAI_TRY(M.err.alloc(1));
        SPAI_HIP(hipMemset(M.err.p, 0, 4));
    }
    Batch &B = M.batch;
    if (M.cap < n_games) {
        M.cap = 0;
        B.cap = 0;
        SPAI_TRY(B.tree.alloc(n_games));
        SPAI_TRY(B.x.alloc((size_t)n_games * 64 * kInCh));
        SPAI_TRY(B.logits.alloc((size_t)n_games * kPolicy));
        SPAI_TRY(B.value.alloc(n_games));
        SPAI_TRY(M.active.alloc(n_games));
        SPAI_TRY(M.rec[0].alloc(n_games));
        SPAI_TRY(M.rec[1].alloc(n_games));
        SPAI_TRY(M.start_rec.alloc(n_games));
        free_pinned(M);
        for (int p = 0; p < 2; ++p) {
            SPAI_HIP(hipHostMalloc((void **)&M.h_list[p], sizeof(uint32_t) * n_games, hipHostMallocDefault));
            SPAI_HIP(hipHostMalloc((void **)&M.h_rec[p], sizeof(uint4) * n_games, hipHostMallocDefault));
        }
        SPAI_HIP(hipHostMalloc((void **)&M.h_srec, sizeof(uint4) * n_games, hipHostMallocDefault));
        B.cap = n_games;
        M.cap = n_games;
    }
    return SPAI_OK;
}

}  // namespace

void match_release(spai_chess *e) {
    MatchBufs &M = e->match;
    Batch &B = M.batch;
    B.counts.release();
    B.tree.release();
    B.x.release();
    B.xf.release();
    B.logits.release();
    B.value.release();
    B.cap = 0;
    M.active.release();
    M.err.release();
    M.rec[0].release();
    M.rec[1].release();
    M.start_rec.release();
    M.start.release();
    free_pinned(M);
    M.cap = 0;
    if (M.stream) (void)hipStreamDestroy(M.stream);
    M.stream = nullptr;
}

int match_set_one_stream(spai_chess *e, int on) {
    e->match.one_stream = on != 0;
    return SPAI_OK;
}

int match_run(spai_chess *e, const spai_chess_match_player *a, const spai_chess_match_player *b, uint32_t n_games,
              uint64_t gid_base, const spai_chess_match_config *cfg, spai_chess_match_game *games, uint16_t *moves,
              spai_chess_match_stats *stats) {
    const auto t_start = std::chrono::steady_clock::now();
    const uint32_t W = 2 * n_games;
    // the start positions, checked before anything on the device changes
    const uint32_t n_pairs = (uint32_t)((gid_base + n_games - 1) / 2 - gid_base / 2) + 1;
    std::vector<Board> h_start;
    if (cfg->start) {
        h_start.resize(n_pairs);
        for (uint32_t i = 0; i < n_pairs; ++i) {
            h_start[i] = from_abi(cfg->start[i]);
            SPAI_CHECK(popc(h_start[i].pc[KING] & h_start[i].col[WHITE]) == 1 &&
                           popc(h_start[i].pc[KING] & h_start[i].col[BLACK]) == 1,
                       SPAI_ERR_INVALID, "start %u: each side needs exactly one king", i);
        }
    }
    // the host's record of every game and the ply's lists: declared before the guard below, so
    // they outlive its synchronisation on every return
    std::vector<spai_chess_match_game> G(n_games);
    std::vector<std::vector<uint16_t>> mv(n_games);
    std::vector<uint32_t> live, next;
    uint32_t f0 = 0;
    SPAI_TRY(trees_create(e, W));
    SPAI_TRY(match_buffers(e, n_games));
    MatchBufs &M = e->match;
    const Quiesce quiesce{e};
    const bool one_stream = M.one_stream;   // both chains on the engine's stream (spai_chess_match_set_one_stream)
    // what each player's chain runs, but for its trees of the ply; no timer: the engine's is not sampled
    Chain side[2];
    side[0] = engine_chain(e, 0, a->num_searches);
    side[0].kind = a->eval;
    side[0].net = a->eval == SPAI_EVAL_NET ? a->net : nullptr;
    side[0].timer = nullptr;
    side[1].stream = one_stream ? e->stream : M.stream;
    side[1].active = M.active.p;
    side[1].batch = &M.batch;
    side[1].err = M.err.p;
    side[1].kind = b->eval;
    side[1].net = b->eval == SPAI_EVAL_NET ? b->net : nullptr;
    side[1].sims = b->num_searches;
    const TV tv = view(e);
    const Board *d_start = nullptr;
    if (cfg->start) {
        if (M.start.n < n_pairs) SPAI_TRY(M.start.alloc(n_pairs));
        SPAI_HIP(hipMemcpyAsync(M.start.p, h_start.data(), sizeof(Board) * n_pairs, hipMemcpyHostToDevice, e->stream));
        d_start = M.start.p;
    }
    k_cmatch_start<<<blocks_for(n_games), 64 * kWavesPerBlock, 0, e->stream>>>(
        tv, n_games, gid_base, cfg->seed, cfg->opening_plies, d_start, M.start_rec.p, e->err.p);
    SPAI_HIP(hipGetLastError());
    const uint4 *srec = M.h_srec;
    SPAI_HIP(hipMemcpyAsync(M.h_srec, M.start_rec.p, sizeof(uint4) * n_games, hipMemcpyDeviceToHost, e->stream));
    SPAI_HIP(hipMemcpyAsync(&f0, e->err.p, 4, hipMemcpyDeviceToHost, e->stream));
    SPAI_HIP(hipStreamSynchronize(e->stream));
    SPAI_TRY(err_code(e, f0));
    for (uint32_t g = 0; g < n_games; ++g) {
        const uint4 r = srec[g];
        SPAI_CHECK((r.x & 0xFFu) == SPAI_ONGOING, SPAI_ERR_INVALID, "game %u: the start position is not Ongoing (status %u)",
                   g, r.x & 0xFFu);
        SPAI_CHECK(r.w == cfg->opening_plies, SPAI_ERR_INVALID, "internal: game %u's opening stopped at ply %u", g, r.w);
        G[g] = spai_chess_match_game{};
        G[g].game_id = gid_base + g;
        G[g].a_moves_first = (int8_t)(((gid_base + g) & 1ull) == 0);
        G[g].n_moves = r.w;
        const uint16_t om[3] = {(uint16_t)(r.y & 0xFFFFu), (uint16_t)(r.y >> 16), (uint16_t)(r.z & 0xFFFFu)};
        mv[g].assign(om, om + r.w);
    }
    for (uint32_t g = 0; g < n_games; ++g) {
        if (cfg->max_plies && G[g].n_moves >= cfg->max_plies) G[g].adjudicated = 1;
        else live.push_back(g);
    }
    // the leaf counters sized now: an allocation inside the ply loop would join the device
    for (int p = 0; p < 2; ++p)
        if (side[p].batch->counts.n < side[p].sims) SPAI_TRY(side[p].batch->counts.alloc(side[p].sims));
    // likewise the fp32 planes of a chain whose player's net is fp32 (each chain follows its own net)
    for (int p = 0; p < 2; ++p) SPAI_TRY(batch_attach(*side[p].batch, side[p].net));
    uint32_t *const *list = M.h_list;
    uint4 *const *hrec = M.h_rec;
    double sims[2] = {0, 0}, evals[2] = {0, 0};
    for (uint32_t searched = 0; !live.empty(); ++searched) {
        // a ply's trees: player A's of the live games where A is to move, B's of the others
        side[0].n = side[1].n = 0;
        for (uint32_t g : live) {
            const uint32_t p = (uint32_t)((gid_base + g + searched) & 1ull);
            list[p][side[p].n++] = 2 * g + p;
        }
        // both chains enqueued before the host waits for either (every copy is pinned, none blocks)
        for (int p = 0; p < 2; ++p) {
            Chain &C = side[p];
            if (!C.n) continue;   // an empty chain launches nothing
            SPAI_HIP(hipMemcpyAsync((void *)C.active, list[p], 4 * C.n, hipMemcpyHostToDevice, C.stream));
            SPAI_TRY(chain_launch(e, C));
            k_cmatch_move<<<blocks_for(C.n), 64 * kWavesPerBlock, 0, C.stream>>>(tv, C.active, C.n, M.rec[p].p, C.err);
            SPAI_HIP(hipGetLastError());
            SPAI_HIP(hipMemcpyAsync(hrec[p], M.rec[p].p, sizeof(uint4) * C.n, hipMemcpyDeviceToHost, C.stream));
        }
        for (int p = 0; p < 2; ++p) {
            double ev = 0;
            SPAI_TRY(chain_finish(e, side[p], &ev));
            evals[p] += ev;
            sims[p] += (double)side[p].n * side[p].sims;
        }
        next.clear();
        for (int p = 0; p < 2; ++p)
            for (uint32_t i = 0; i < side[p].n; ++i) {
                const uint4 r = hrec[p][i];
                const uint32_t flags = r.y >> 8;
                SPAI_CHECK(!(flags & kRecNoVisit), SPAI_ERR_NAN,
                           "no visited root child to play (num_searches = 1 visits none)");
                SPAI_CHECK(!(flags & kRecMismatch), SPAI_ERR_INVALID,
                           "internal: the two trees of game %u disagree on the move", list[p][i] / 2);
            }
        for (int p = 0; p < 2; ++p)
            for (uint32_t i = 0; i < side[p].n; ++i) {
                const uint4 r = hrec[p][i];
                const uint32_t g = list[p][i] / 2;
                const int status = (int)(r.y & 0xFFu);
                mv[g].push_back((uint16_t)(r.x & 0xFFFFu));
                G[g].n_moves += 1;
                G[g].status = (uint8_t)status;
                if (status == SPAI_WON) G[g].result_a = p == 0 ? 1 : -1;   // the mover wins
                else if (status == SPAI_ONGOING && cfg->max_plies && G[g].n_moves >= cfg->max_plies)
                    G[g].adjudicated = 1;
            }
        for (uint32_t g : live)
            if (G[g].status == SPAI_ONGOING && !G[g].adjudicated) next.push_back(g);
        live.swap(next);
    }
    if (games)
        for (uint32_t g = 0; g < n_games; ++g) games[g] = G[g];
    if (moves)
        for (uint32_t g = 0; g < n_games; ++g) {
            uint16_t *dst = moves + (size_t)g * cfg->moves_stride;
            const uint32_t n = std::min<uint32_t>(G[g].n_moves, cfg->moves_stride);
            for (uint32_t k = 0; k < cfg->moves_stride; ++k) dst[k] = k < n ? mv[g][k] : 0;
        }
    if (stats) {
        *stats = spai_chess_match_stats{};
        for (const spai_chess_match_game &g : G) {
            const int f = g.a_moves_first ? 0 : 1;
            (g.result_a > 0 ? stats->a_wins : g.result_a < 0 ? stats->b_wins : stats->draws)[f] += 1;
            stats->adjudicated += g.adjudicated;
            stats->plies += g.n_moves;
        }
        for (int p = 0; p < 2; ++p) {
            stats->sims[p] = sims[p];
            stats->evals[p] = evals[p];
        }
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
    return SPAI_OK;
}

}  // namespace chess
}  // namespace spai
