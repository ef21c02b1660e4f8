// selfplay.hip — SelfPlayWorker::self_play (learner_concurrent.rs:169-242) on the
// device-resident Connect4 search (search.hip): the move step k_advance and the
// run loop behind spai_selfplay_run / spai_selfplay_stream.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "philox.h"
#include "search_internal.h"

namespace spai {
namespace {
// Self-play's move after a search call (learner_concurrent.rs:177-203), per active
// tree: the root's visit counts, the sampled child (the Philox uniform of philox.h
// and rand's WeightedIndex<f32> over (visits as f32).powf(T), the weights from a
// table of the host's powf, so the pick is the host sampler's bit for bit), and for
// a game that goes on the child written as the tree's new root (use_subtree).  What
// goes back to the host, in one copy: search_internal.h "move step".
__global__ void k_advance(TreeView T, RootsOut R, const uint32_t *__restrict__ active, uint32_t n_active,
                          const float *__restrict__ pow_tab, uint32_t pow_n, uint64_t seed,
                          const uint64_t *__restrict__ slot_gid, uint32_t *__restrict__ slot_move,
                          const uint32_t *err, const uint32_t *cache_fill, ChainCounts cc, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    move_header(err, cache_fill, cc, n_active, out);
    if (i >= n_active) return;
    const uint32_t t = active[i];
    uint32_t *rec = out + 2 + (size_t)i * kMoveRec;
    uint32_t vis[c4::kActions];
    const uint32_t rw = move_load_root(T, t, rec, vis);
    const uint32_t nch = rw == kNoChildren ? 0 : rw >> 24;
    bool beyond = false;
    int idx = -1;   // weighted_index_with: -1 without children
    if (nch > 0) {   // WeightedIndex<f32> over (visits as f32).powf(T) (learner_concurrent.rs:189-193)
        float w[c4::kActions];
        for (uint32_t k = 0; k < nch; ++k) {
            beyond |= vis[k] >= pow_n;
            w[k] = pow_tab[min(vis[k], pow_n - 1)];
        }
        idx = weighted_index_f32(w, (int)nch, sample_u01_f32(seed, slot_gid[t], slot_move[t]));
    }
    if (beyond || idx < 0) {
        rec[kRecPick] = kPickNone | (beyond ? kPickNoTable : (uint32_t)(-idx));
        return;
    }
    c4::State cs;
    (void)move_apply(T, R, t, rw, idx, rec, cs);
    slot_move[t] += 1;   // the game's next move number (its sampling counter)
}
// self-play: tree slot list[i] starts game list[n + i] (refill) or game gid_base +
// slot (list == null, every slot in [0, n)): an empty board as its root, an empty
// arena, move number 0
__global__ void k_slots_start(TreeView T, RootsOut R, uint64_t *__restrict__ slot_gid,
                              uint32_t *__restrict__ slot_move, const uint32_t *__restrict__ list, uint32_t n,
                              uint64_t gid_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = list ? list[i] : i;
    tree_clear(T, R, t);
    root_position(R, t, c4::State{0, 0, 0, c4::kOngoing});
    slot_gid[t] = gid_base + (list ? list[n + i] : i);
    slot_move[t] = 0;
}
}  // namespace

// the device buffer of a move step's records and its two pinned host copies (move
// m's is read while m + 1 runs), at least n_words each
int move_buffers(spai_engine *e, size_t n_words) {
    if (e->h_move_n >= n_words) return SPAI_OK;
    e->h_move_n = 0;
    for (uint32_t *&h : e->h_move) {
        if (h) (void)hipHostFree(h);
        h = nullptr;
        void *ph = nullptr;
        SPAI_HIP(hipHostMalloc(&ph, n_words * 4, hipHostMallocDefault));
        h = (uint32_t *)ph;
    }
    SPAI_TRY(e->move_out.alloc(n_words));
    e->h_move_n = n_words;
    return SPAI_OK;
}
// SelfPlayWorker::self_play (learner_concurrent.rs:169-242).  Per move: the search
// call, then k_advance samples every game's move on the device and moves its
// root, and one pinned copy brings back the records.  The next move's search is
// launched as soon as the host knows which games go on; this move's bookkeeping
// (policy targets, histories, finished games to the sink, in the reference's
// order) runs on the host while it searches.
// window < n_games (spai_selfplay_stream): the games run through `window` tree
// slots; a slot whose game ended takes the next game before the next search call.
// Each game's draws are keyed by its id and its own move number (per slot on the
// device), so every game is the one spai_selfplay_run would play.
int selfplay_run(spai_engine *e, uint32_t n_games, uint64_t gid_base, spai_sample_sink sink, void *user,
                 spai_selfplay_stats *stats, uint32_t window) {
    const auto t_start = std::chrono::steady_clock::now();
    const uint32_t W = (window == 0 || window >= n_games) ? n_games : window;   // tree slots
    SPAI_TRY(trees_create(e, W));
    SPAI_CHECK(e->cfg.eval != SPAI_EVAL_NET || e->net, SPAI_ERR_INVALID,
               "eval = NET but no net set (spai_engine_set_net)");
    Trees &T = e->trees;
    hipStream_t st = e->stream;
    const uint32_t ns = e->cfg.num_searches;
    // every game's history in flat per-game slabs of the longest game (42 plies):
    // growing 3 x n_games vectors made every game reallocate at the same moves
    constexpr size_t kPlies = c4::kCells;
    // (visits as f32).powf(T) for every count a root child can reach (a search call
    // adds at most ns visits to a root, a game has at most kPlies moves), by the
    // host's powf (the f32::powf of the reference), once per temperature
    const uint32_t pow_n = ns * (uint32_t)kPlies + 1;
    const float temp = e->cfg.temperature;
    if (e->pow_tab_t != temp || e->pow_tab.n < pow_n) {
        std::vector<float> tab(pow_n);
        for (uint32_t k = 0; k < pow_n; ++k) tab[k] = ::powf((float)k, temp);   // Rust f32::powf = libm powf
        e->pow_tab_t = -1.0f;
        SPAI_TRY(e->pow_tab.alloc(pow_n));
        SPAI_HIP(hipMemcpy(e->pow_tab.p, tab.data(), pow_n * sizeof(float), hipMemcpyHostToDevice));
        e->pow_tab_t = temp;
    }
    // records, then every chain's leaf counters (tail mode: up to ns + kTailChunk + 1)
    SPAI_TRY(move_buffers(e, 2 + (size_t)W * kMoveRec +
                                 (size_t)spai_engine::kChains * (std::max(ns, 1u) + kTailChunk + 1)));
    std::vector<c4::State> h_states((size_t)W * kPlies);   // per tree slot
    std::vector<float> h_pol((size_t)W * kPlies * 7);
    std::vector<int32_t> h_moves((size_t)W * kPlies);
    std::vector<uint32_t> h_len(W, 0);
    std::vector<uint32_t> act[2];   // this move's trees and the next move's (the launch reads them)
    act[0].resize(W);
    for (uint32_t i = 0; i < W; ++i) act[0][i] = i;
    std::vector<uint32_t> slot_game(W);   // the game (index < n_games) each slot plays
    for (uint32_t i = 0; i < W; ++i) slot_game[i] = i;
    uint32_t next_game = W;
    std::vector<uint32_t> refill[2];   // per move parity: [slots..., games...] uploaded for k_slots_start
    std::vector<float> enc, sv;
    double sims = 0, evals = 0, games = 0, positions = 0, moves = 0;
    // optional per-move trace (diagnostics): SPAI_TRACE_MOVES=<csv path>
    FILE *trace = nullptr;
    if (const char *tp = std::getenv("SPAI_TRACE_MOVES")) trace = std::fopen(tp, "a");
    struct TraceClose {
        FILE *f;
        ~TraceClose() {
            if (f) std::fclose(f);
        }
    } trace_close{trace};
    const TreeView tv = tree_view(e);
    const RootsOut ro = roots_out(e);
    SearchRun R;
    // root noise (spai_set_root_noise): every search is keyed by the move draw's own keys, the
    // slot's game id and that game's move number, which k_slots_start and k_advance keep per
    // tree slot on the device; so a game does not depend on the window or on gid_base's split
    RootNoise noise{};
    bool noisy = false;
    SPAI_TRY(root_noise_prepare(e, noise, noisy));
    // every slot starts its first game (id gid_base + slot) at move 0
    k_slots_start<<<(W + 255) / 256, 256, 0, st>>>(tv, ro, T.slot_gid.p, T.slot_move.p, nullptr, W, gid_base);
    SPAI_HIP(hipGetLastError());
    // enqueue a move over the trees a: slots in rf start their new games, the search
    // call, k_advance, the records' copy to dst
    auto launch = [&](const std::vector<uint32_t> &a, const std::vector<uint32_t> &rf, uint32_t *dst) -> int {
        const uint32_t na = (uint32_t)a.size();
        if (!rf.empty()) {
            const uint32_t nr = (uint32_t)(rf.size() / 2);
            SPAI_HIP(hipMemcpyAsync(T.refill.p, rf.data(), rf.size() * 4, hipMemcpyHostToDevice, st));
            k_slots_start<<<(nr + 255) / 256, 256, 0, st>>>(tv, ro, T.slot_gid.p, T.slot_move.p, T.refill.p, nr,
                                                           gid_base);
        }
        SPAI_TRY(search_launch(e, na, a.data(), ns, R, noisy ? &noise : nullptr));
        ChainCounts cc{{}, {}, R.n_counts};
        for (int h = 0; h < R.nchain; ++h) {
            cc.p[h] = e->batch[h].iter_counts.p;
            cc.n[h] = R.n_counts;
        }
        k_advance<<<(na + 63) / 64, 64, 0, st>>>(tv, ro, e->active.p, na, e->pow_tab.p, (uint32_t)e->pow_tab.n,
                                                 e->cfg.seed, T.slot_gid.p, T.slot_move.p, e->err.p,
                                                 e->cache.buckets ? e->cache.ctr.p : nullptr, cc, e->move_out.p);
        SPAI_HIP(hipGetLastError());
        const size_t words = 2 + (size_t)na * kMoveRec + (size_t)R.nchain * R.n_counts;
        SPAI_HIP(hipMemcpyAsync(dst, e->move_out.p, words * 4, hipMemcpyDeviceToHost, st));
        return SPAI_OK;
    };
    // every return below, errors included, leaves the engine quiescent (the moves in
    // flight write device roots and a pinned buffer)
    const Quiesce quiesce{e, 0u};
    uint64_t move_no = 0;
    int cur = 0;
    auto tm0 = std::chrono::steady_clock::now();
    SPAI_TRY(launch(act[0], refill[0], e->h_move[0]));
    while (!act[cur].empty()) {
        const std::vector<uint32_t> &A = act[cur];
        const uint32_t na = (uint32_t)A.size();
        const uint32_t *mo = e->h_move[move_no & 1];
        SPAI_HIP(hipStreamSynchronize(st));
        const auto tm1 = std::chrono::steady_clock::now();
        const uint32_t passes = e->last_tail_passes;
        uint32_t max_ev = 0;
        double served = 0;   // live leaves of the call over its trees (hits of the evaluation cache included)
        bool stop = false;   // a game without a move: its error is raised in the bookkeeping below
        for (uint32_t i = 0; i < na; ++i) {
            const uint32_t *rec = move_rec(mo, i);
            max_ev = std::max(max_ev, rec[kRecEvals]);
            served += rec[kRecEvals];
            stop |= (rec[kRecPick] & kPickNone) != 0;
        }
        SPAI_TRY(search_finish(e, R, ns, move_rec(mo, na), mo[0], max_ev, served, mo[1]));
        const double fwd_leaves = e->last_evals_per_iter * ns;
        sims += (double)na * ns;
        evals += served;
        moves += 1;
        // the games that go on, in order (trees_vec.remove keeps it), and their next move;
        // streaming: slots whose game ended take the next games (appended)
        std::vector<uint32_t> &N = act[cur ^ 1];
        std::vector<uint32_t> &RF = refill[(move_no + 1) & 1];
        N.clear();
        RF.clear();
        auto tm2 = tm1;
        if (!stop) {
            for (uint32_t i = 0; i < na; ++i)
                if (pick_status(move_rec(mo, i)[kRecPick]) == c4::kOngoing) N.push_back(A[i]);
            for (uint32_t i = 0; i < na && next_game < n_games; ++i)
                if (pick_status(move_rec(mo, i)[kRecPick]) != c4::kOngoing) {
                    RF.push_back(A[i]);
                    RF.push_back(next_game++);
                }
            const size_t nr = RF.size() / 2;
            if (nr) {   // [slots..., games...]
                std::vector<uint32_t> tmp(RF);
                for (size_t j = 0; j < nr; ++j) {
                    RF[j] = tmp[2 * j];
                    RF[nr + j] = tmp[2 * j + 1];
                    N.push_back(RF[j]);
                }
            }
            tm2 = std::chrono::steady_clock::now();
            if (!N.empty()) SPAI_TRY(launch(N, RF, e->h_move[(move_no + 1) & 1]));
        }
        const auto tm3 = std::chrono::steady_clock::now();
        for (int k = (int)na - 1; k >= 0; --k) {   // for i in (0..trees_vec.len()).rev()
            const uint32_t t = A[k];
            const uint32_t *rec = move_rec(mo, k);
            const uint32_t w = rec[kRecRoot], pick = rec[kRecPick];
            if (pick & kPickNone) {
                SPAI_CHECK(pick_index(pick) != (int)kPickNoTable, SPAI_ERR_INVALID,
                           "internal: game %u has a visit count beyond the visits^T table", t);
                SPAI_CHECK(false, SPAI_ERR_NAN, "WeightedIndex over all-zero visit counts (game %u)", t);
            }
            const uint32_t nch = root_children(w), first = w & 0xFFFFFFu;
            T.h_root_first[t] = first;
            T.h_root_nch[t] = (uint8_t)nch;
            const c4::State rs = T.h_root_state[t];
            const uint32_t legal = c4::legal_mask(rs.x, rs.o, rs.status);
            float pol[c4::kActions] = {0, 0, 0, 0, 0, 0, 0};   // root visit policy (mcts.rs:310-331)
            for (uint32_t j = 0; j < nch; ++j) pol[c4::kth_bit(legal, (int)j)] = (float)rec[kRecVisits + j];
            const int idx = pick_index(pick), a = pick_action(pick);
            c4::State cs;
            SPAI_CHECK(move_replays(rec, rs, cs), SPAI_ERR_INVALID, "internal: game %u's device move does not replay",
                       t);
            const size_t m = ++h_len[t];   // plies so far, this one included
            SPAI_CHECK(m <= kPlies, SPAI_ERR_INVALID, "internal: game %u longer than %zu plies", t, kPlies);
            c4::State *hs = h_states.data() + (size_t)t * kPlies;
            float *hp = h_pol.data() + (size_t)t * kPlies * 7;
            int32_t *hm = h_moves.data() + (size_t)t * kPlies;
            hs[m - 1] = rs;
            normalize_policy(pol, hp + (m - 1) * 7);
            hm[m - 1] = a;
            if (cs.status != c4::kOngoing) {                  // is_terminal: emit, trees_vec.remove(i)
                const float v = c4::terminal_value(cs.status);
                enc.assign(sink ? m * 126 : 0, 0.f);
                sv.resize(m);
                for (size_t j = 0; j < (sink ? m : 0); ++j) {
                    const c4::State &s = hs[j];
                    const bool xm = c4::x_to_move(s.n);
                    const uint64_t mine = xm ? s.x : s.o, theirs = xm ? s.o : s.x;
                    for (int r = 0; r < 6; ++r)
                        for (int cc = 0; cc < 7; ++cc) {
                            const int b = cc * 7 + r, cell = r * 7 + cc;
                            if ((mine >> b) & 1) enc[j * 126 + cell] = 1.f;
                            else if ((theirs >> b) & 1) enc[j * 126 + 42 + cell] = 1.f;
                            else enc[j * 126 + 84 + cell] = 1.f;
                        }
                    // x.get_current_player() == state.get_current_player() ? value : -value
                    sv[j] = ((s.n & 1) == (cs.n & 1)) ? v : -v;
                }
                if (sink) sink(user, (uint32_t)(gid_base + slot_game[t]), (uint32_t)m, enc.data(), hp, sv.data(), hm);
                games += 1;
                positions += (double)m;
                h_len[t] = 0;
            } else {                                          // use_subtree(selected_id), already on the device
                T.h_root[t] = first + (uint32_t)idx;
                T.h_root_state[t] = cs;
                T.h_root_nch[t] = 0;
            }
        }
        {   // streaming: the refilled slots' host mirrors start their new games (k_slots_start
            // reset the device side ahead of the search call already in flight)
            const std::vector<uint32_t> &RFc = refill[(move_no + 1) & 1];
            const size_t nr = RFc.size() / 2;
            for (size_t j = 0; j < nr; ++j) {
                const uint32_t t = RFc[j];
                slot_game[t] = RFc[nr + j];
                T.h_root[t] = 0;
                T.h_root_state[t] = c4::State{0, 0, 0, c4::kOngoing};
                T.h_root_first[t] = 0;
                T.h_root_nch[t] = 0;
            }
        }
        if (trace)   // move, active trees, leaves evaluated, search seconds (launch to records), host seconds
                     // between the records and the next launch, search passes (tail mode; 0: one launch pair
                     // per iteration), bookkeeping seconds (overlapping the next search), leaves the forward
                     // ran (the rest of the evaluated ones came from the evaluation cache)
            std::fprintf(trace, "%llu,%u,%.0f,%.6f,%.6f,%u,%.6f,%.0f\n", (unsigned long long)move_no, na, served,
                         std::chrono::duration<double>(tm1 - tm0).count(),
                         std::chrono::duration<double>(tm2 - tm1).count(), passes,
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - tm3).count(), fwd_leaves);
        tm0 = tm2;
        cur ^= 1;
        ++move_no;
    }
    if (stats) {
        stats->sims = sims;
        stats->evals = evals;
        stats->games = games;
        stats->positions = positions;
        stats->moves = moves;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    }
    return SPAI_OK;
}

}  // namespace spai
