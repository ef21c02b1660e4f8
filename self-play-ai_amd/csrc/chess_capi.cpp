// chess_capi.cpp — extern "C" entry points of the chess section of include/spai.h.
#include <cstring>
#include <new>

#include "chess_engine.h"

using namespace spai;
using namespace spai::chess;

#define CH_CHECK(e)                                                       \
    do {                                                                  \
        SPAI_CHECK(e, SPAI_ERR_INVALID, "null chess engine handle");      \
        SPAI_SET_DEVICE(e);                                               \
    } while (0)


namespace {
void release_all(spai_chess *e) {
    spai::chess::Slots &S = e->slots;
    S.board.release();
    S.hist.release();
    S.n_hist.release();
    S.moves.release();
    S.u32.release();
    S.i32.release();
    S.f32.release();
    S.f32b.release();
    spai::chess::Trees &T = e->trees;
    T.nodes.release();
    T.first.release();
    T.nhash.release();
    T.root.release();
    T.fill.release();
    T.half.release();
    T.root_board.release();
    T.root_reps.release();
    T.hist.release();
    T.hist_n.release();
    T.path.release();
    T.depth.release();
    T.leaf_moves.release();
    T.leaf_n.release();
    T.leaf_hash.release();
    T.leaf_key.release();
    T.st_nch.release();
    T.st_visits.release();
    T.st_ids.release();
    T.st_moves.release();
    T.adv_pick.release();
    T.adv_out.release();
    T.adv_board.release();
    spai::chess::Batch &B = e->batch;
    B.counts.release();
    B.tree.release();
    B.x.release();
    B.xf.release();
    B.logits.release();
    B.value.release();
    e->active.release();
    e->noise_gid.release();
    e->noise_move.release();
    e->noise_done.release();
    e->err.release();
    match_release(e);
    for (hipEvent_t ev : e->timer.ev) (void)hipEventDestroy(ev);
    e->timer.ev.clear();
}
}  // namespace

extern "C" {

int spai_chess_config_default(spai_config *cfg) {
    SPAI_PTR(cfg);
    *cfg = spai_config{};
    cfg->c = 2.0f;              // mcts.rs:49
    cfg->num_searches = 400;    // BASELINE config 4 (chess, 400 sims/move)
    cfg->temperature = 1.25f;   // learner_concurrent.rs:53
    cfg->max_trees = 1024;      // BASELINE config 4 (1024 parallel games)
    // longest game: transposition-table entries per game.  The reference's rules end a
    // game by the fifty-move counter (chess.rs:124-144,154-166: a draw at 100 plies with
    // no pawn move, capture or castle-right change).  Pawn moves and captures alone bound
    // a game at 5,949 moves = 11,898 plies; the reference's extra reset on a castle-rights
    // change can happen at most 4 more times (each side loses its kingside and queenside
    // rights separately), each worth at most 100 further plies: 12,298 plies.  12,304
    // entries (96 KB per game) therefore cover the longest legal game; a longer one would
    // be reported as SPAI_ERR_CAPACITY ("game longer than cfg.max_moves").
    cfg->max_moves = 12304;
    cfg->eval = SPAI_EVAL_NET;
    cfg->seed = 0;
    return SPAI_OK;
}

int spai_chess_create(const spai_config *cfg, int device, spai_chess **out) {
    SPAI_PTR(cfg);
    SPAI_PTR(out);
    SPAI_CHECK(cfg->eval <= SPAI_EVAL_HASH, SPAI_ERR_INVALID, "bad eval kind %u", cfg->eval);
    SPAI_CHECK(cfg->max_moves >= 1 && cfg->max_trees >= 1 && cfg->num_searches >= 1, SPAI_ERR_INVALID,
               "max_moves, max_trees and num_searches must be >= 1");
    SPAI_CHECK(cfg->max_moves <= 65535, SPAI_ERR_INVALID, "max_moves %u > 65535", cfg->max_moves);
    int ndev = 0;
    SPAI_HIP(hipGetDeviceCount(&ndev));
    SPAI_CHECK(device >= 0 && device < ndev, SPAI_ERR_DEVICE, "device %d not present (%d visible)", device, ndev);
    SPAI_HIP(hipSetDevice(device));
    spai_chess *e = new (std::nothrow) spai_chess();
    SPAI_CHECK(e, SPAI_ERR_INVALID, "out of host memory");
    e->device = device;
    e->cfg = *cfg;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) e->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess || e->err.alloc(1) != SPAI_OK ||
        hipMemsetAsync(e->err.p, 0, 4, e->stream) != hipSuccess) {
        set_error("chess engine stream / scratch allocation failed");
        delete e;
        return SPAI_ERR_DEVICE;
    }
    *out = e;
    return SPAI_OK;
}

int spai_chess_destroy(spai_chess *e) {
    if (!e) return SPAI_OK;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    release_all(e);
    (void)hipStreamDestroy(e->stream);
    delete e;
    return SPAI_OK;
}

int spai_chess_sync(spai_chess *e) {
    CH_CHECK(e);
    SPAI_HIP(hipStreamSynchronize(e->stream));
    return SPAI_OK;
}

int spai_chess_games_resize(spai_chess *e, uint32_t n) {
    CH_CHECK(e);
    return slots_resize(e, n, e->cfg.max_moves);
}

int spai_chess_games_write(spai_chess *e, uint32_t first, uint32_t n, const spai_chess_state *s) {
    CH_CHECK(e);
    if (n) SPAI_PTR(s);
    return slots_write(e, first, n, s);
}

int spai_chess_games_read(spai_chess *e, uint32_t first, uint32_t n, spai_chess_state *s) {
    CH_CHECK(e);
    if (n) SPAI_PTR(s);
    return slots_read(e, first, n, s);
}

int spai_chess_legal_moves(spai_chess *e, uint32_t first, uint32_t n, uint16_t *moves, uint32_t *counts) {
    CH_CHECK(e);
    return slots_legal(e, first, n, moves, counts);
}

int spai_chess_apply(spai_chess *e, uint32_t first, uint32_t n, const uint16_t *moves, int32_t *rc) {
    CH_CHECK(e);
    if (n) SPAI_PTR(moves);
    return slots_apply(e, first, n, moves, rc);
}

int spai_chess_status(spai_chess *e, uint32_t first, uint32_t n, uint8_t *status, uint32_t *reps, float *value,
                      uint8_t *terminated) {
    CH_CHECK(e);
    return slots_status(e, first, n, status, reps, value, terminated);
}

int spai_chess_rules_bench(spai_chess *e, uint32_t first, uint32_t n, uint32_t iters, double *ms) {
    CH_CHECK(e);
    SPAI_PTR(ms);
    return slots_rules_bench(e, first, n, iters, ms);
}

int spai_chess_perft(spai_chess *e, uint32_t slot, int depth, uint64_t *counts) {
    CH_CHECK(e);
    SPAI_PTR(counts);
    return perft(e, slot, depth, counts);
}

int spai_chess_encode(spai_chess *e, uint32_t first, uint32_t n, float *out) {
    CH_CHECK(e);
    if (n) SPAI_PTR(out);
    return slots_encode(e, first, n, out);
}

int spai_chess_mask_invalid(spai_chess *e, uint32_t first, uint32_t n, const float *policy, uint32_t len,
                            float *out) {
    CH_CHECK(e);
    if (n) {
        SPAI_PTR(policy);
        SPAI_PTR(out);
    }
    return slots_mask(e, first, n, policy, len, out);
}

int spai_chess_move_index(int side, uint16_t move, int32_t *index) {
    SPAI_PTR(index);
    SPAI_CHECK(side == 0 || side == 1, SPAI_ERR_INVALID, "side must be 0 or 1");
    SPAI_CHECK(((move >> 12) & 7) <= 4 && (move & 63) != ((move >> 6) & 63), SPAI_ERR_INVALID, "bad move code %u",
               move);
    *index = policy_index(side, move);
    return SPAI_OK;
}

int spai_chess_index_move(int side, int32_t index, uint16_t *move) {
    SPAI_PTR(move);
    SPAI_CHECK(side == 0 || side == 1, SPAI_ERR_INVALID, "side must be 0 or 1");
    SPAI_CHECK(index >= 0 && index < kPolicy, SPAI_ERR_INVALID, "index %d out of [0, 4672)", index);
    *move = (uint16_t)get_action_host(side, index);
    return SPAI_OK;
}

int spai_chess_net_num_params(int blocks, size_t *count) {
    SPAI_PTR(count);
    SPAI_CHECK(blocks >= 0, SPAI_ERR_INVALID, "blocks < 0");
    *count = net_num_params(blocks);
    return SPAI_OK;
}

int spai_chess_net_init_params(int blocks, uint64_t seed, float *params) {
    SPAI_PTR(params);
    SPAI_CHECK(blocks >= 0, SPAI_ERR_INVALID, "blocks < 0");
    net_init_params(blocks, seed, params);
    return SPAI_OK;
}

int spai_chess_net_create(spai_chess *e, int blocks, const float *params, size_t n_params, spai_chess_net **out) {
    return spai_chess_net_create_dtype(e, blocks, params, n_params, SPAI_DTYPE_BF16, out);
}

int spai_chess_net_create_dtype(spai_chess *e, int blocks, const float *params, size_t n_params, int dtype,
                                spai_chess_net **out) {
    CH_CHECK(e);
    SPAI_PTR(out);
    return net_create(e, blocks, params, n_params, dtype, out);
}

int spai_chess_net_dtype(spai_chess_net *net, int *dtype) {
    SPAI_PTR(net);
    SPAI_PTR(dtype);
    *dtype = net->dtype;
    return SPAI_OK;
}

int spai_chess_net_image(spai_chess_net *net, void *out, size_t cap, size_t *bytes) {
    SPAI_PTR(net);
    SPAI_PTR(bytes);
    CH_CHECK(net->eng);
    return net_image(net, out, cap, bytes);
}

int spai_chess_net_destroy(spai_chess_net *net) {
    if (!net) return SPAI_OK;
    (void)hipSetDevice(net->eng->device);
    if (net->eng->net == net) net->eng->net = nullptr;
    net_destroy(net);
    return SPAI_OK;
}

int spai_chess_net_forward(spai_chess_net *net, uint32_t n, const float *x, float *logits, float *value) {
    SPAI_PTR(net);
    CH_CHECK(net->eng);
    if (n) {
        SPAI_PTR(x);
        SPAI_PTR(logits);
        SPAI_PTR(value);
    }
    return net_forward_host(net, n, x, logits, value);
}

int spai_chess_predict(spai_chess_net *net, uint32_t first, uint32_t n, float *priors, float *values) {
    SPAI_PTR(net);
    CH_CHECK(net->eng);
    if (n) {
        SPAI_PTR(priors);
        SPAI_PTR(values);
    }
    return net_predict(net, first, n, priors, values);
}

int spai_chess_set_net(spai_chess *e, spai_chess_net *net) {
    CH_CHECK(e);
    SPAI_CHECK(!net || net->eng == e, SPAI_ERR_INVALID, "net belongs to another engine");
    e->net = net;
    return SPAI_OK;
}

int spai_chess_trees_create(spai_chess *e, uint32_t n) {
    CH_CHECK(e);
    return trees_create(e, n);
}

int spai_chess_search(spai_chess *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
                      uint32_t *child_ids, float *child_visits, uint16_t *child_moves, uint32_t *n_children) {
    CH_CHECK(e);
    SPAI_PTR(tree_idx);
    return search(e, n, tree_idx, num_searches, policy, child_ids, child_visits, child_moves, n_children, nullptr);
}

int spai_chess_set_root_noise(spai_chess *e, float alpha, float epsilon) {
    CH_CHECK(e);
    SPAI_CHECK(alpha >= 0.01f && alpha <= 100.0f, SPAI_ERR_INVALID, "root noise: alpha %g not in [0.01, 100]",
               (double)alpha);
    SPAI_CHECK(epsilon >= 0.0f && epsilon <= 1.0f, SPAI_ERR_INVALID, "root noise: epsilon %g not in [0, 1]",
               (double)epsilon);
    e->noise_alpha = alpha;
    e->noise_eps = epsilon;
    return SPAI_OK;
}

int spai_chess_get_root_noise(spai_chess *e, float *alpha, float *epsilon) {
    CH_CHECK(e);
    if (alpha) *alpha = e->noise_alpha;
    if (epsilon) *epsilon = e->noise_eps;
    return SPAI_OK;
}

int spai_chess_root_noise(spai_chess *e, uint32_t count, const uint64_t *game_id, const uint32_t *move_no,
                          const uint32_t *n_children, float alpha, float *eta) {
    CH_CHECK(e);
    SPAI_CHECK(alpha >= 0.01f && alpha <= 100.0f, SPAI_ERR_INVALID, "root noise: alpha %g not in [0.01, 100]",
               (double)alpha);
    if (count) {
        SPAI_PTR(game_id);
        SPAI_PTR(move_no);
        SPAI_PTR(n_children);
        SPAI_PTR(eta);
    }
    return root_noise_draws(e, count, game_id, move_no, n_children, alpha, eta);
}

int spai_chess_search_keyed(spai_chess *e, uint32_t n, const uint32_t *tree_idx, const uint64_t *game_id,
                            const uint32_t *move_no, uint32_t num_searches, float *policy, uint32_t *child_ids,
                            float *child_visits, uint16_t *child_moves, uint32_t *n_children) {
    CH_CHECK(e);
    SPAI_PTR(tree_idx);
    SPAI_PTR(game_id);
    SPAI_PTR(move_no);
    return search(e, n, tree_idx, num_searches, policy, child_ids, child_visits, child_moves, n_children, nullptr,
                  game_id, move_no);
}

int spai_chess_tree_reset(spai_chess *e, uint32_t tree, uint32_t slot) {
    CH_CHECK(e);
    return tree_reset_from_slot(e, tree, slot);
}

int spai_chess_tree_use_subtree(spai_chess *e, uint32_t tree, uint32_t child_index) {
    CH_CHECK(e);
    return tree_use_subtree(e, tree, child_index);
}

int spai_chess_tree_root(spai_chess *e, uint32_t tree, spai_chess_state *root, uint32_t *visits, float *value_sum) {
    CH_CHECK(e);
    return tree_root(e, tree, root, visits, value_sum);
}

int spai_chess_trees_advance(spai_chess *e, uint32_t n, const uint32_t *tree_idx, const uint32_t *child_index,
                             uint8_t *status, uint32_t *reps) {
    CH_CHECK(e);
    SPAI_PTR(tree_idx);
    SPAI_PTR(child_index);
    return trees_advance(e, n, tree_idx, child_index, status, reps);
}

int spai_chess_selfplay_run(spai_chess *e, uint32_t n_games, uint64_t game_id_base, spai_chess_sample_sink sink,
                            void *user, spai_selfplay_stats *stats) {
    CH_CHECK(e);
    return selfplay_run(e, n_games, game_id_base, sink, user, stats);
}

int spai_chess_selfplay_stream(spai_chess *e, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                               spai_chess_sample_sink sink, void *user, spai_selfplay_stats *stats) {
    CH_CHECK(e);
    if (window == 0) {
        set_error("window must be > 0");
        return SPAI_ERR_INVALID;
    }
    return selfplay_run(e, n_games, game_id_base, sink, user, stats, window);
}

int spai_chess_selfplay_compact(spai_chess *e, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                                spai_chess_compact_sink sink, void *user, spai_selfplay_stats *stats) {
    CH_CHECK(e);
    return selfplay_run(e, n_games, game_id_base, nullptr, user, stats, window, sink);
}

int spai_chess_tree_children(spai_chess *e, uint32_t tree, uint16_t *moves, uint32_t *visits, uint32_t *n) {
    CH_CHECK(e);
    return tree_children(e, tree, moves, visits, n);
}

int spai_chess_tree_child_stats(spai_chess *e, uint32_t tree, uint16_t *moves, uint32_t *visits, float *value_sums,
                                float *priors, uint32_t *n) {
    CH_CHECK(e);
    return tree_child_stats(e, tree, moves, visits, value_sums, priors, n);
}

int spai_chess_match_set_one_stream(spai_chess *e, int on) {
    CH_CHECK(e);
    return match_set_one_stream(e, on);
}

int spai_chess_match_config_default(spai_chess_match_config *cfg) {
    SPAI_PTR(cfg);
    *cfg = spai_chess_match_config{};
    cfg->struct_size = (uint32_t)sizeof(spai_chess_match_config);
    cfg->opening_plies = 2;
    cfg->max_plies = 512;
    return SPAI_OK;
}

int spai_chess_match_run(spai_chess *e, const spai_chess_match_player *a, const spai_chess_match_player *b,
                         uint32_t n_games, uint64_t gid_base, const spai_chess_match_config *cfg,
                         spai_chess_match_game *games, uint16_t *moves, spai_chess_match_stats *stats) {
    CH_CHECK(e);
    SPAI_PTR(a);
    SPAI_PTR(b);
    SPAI_PTR(cfg);
    SPAI_CHECK(cfg->struct_size == sizeof(spai_chess_match_config), SPAI_ERR_INVALID,
               "spai_chess_match_config.struct_size %u, expected %zu", cfg->struct_size,
               sizeof(spai_chess_match_config));
    SPAI_CHECK(cfg->opening_plies <= 3, SPAI_ERR_INVALID, "opening_plies %u > 3", cfg->opening_plies);
    SPAI_CHECK(!cfg->start || cfg->opening_plies == 0, SPAI_ERR_INVALID,
               "start positions take no opening (opening_plies %u)", cfg->opening_plies);
    SPAI_CHECK(!moves || cfg->moves_stride > 0, SPAI_ERR_INVALID, "moves given with moves_stride 0");
    SPAI_CHECK(n_games > 0 && 2 * (uint64_t)n_games <= e->cfg.max_trees, SPAI_ERR_INVALID,
               "a match of %u games needs %llu trees, max_trees=%u", n_games, 2ull * n_games, e->cfg.max_trees);
    for (const spai_chess_match_player *p : {a, b}) {
        SPAI_CHECK(p->eval >= SPAI_EVAL_NET && p->eval <= SPAI_EVAL_HASH, SPAI_ERR_INVALID, "bad eval kind %d", p->eval);
        SPAI_CHECK(p->eval != SPAI_EVAL_NET || p->net, SPAI_ERR_INVALID, "player with eval = NET but no net");
        SPAI_CHECK(p->eval != SPAI_EVAL_NET || p->net->eng == e, SPAI_ERR_INVALID, "net belongs to another engine");
        SPAI_CHECK(p->num_searches >= 1 && p->num_searches <= e->cfg.num_searches, SPAI_ERR_INVALID,
                   "player num_searches %u not in [1, cfg.num_searches=%u]", p->num_searches, e->cfg.num_searches);
    }
    return match_run(e, a, b, n_games, gid_base, cfg, games, moves, stats);
}

int spai_chess_set_timing(spai_chess *e, int enabled) {
    CH_CHECK(e);
    KernelTimer &t = e->timer;
    t.enabled = enabled != 0;
    for (int k = 0; k < 3; ++k) t.total_ms[k] = t.launches[k] = t.items[k] = 0;
    t.used = 0;
    t.which.clear();
    return SPAI_OK;
}

int spai_chess_timing(spai_chess *e, double *avg_ms, double *launches, double *items) {
    CH_CHECK(e);
    const KernelTimer &t = e->timer;
    for (int k = 0; k < 3; ++k) {
        if (avg_ms) avg_ms[k] = t.launches[k] > 0 ? t.total_ms[k] / t.launches[k] : 0.0;
        if (launches) launches[k] = t.launches[k];
        if (items) items[k] = t.items[k];
    }
    return SPAI_OK;
}

}  // extern "C"
