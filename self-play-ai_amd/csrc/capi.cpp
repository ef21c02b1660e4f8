// capi.cpp — extern "C" entry points of include/spai.h.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "philox.h"
#include "spai_internal.h"

namespace spai {
namespace {
thread_local char g_err[1024] = "";
}

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// net_init_params: tch 0.13 default initialisers (see DESIGN.md "Random init"),
// the same Philox stream as oracle/spai_oracle.c or_net_init_params.
namespace {
float philox_unit(uint64_t seed, uint32_t tensor, uint64_t idx) {
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t ctr[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), tensor, 0x5EEDu};
    uint32_t out[4];
    philox4x32(ctr, key, out);
    return (float)(out[0] >> 8) * (1.0f / 16777216.0f);
}
}  // namespace
}  // namespace spai

namespace spai {
void net_init_params(int game, int blocks, int hidden, uint64_t seed, float *params) {
    (void)game;
    uint32_t t = 0;
    float *p = params;
    auto uni = [&](size_t n, float lo, float hi) {
        for (size_t i = 0; i < n; ++i) p[i] = lo + (hi - lo) * philox_unit(seed, t, i);
        p += n;
        ++t;
    };
    auto cst = [&](size_t n, float v) {
        for (size_t i = 0; i < n; ++i) p[i] = v;
        p += n;
        ++t;
    };
    auto conv = [&](int ci, int co) {
        const float b = (float)std::sqrt(6.0 / (double)(ci * 9));
        uni((size_t)co * ci * 9, -b, b);
        cst(co, 0.f);
    };
    auto bn = [&](int c) {
        uni(c, 0.f, 1.f);
        cst(c, 0.f);
        cst(c, 0.f);
        cst(c, 1.f);
    };
    auto lin = [&](int in, int out) {
        const float b = (float)std::sqrt(6.0 / (double)in), bb = (float)(1.0 / std::sqrt((double)in));
        uni((size_t)out * in, -b, b);
        uni(out, -bb, bb);
    };
    conv(3, hidden);
    bn(hidden);
    for (int i = 0; i < blocks; ++i) {
        conv(hidden, hidden);
        bn(hidden);
        conv(hidden, hidden);
        bn(hidden);
    }
    conv(hidden, 32);
    bn(32);
    lin(32 * c4::kCells, c4::kActions);
    conv(hidden, 3);
    bn(3);
    lin(3 * c4::kCells, 1);
}
}  // namespace spai

using namespace spai;

#define ENG_CHECK(e)                                                 \
    do {                                                             \
        SPAI_CHECK(e, SPAI_ERR_INVALID, "null engine handle");       \
        SPAI_SET_DEVICE(e);                                          \
    } while (0)


extern "C" {

const char *spai_last_error(void) { return g_err; }

const char *spai_version(void) { return "spai 0.5 (gfx950)"; }

int spai_device_count(int *count) {
    SPAI_PTR(count);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = e == hipSuccess ? n : 0;
    return SPAI_OK;
}

int spai_config_default(int game, spai_config *cfg) {
    SPAI_PTR(cfg);
    SPAI_CHECK(game == SPAI_GAME_CONNECT4, SPAI_ERR_UNSUPPORTED, "device engine: only Connect4 is built (game %d)", game);
    *cfg = spai_config{};
    cfg->c = 2.0f;              // mcts.rs:49
    cfg->num_searches = 600;    // mcts.rs:50
    cfg->temperature = 1.25f;   // mcts.rs:51
    cfg->max_trees = 100;       // num_batched_self_play_games, learner_concurrent.rs:56
    cfg->max_moves = c4::kMaxPlies;
    cfg->eval = SPAI_EVAL_NET;
    cfg->seed = 0;
    return SPAI_OK;
}

int spai_engine_create(int game, const spai_config *cfg, int device, spai_engine **out) {
    SPAI_PTR(cfg);
    SPAI_PTR(out);
    SPAI_CHECK(game == SPAI_GAME_CONNECT4, SPAI_ERR_UNSUPPORTED, "device engine: only Connect4 is built (game %d)", game);
    SPAI_CHECK(cfg->eval <= SPAI_EVAL_HASH, SPAI_ERR_INVALID, "bad eval kind %u", cfg->eval);
    SPAI_CHECK(cfg->max_moves <= c4::kMaxPlies, SPAI_ERR_INVALID, "max_moves %u > 42", cfg->max_moves);
    int ndev = 0;
    SPAI_HIP(hipGetDeviceCount(&ndev));
    SPAI_CHECK(device >= 0 && device < ndev, SPAI_ERR_DEVICE, "device %d not present (%d visible)", device, ndev);
    SPAI_HIP(hipSetDevice(device));
    // SPAI_BLOCKING_SYNC=1 (A/B knob): host waits on the device sleep instead of spinning,
    // so a rank's self-play host loop needs less than a core beside its GPU (DESIGN.md §6:
    // the host-core budget of an 8-GPU node).  Takes effect only before the device's
    // first use in the process.
    static const bool blocking_sync = [] {
        const char *v = std::getenv("SPAI_BLOCKING_SYNC");
        return v && std::atoi(v) != 0;
    }();
    if (blocking_sync) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    spai_engine *e = new (std::nothrow) spai_engine();
    SPAI_CHECK(e, SPAI_ERR_INVALID, "out of host memory");
    e->game = game;
    e->device = device;
    e->cfg = *cfg;
    bool ok = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess && e->err.alloc(1) == SPAI_OK;
    for (int h = 1; h < spai_engine::kChains && ok; ++h)
        ok = hipStreamCreateWithFlags(&e->chain_stream[h], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&e->ev_join[h], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        set_error("engine stream / scratch allocation failed");
        delete e;
        return SPAI_ERR_DEVICE;
    }
    e->chain_stream[0] = e->stream;
    *out = e;
    return SPAI_OK;
}

int spai_engine_destroy(spai_engine *e) {
    if (!e) return SPAI_OK;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    Trees &T = e->trees;
    T.nodes.release();
    T.root.release();
    T.next_free.release();
    T.root_x.release();
    T.root_o.release();
    T.root_n.release();
    T.root_status.release();
    T.path.release();
    T.depth.release();
    T.slot.release();
    T.left.release();
    T.evals.release();
    for (Batch &B : e->batch) {
        B.tree.release();
        B.mine.release();
        B.theirs.release();
        B.priors.release();
        B.value.release();
        B.iter_counts.release();
        B.iter_more.release();
        B.iter_hits.release();
    }
    e->cache.table.release();
    e->cache.ctr.release();
    e->games.x.release();
    e->games.o.release();
    e->games.n.release();
    e->games.status.release();
    e->active.release();
    e->err.release();
    e->stats.release();
    e->pow_tab.release();
    e->move_out.release();
    e->noise_done.release();
    e->noise_gid.release();
    e->noise_move.release();
    for (uint32_t *&h : e->h_move)
        if (h) (void)hipHostFree(h);
    for (hipEvent_t ev : e->timer.ev) (void)hipEventDestroy(ev);
    for (int h = 1; h < spai_engine::kChains; ++h) {
        if (e->chain_stream[h]) (void)hipStreamSynchronize(e->chain_stream[h]);
        if (e->chain_stream[h]) (void)hipStreamDestroy(e->chain_stream[h]);
        if (e->ev_join[h]) (void)hipEventDestroy(e->ev_join[h]);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    (void)hipStreamDestroy(e->stream);
    delete e;
    return SPAI_OK;
}

int spai_engine_sync(spai_engine *e) {
    ENG_CHECK(e);
    SPAI_HIP(hipStreamSynchronize(e->stream));
    return SPAI_OK;
}

int spai_games_resize(spai_engine *e, uint32_t n) { ENG_CHECK(e); return rules_resize(e, n); }
int spai_games_reset(spai_engine *e, uint32_t first, uint32_t n) { ENG_CHECK(e); return rules_reset(e, first, n); }
int spai_games_write(spai_engine *e, uint32_t first, uint32_t n, const spai_c4_state *s) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(s);
    return rules_write(e, first, n, s);
}
int spai_games_read(spai_engine *e, uint32_t first, uint32_t n, spai_c4_state *s) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(s);
    return rules_read(e, first, n, s);
}
int spai_legal_mask(spai_engine *e, uint32_t first, uint32_t n, uint32_t *mask) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(mask);
    return rules_legal(e, first, n, mask);
}
int spai_apply(spai_engine *e, uint32_t first, uint32_t n, const int32_t *actions, int32_t *rc) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(actions);
    return rules_apply(e, first, n, actions, rc);
}
int spai_value_terminated(spai_engine *e, uint32_t first, uint32_t n, float *v, uint8_t *t) {
    ENG_CHECK(e);
    if (n) {
        SPAI_PTR(v);
        SPAI_PTR(t);
    }
    return rules_value_term(e, first, n, v, t);
}
int spai_encode(spai_engine *e, uint32_t first, uint32_t n, float *out) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(out);
    return rules_encode(e, first, n, out);
}
int spai_mask_invalid(spai_engine *e, uint32_t first, uint32_t n, const float *p, uint32_t len, float *out) {
    ENG_CHECK(e);
    if (n) {
        SPAI_PTR(p);
        SPAI_PTR(out);
    }
    return rules_mask(e, first, n, p, len, out);
}
int spai_rules_bench(spai_engine *e, uint32_t n, uint32_t iters, double *ms) {
    ENG_CHECK(e);
    SPAI_PTR(ms);
    return rules_bench(e, n, iters, ms);
}

int spai_net_num_params(int game, int blocks, int hidden, size_t *count) {
    SPAI_PTR(count);
    SPAI_CHECK(game == SPAI_GAME_CONNECT4 && blocks >= 0 && hidden > 0, SPAI_ERR_UNSUPPORTED,
               "net shape not supported (game %d, blocks %d, hidden %d)", game, blocks, hidden);
    *count = net_num_params(game, blocks, hidden);
    return SPAI_OK;
}

int spai_net_init_params(int game, int blocks, int hidden, uint64_t seed, float *params) {
    SPAI_PTR(params);
    SPAI_CHECK(game == SPAI_GAME_CONNECT4 && blocks >= 0 && hidden > 0, SPAI_ERR_UNSUPPORTED,
               "net shape not supported");
    net_init_params(game, blocks, hidden, seed, params);
    return SPAI_OK;
}

int spai_net_create(spai_engine *e, int blocks, int hidden, const float *params, size_t nparams, int dtype,
                    spai_net **out) {
    ENG_CHECK(e);
    SPAI_PTR(out);
    return net_create(e, blocks, hidden, params, nparams, dtype, out);
}

int spai_net_destroy(spai_net *n) {
    if (!n) return SPAI_OK;
    if (n->eng) {
        (void)hipSetDevice(n->eng->device);
        (void)hipStreamSynchronize(n->eng->stream);
        if (n->eng->net == n) n->eng->net = nullptr;
    }
    net_destroy(n);
    return SPAI_OK;
}

int spai_net_forward(spai_net *n, uint32_t cnt, const float *x, float *logits, float *value) {
    SPAI_PTR(n);
    ENG_CHECK(n->eng);
    if (cnt) {
        SPAI_PTR(x);
        SPAI_PTR(logits);
        SPAI_PTR(value);
    }
    return net_forward_x(n, cnt, x, logits, value);
}

int spai_predict(spai_net *n, uint32_t cnt, const spai_c4_state *s, float *priors, float *values) {
    SPAI_PTR(n);
    ENG_CHECK(n->eng);
    if (cnt) {
        SPAI_PTR(s);
        SPAI_PTR(priors);
        SPAI_PTR(values);
    }
    return net_predict(n, cnt, s, priors, values);
}

int spai_engine_set_net(spai_engine *e, spai_net *n) {
    ENG_CHECK(e);
    SPAI_CHECK(!n || n->eng == e, SPAI_ERR_INVALID, "net belongs to another engine");
    e->net = n;
    return eval_cache_clear(e);   // cached evaluations belong to the previous weights
}

int spai_net_set_params(spai_net *n, const float *params, size_t n_params) {
    SPAI_PTR(n);
    SPAI_PTR(params);
    ENG_CHECK(n->eng);
    return net_set_params(n, params, n_params);
}

int spai_net_set_params_from_learner(spai_net *n, spai_learner *l) {
    SPAI_PTR(n);
    SPAI_PTR(l);
    ENG_CHECK(n->eng);
    return net_set_params_from_learner(n, l);
}

int spai_eval_cache_set_capacity(spai_engine *e, uint64_t entries) {
    ENG_CHECK(e);
    return eval_cache_set_capacity(e, entries);
}

int spai_eval_cache_get_stats(spai_engine *e, spai_eval_cache_stats *out) {
    ENG_CHECK(e);
    SPAI_PTR(out);
    return eval_cache_stats(e, out);
}

int spai_eval_cache_thin(spai_engine *e, uint64_t keep_entries) {
    ENG_CHECK(e);
    return eval_cache_thin(e, keep_entries);
}

int spai_trees_create(spai_engine *e, uint32_t n) { ENG_CHECK(e); return trees_create(e, n); }
int spai_tree_reset(spai_engine *e, uint32_t t, const spai_c4_state *root) { ENG_CHECK(e); return tree_reset(e, t, root); }
int spai_search(spai_engine *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
                uint32_t *child_ids, float *child_visits, uint32_t *n_children) {
    ENG_CHECK(e);
    if (n) SPAI_PTR(tree_idx);
    return search(e, n, tree_idx, num_searches, policy, child_ids, child_visits, n_children, nullptr);
}
int spai_set_root_noise(spai_engine *e, float alpha, float epsilon) {
    ENG_CHECK(e);
    SPAI_CHECK(alpha >= 0.01f && alpha <= 100.0f, SPAI_ERR_INVALID, "root noise: alpha %g not in [0.01, 100]",
               (double)alpha);
    SPAI_CHECK(epsilon >= 0.0f && epsilon <= 1.0f, SPAI_ERR_INVALID, "root noise: epsilon %g not in [0, 1]",
               (double)epsilon);
    e->noise_alpha = alpha;
    e->noise_eps = epsilon;
    return SPAI_OK;
}

int spai_get_root_noise(spai_engine *e, float *alpha, float *epsilon) {
    ENG_CHECK(e);
    if (alpha) *alpha = e->noise_alpha;
    if (epsilon) *epsilon = e->noise_eps;
    return SPAI_OK;
}

int spai_root_noise(spai_engine *e, uint32_t count, const uint64_t *game_id, const uint32_t *move_no,
                    const uint32_t *n_children, float alpha, float *eta) {
    ENG_CHECK(e);
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

int spai_search_keyed(spai_engine *e, uint32_t n, const uint32_t *tree_idx, const uint64_t *game_id,
                      const uint32_t *move_no, uint32_t num_searches, float *policy, uint32_t *child_ids,
                      float *child_visits, uint32_t *n_children) {
    ENG_CHECK(e);
    if (n) {
        SPAI_PTR(tree_idx);
        SPAI_PTR(game_id);
        SPAI_PTR(move_no);
    }
    return search(e, n, tree_idx, num_searches, policy, child_ids, child_visits, n_children, nullptr, game_id,
                  move_no);
}

int spai_tree_use_subtree(spai_engine *e, uint32_t t, uint32_t child) { ENG_CHECK(e); return tree_use_subtree(e, t, child); }
int spai_tree_node(spai_engine *e, uint32_t t, uint32_t node, spai_c4_state *st, uint32_t *visits, float *w) {
    ENG_CHECK(e);
    return tree_node(e, t, node, st, visits, w);
}
int spai_tree_child_stats(spai_engine *e, uint32_t t, uint32_t *child_ids, uint32_t *visits, float *value_sums,
                          float *priors, uint32_t *n_children) {
    ENG_CHECK(e);
    return tree_child_stats(e, t, child_ids, visits, value_sums, priors, n_children);
}
int spai_tree_size(spai_engine *e, uint32_t t, uint32_t *nodes) {
    ENG_CHECK(e);
    SPAI_PTR(nodes);
    return tree_size(e, t, nodes);
}

int spai_selfplay_run(spai_engine *e, uint32_t n_games, uint64_t gid_base, spai_sample_sink sink, void *user,
                      spai_selfplay_stats *stats) {
    ENG_CHECK(e);
    SPAI_CHECK(n_games > 0 && n_games <= e->cfg.max_trees, SPAI_ERR_INVALID, "n_games %u not in [1, max_trees=%u]",
               n_games, e->cfg.max_trees);
    return selfplay_run(e, n_games, gid_base, sink, user, stats);
}

int spai_selfplay_stream(spai_engine *e, uint32_t n_games, uint32_t window, uint64_t gid_base, spai_sample_sink sink,
                         void *user, spai_selfplay_stats *stats) {
    ENG_CHECK(e);
    if (e->game != SPAI_GAME_CONNECT4) {
        set_error("self-play streaming: Connect4 engines");
        return SPAI_ERR_UNSUPPORTED;
    }
    if (window == 0) {
        set_error("window must be > 0");
        return SPAI_ERR_INVALID;
    }
    return selfplay_run(e, n_games, gid_base, sink, user, stats, window);
}

int spai_match_config_default(spai_match_config *cfg) {
    SPAI_PTR(cfg);
    *cfg = spai_match_config{};
    cfg->struct_size = (uint32_t)sizeof(spai_match_config);
    cfg->opening_plies = 4;
    cfg->seed = 0;
    return SPAI_OK;
}

int spai_match_run(spai_engine *e, const spai_match_player *a, const spai_match_player *b, uint32_t n_games,
                   uint64_t gid_base, const spai_match_config *cfg, spai_match_game *games, spai_match_stats *stats) {
    ENG_CHECK(e);
    SPAI_PTR(a);
    SPAI_PTR(b);
    SPAI_PTR(cfg);
    SPAI_CHECK(cfg->struct_size == sizeof(spai_match_config), SPAI_ERR_INVALID,
               "spai_match_config.struct_size %u, expected %zu", cfg->struct_size, sizeof(spai_match_config));
    SPAI_CHECK(cfg->opening_plies <= 6, SPAI_ERR_INVALID, "opening_plies %u > 6", cfg->opening_plies);
    SPAI_CHECK(n_games > 0 && 2 * (uint64_t)n_games <= e->cfg.max_trees, SPAI_ERR_INVALID,
               "a match of %u games needs %llu trees, max_trees=%u", n_games, 2ull * n_games, e->cfg.max_trees);
    for (const spai_match_player *p : {a, b}) {
        SPAI_CHECK(p->eval >= SPAI_EVAL_NET && p->eval <= SPAI_EVAL_HASH, SPAI_ERR_INVALID, "bad eval kind %d", p->eval);
        SPAI_CHECK(p->eval != SPAI_EVAL_NET || p->net, SPAI_ERR_INVALID, "player with eval = NET but no net");
        SPAI_CHECK(p->eval != SPAI_EVAL_NET || p->net->eng == e, SPAI_ERR_INVALID, "net belongs to another engine");
        SPAI_CHECK(p->num_searches >= 1 && p->num_searches <= e->cfg.num_searches, SPAI_ERR_INVALID,
                   "player num_searches %u not in [1, cfg.num_searches=%u]", p->num_searches, e->cfg.num_searches);
    }
    return match_run(e, a, b, n_games, gid_base, cfg, games, stats);
}

int spai_engine_set_timing(spai_engine *e, int enabled) {
    ENG_CHECK(e);
    KernelTimer &K = e->timer;
    K.enabled = enabled != 0;
    K.stride = enabled > 1 ? (uint32_t)enabled : enabled < 0 ? 1u : 4u;
    for (int i = 0; i < 3; ++i) K.total_ms[i] = K.launches[i] = K.items[i] = 0;
    K.used = 0;
    K.which.clear();
    K.iter.clear();
    return SPAI_OK;
}

int spai_engine_timing(spai_engine *e, double *avg_ms, double *launches) {
    ENG_CHECK(e);
    KernelTimer &K = e->timer;
    for (int i = 0; i < 3; ++i) {
        if (avg_ms) avg_ms[i] = K.launches[i] ? K.total_ms[i] / K.launches[i] : 0.0;
        if (launches) launches[i] = K.launches[i];
    }
    return SPAI_OK;
}

int spai_net_phase_cycles(spai_net *n, uint32_t count, double *cycles) {
    SPAI_PTR(n);
    SPAI_PTR(cycles);
    ENG_CHECK(n->eng);
    return net_phase_stamps(n, count, cycles);
}

int spai_net_bench(spai_net *n, uint32_t count, uint32_t iters, double *ms) {
    SPAI_PTR(n);
    SPAI_PTR(ms);
    ENG_CHECK(n->eng);
    return net_bench(n, count, iters, ms);
}

int spai_net_bench_conc(spai_net *n, uint32_t count, uint32_t iters, int conc, double *ms) {
    SPAI_PTR(n);
    SPAI_PTR(ms);
    ENG_CHECK(n->eng);
    if (conc < 1) {
        set_error("conc %d < 1", conc);
        return SPAI_ERR_INVALID;
    }
    return net_bench(n, count, iters, ms, conc);
}

int spai_engine_timing_items(spai_engine *e, double *total_ms, double *items) {
    ENG_CHECK(e);
    for (int i = 0; i < 3; ++i) {
        if (total_ms) total_ms[i] = e->timer.total_ms[i];
        if (items) items[i] = e->timer.items[i];
    }
    return SPAI_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- learner
int spai_adam_config_default(spai_adam_config *cfg) {
    SPAI_PTR(cfg);
    cfg->lr = 1e-3f;   // Adam::default().build(vs, 1e-3) (model/mod.rs:107)
    cfg->beta1 = 0.9f;
    cfg->beta2 = 0.999f;
    cfg->eps = 1e-8f;
    cfg->bn_momentum = 0.1f;   // nn::batch_norm2d(.., Default::default())
    cfg->bn_eps = 1e-5f;
    return SPAI_OK;
}

int spai_learner_create(spai_engine *e, int blocks, int hidden, const float *params, size_t n,
                        const spai_adam_config *cfg, spai_learner **out) {
    ENG_CHECK(e);
    SPAI_PTR(params);
    SPAI_PTR(out);
    *out = nullptr;
    return learner_create(e, blocks, hidden, params, n, cfg, out);
}

int spai_learner_destroy(spai_learner *l) {
    if (!l) return SPAI_OK;
    learner_destroy(l);
    return SPAI_OK;
}

int spai_learner_train_batch(spai_learner *l, uint32_t n, const float *states, const float *policies,
                             const float *values, float *loss) {
    SPAI_PTR(l);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    ENG_CHECK(l->eng);
    return learner_train_batch(l, n, states, policies, values, loss);
}

int spai_learner_train_batches(spai_learner *l, uint32_t k, uint32_t n, const float *states, const float *policies,
                               const float *values, float *losses) {
    SPAI_PTR(l);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    ENG_CHECK(l->eng);
    return learner_train_batches(l, k, n, states, policies, values, losses);
}

int spai_learner_params(spai_learner *l, float *params, size_t n) {
    SPAI_PTR(l);
    SPAI_PTR(params);
    ENG_CHECK(l->eng);
    return learner_params(l, params, n, false);
}

int spai_learner_grads(spai_learner *l, float *grads, size_t n) {
    SPAI_PTR(l);
    SPAI_PTR(grads);
    ENG_CHECK(l->eng);
    return learner_params(l, grads, n, true);
}

int spai_learner_activation(spai_learner *l, int layer, float *out, size_t n) {
    SPAI_PTR(l);
    SPAI_PTR(out);
    ENG_CHECK(l->eng);
    return learner_activation(l, layer, out, n);
}

int spai_comm_unique_id(uint8_t *id) {
    SPAI_PTR(id);
    return comm_unique_id(id);
}

int spai_learner_set_comm(spai_learner *l, int rank, int world, const uint8_t *id) {
    SPAI_PTR(l);
    ENG_CHECK(l->eng);
    if (world > 1) SPAI_PTR(id);   // world 1: an id makes a 1-rank RCCL communicator, NULL none
    return learner_set_comm(l, rank, world, id);
}

int spai_learner_broadcast(spai_learner *l, int root) {
    SPAI_PTR(l);
    ENG_CHECK(l->eng);
    return learner_broadcast(l, root);
}

int spai_learner_set_host_comm(spai_learner *l, int rank, int world, spai_host_allreduce fn, void *user) {
    SPAI_PTR(l);
    ENG_CHECK(l->eng);
    return learner_set_host_comm(l, rank, world, fn, user);
}

int spai_learner_last_batch(spai_learner *l, uint32_t *n) {
    SPAI_PTR(l);
    SPAI_PTR(n);
    *n = l->last_batch;
    return SPAI_OK;
}

// ---------------------------------------------------------------- checkpoints
int spai_params_save_safetensors(int game, int blocks, int hidden, const float *params, size_t n, const char *path) {
    SPAI_PTR(params);
    SPAI_PTR(path);
    return params_save_safetensors(game, blocks, hidden, params, n, path);
}

int spai_params_load_safetensors(int game, int blocks, int hidden, const char *path, float *params, size_t n) {
    SPAI_PTR(params);
    SPAI_PTR(path);
    return params_load_safetensors(game, blocks, hidden, path, params, n);
}

// ---------------------------------------------------------------- replay + pipeline
int spai_replay_create(uint32_t capacity, spai_replay **out) {
    SPAI_PTR(out);
    return replay_create(capacity, out);
}

int spai_replay_destroy(spai_replay *r) {
    if (r) replay_destroy(r);
    return SPAI_OK;
}

int spai_replay_push(spai_replay *r, uint32_t n, const float *states, const float *policies, const float *values) {
    SPAI_PTR(r);
    if (n) {
        SPAI_PTR(states);
        SPAI_PTR(policies);
        SPAI_PTR(values);
    }
    return replay_push(r, n, states, policies, values);
}

int spai_replay_pop(spai_replay *r, uint32_t n, float *states, float *policies, float *values) {
    SPAI_PTR(r);
    if (n) {
        SPAI_PTR(states);
        SPAI_PTR(policies);
        SPAI_PTR(values);
    }
    return replay_pop_now(r, n, states, policies, values);
}

int spai_replay_size(spai_replay *r, uint32_t *n) {
    SPAI_PTR(r);
    SPAI_PTR(n);
    return replay_size(r, n);
}

int spai_choose_multiple(uint32_t n, uint32_t k, uint64_t seed, uint64_t stream, uint32_t *out) {
    SPAI_PTR(out);
    std::vector<uint32_t> v;
    choose_multiple(n, k, seed, stream, v);
    std::copy(v.begin(), v.end(), out);
    return SPAI_OK;
}

#define PIPE_CFG_CHECK(cfg)                                                                                  \
    SPAI_CHECK((cfg)->struct_size == sizeof(spai_pipeline_config), SPAI_ERR_INVALID,                        \
               "spai_pipeline_config.struct_size is %u, this library expects %zu (set it to "                \
               "sizeof(spai_pipeline_config) of the header the library was built with)",                   \
               (unsigned)(cfg)->struct_size, sizeof(spai_pipeline_config))

int spai_pipeline_config_default(spai_pipeline_config *cfg) {
    SPAI_PTR(cfg);
    PIPE_CFG_CHECK(cfg);
    static const int dev0 = 0;
    *cfg = spai_pipeline_config{};
    cfg->struct_size = sizeof(spai_pipeline_config);
    cfg->n_selfplay = 1;
    cfg->selfplay_devices = &dev0;
    cfg->learner_device = 0;
    cfg->games_per_batch = 100;   // SelfPlayArgs::default (learner_concurrent.rs:50-59)
    cfg->num_searches = 600;
    cfg->c = 2.0f;
    cfg->temperature = 1.25f;
    cfg->batch_size = 128;        // TrainingArgs::default (:61-69)
    cfg->batches_per_iter = 20;
    cfg->train_iters = 10;
    cfg->replay_capacity = 128 * 100;   // main.rs:142
    cfg->sample_fraction = 0.3f;        // learner_concurrent.rs:278
    cfg->blocks = 4;                    // model::connect_four::Args::default
    cfg->seed = 0;
    cfg->checkpoint_dir = nullptr;
    return SPAI_OK;
}

int spai_pipeline_run(const spai_pipeline_config *cfg, const float *init_params, size_t n_params,
                      spai_pipeline_stats *stats) {
    SPAI_PTR(cfg);
    PIPE_CFG_CHECK(cfg);
    SPAI_PTR(init_params);
    return pipeline_run(cfg, init_params, n_params, stats);
}

int spai_learner_train(spai_learner *l, uint32_t n, const float *states, const float *policies, const float *values,
                       uint32_t epochs, uint32_t batch, uint64_t seed, float *loss) {
    SPAI_PTR(l);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    ENG_CHECK(l->eng);
    return learner_train_epochs(l, n, states, policies, values, epochs, batch, seed, loss);
}
