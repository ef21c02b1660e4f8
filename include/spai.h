/*
 * spai.h — C ABI of the MI355X-native batched self-play MCTS engine.
 *
 * This is the drop-in boundary for the reference's hot path
 * (joshua16266261/self-play-ai).  The reference is in-process Rust with no FFI;
 * each entry point below replaces one trait method or function of that path,
 * cited as path:line relative to the reference root.  A Rust binding that
 * implements the reference traits on top of these symbols is in INTEGRATION.md.
 *
 * Conventions
 *  - Every function returns SPAI_OK (0) or a negative spai_error.  The message
 *    of the last failure on the calling thread is spai_last_error().  The
 *    reference reports rules errors as Result<_, String> (game/mod.rs:26,31)
 *    and panics on everything else (unwrap); those panics map to error codes.
 *  - Handles are opaque.  Buffers passed in or out are caller-owned HOST
 *    memory unless a parameter says "device".  Device memory and HIP streams
 *    are owned by the engine.
 *  - No global mutable state: one engine per host thread is fully independent,
 *    mirroring one Mcts + Model per self-play worker (main.rs:169-186).  An
 *    engine handle must not be used from two threads at once.
 *  - Connect4 states cross the boundary as spai_c4_state bitboards:
 *    bit (col*7 + row) of `x` / `o` holds X's / O's stone, row 0 = bottom
 *    (connect_four.rs:18), bit 6 of every column is always clear.  X moves
 *    first; the player to move is X iff num_actions_played is even
 *    (connect_four.rs:20-26,197).
 */
#ifndef SPAI_H
#define SPAI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPAI_VERSION_MAJOR 0
#define SPAI_VERSION_MINOR 5

typedef enum spai_error {
    SPAI_OK = 0,
    SPAI_ERR_INVALID = -1,       /* bad argument / handle / shape (e.g. mask_invalid_actions length) */
    SPAI_ERR_ILLEGAL_MOVE = -2,  /* Err("Illegal move: column already filled"), connect_four.rs:193 */
    SPAI_ERR_GAME_OVER = -3,     /* Err("Game has already ended"), connect_four.rs:209 */
    SPAI_ERR_DEVICE = -4,        /* HIP runtime failure */
    SPAI_ERR_NAN = -5,           /* NaN UCB or all-zero visits: the reference panics (mcts.rs:106-109) */
    SPAI_ERR_CAPACITY = -6,      /* node arena / batch capacity exceeded */
    SPAI_ERR_UNSUPPORTED = -7    /* game or net shape not built for this device path */
} spai_error;

typedef enum spai_game { SPAI_GAME_TICTACTOE = 0, SPAI_GAME_CONNECT4 = 1, SPAI_GAME_CHESS = 2 } spai_game;
typedef enum spai_status { SPAI_ONGOING = 0, SPAI_TIED = 1, SPAI_WON = 2 } spai_status; /* game/mod.rs:9-15 */

/* Evaluator used by search.  NET is Model::predict (model/mod.rs:36-98).  UNIFORM
 * and HASH are deterministic stub evaluators (not in the reference) used to pin
 * search and self-play bit-exactly against the CPU oracle. */
typedef enum spai_eval { SPAI_EVAL_NET = 0, SPAI_EVAL_UNIFORM = 1, SPAI_EVAL_HASH = 2 } spai_eval;

/* Arithmetic of a device net.  BF16: bf16 weights and activations on the MFMA
 * matrix cores, fp32 accumulate (the throughput path).  F32: the reference's
 * own fp32 arithmetic (model/mod.rs:36-98 runs libtorch in fp32), each output
 * summed in the CPU oracle's order, for parity work. */
typedef enum spai_dtype { SPAI_DTYPE_BF16 = 0, SPAI_DTYPE_F32 = 1 } spai_dtype;

typedef struct spai_c4_state {
    uint64_t x;                  /* X stones, bit col*7+row */
    uint64_t o;                  /* O stones */
    uint8_t num_actions_played;  /* connect_four.rs:24 */
    uint8_t status;              /* spai_status, connect_four.rs:25 */
    uint8_t pad[6];
} spai_c4_state;

/* mcts::Args (mcts.rs:9-18,46-59) + SelfPlayArgs (learner_concurrent.rs:21-26,50-59),
 * reduced to what the hot path reads, plus device sizing. */
typedef struct spai_config {
    float c;                 /* PUCT constant; the reference always uses Args::default().c = 2.0 (quirk Q6) */
    uint32_t num_searches;   /* simulations per move (Args.num_searches) */
    float temperature;       /* move sampling exponent on visit counts (learner_concurrent.rs:189-190) */
    uint32_t max_trees;      /* trees (parallel games) held on the device */
    uint32_t max_moves;      /* longest game; sizes the node arena (C4: 42) */
    uint32_t eval;           /* spai_eval */
    uint64_t seed;           /* move-sampling stream: Philox(seed, game id, move number) */
} spai_config;

typedef struct spai_engine spai_engine;
typedef struct spai_net spai_net;

/* ------------------------------------------------------------------ general */
const char *spai_last_error(void);
const char *spai_version(void);
int spai_device_count(int *count);
int spai_config_default(int game, spai_config *cfg);
int spai_engine_create(int game, const spai_config *cfg, int device, spai_engine **out);
int spai_engine_destroy(spai_engine *eng);
int spai_engine_sync(spai_engine *eng);

/* ------------------------------------------------------------------ rules
 * The State trait (game/mod.rs:21-33) batched over n engine-held game slots
 * [first, first+n) laid out as struct-of-arrays bitboards in HBM. */
int spai_games_resize(spai_engine *eng, uint32_t n);                       /* n slots = State::default() */
int spai_games_reset(spai_engine *eng, uint32_t first, uint32_t n);
int spai_games_write(spai_engine *eng, uint32_t first, uint32_t n, const spai_c4_state *states);
int spai_games_read(spai_engine *eng, uint32_t first, uint32_t n, spai_c4_state *states);
/* get_valid_actions (connect_four.rs:213-225) as a bitmask: bit a = action a legal */
int spai_legal_mask(spai_engine *eng, uint32_t first, uint32_t n, uint32_t *mask);
/* get_next_state (connect_four.rs:190-211) in place; rc[i] = 0 or a spai_error for slot i
 * (slot left unchanged on error).  Returns SPAI_OK if every slot succeeded, else the first error. */
int spai_apply(spai_engine *eng, uint32_t first, uint32_t n, const int32_t *actions, int32_t *rc);
/* get_value_and_terminated (connect_four.rs:231-240) */
int spai_value_terminated(spai_engine *eng, uint32_t first, uint32_t n, float *value, uint8_t *terminated);
/* get_encoding (connect_four.rs:242-259): out [n][3][6][7] f32 */
int spai_encode(spai_engine *eng, uint32_t first, uint32_t n, float *out);
/* mask_invalid_actions (connect_four.rs:261-279): policy [n][len] -> out [n][7]; len must be 7 */
int spai_mask_invalid(spai_engine *eng, uint32_t first, uint32_t n, const float *policy, uint32_t len,
                      float *out);
/* Device-resident timing of the rules kernels on n random reachable positions:
 * ms[0] legal mask, ms[1] apply+terminal, ms[2] encode (bf16), per launch. */
int spai_rules_bench(spai_engine *eng, uint32_t n, uint32_t iters, double *ms);

/* ------------------------------------------------------------------ net
 * Net trait (model/mod.rs:22-28) + Model::predict (model/mod.rs:36-98).
 * `params` are fp32 in module construction order (torso, policy head, value
 * head; conv = weight[co][ci][3][3], bias; batch_norm = weight, bias,
 * running_mean, running_var; linear = weight[out][in], bias) — the order tch
 * registers them for model/connect_four.rs:34-44.  Device path: hidden = 64. */
int spai_net_num_params(int game, int blocks, int hidden, size_t *count);
int spai_net_init_params(int game, int blocks, int hidden, uint64_t seed, float *params);
/* Net::new (model/mod.rs:22-28) with its weights: dtype = spai_dtype */
int spai_net_create(spai_engine *eng, int blocks, int hidden, const float *params, size_t nparams, int dtype,
                    spai_net **out);
int spai_net_destroy(spai_net *net);
/* Net::forward(x, train=false): x [n][3][6][7] f32 -> logits [n][7], value [n] (tanh) */
int spai_net_forward(spai_net *net, uint32_t n, const float *x, float *logits, float *value);
/* Model::predict: states -> masked softmax priors [n][7] (softmax then mask_invalid_actions), values [n] */
int spai_predict(spai_net *net, uint32_t n, const spai_c4_state *states, float *priors, float *values);
/* Evaluator that search uses when cfg.eval == SPAI_EVAL_NET (Mcts.model, mcts.rs:41-44) */
int spai_engine_set_net(spai_engine *eng, spai_net *net);
/* Weight refresh in place (either dtype): afterwards `net` is indistinguishable
 * from spai_net_create(eng, blocks, 64, params, n, dtype) -- same allocations,
 * same handle, every packed word equal (the BatchNorm fold and the fragment pack
 * run as a HIP kernel that restates spai_net_create's host packing; the array is
 * uploaded to a staging buffer the net allocates at the first call and keeps).
 * Runs on the engine's stream, behind every search that still reads the old
 * weights; returns once the new ones are in place.  If `net` is the engine's
 * current net the evaluation cache is cleared with a new generation, as by
 * spai_engine_set_net; another net leaves the cache alone.  A wrong n_params is
 * SPAI_ERR_INVALID and leaves the weights as they were.
 * (From a learner's device parameters: spai_net_set_params_from_learner.) */
int spai_net_set_params(spai_net *net, const float *params, size_t n_params);

/* ------------------------------------------------------------------ policy
 * Policy trait methods (game/mod.rs:35-44) on a flat policy array (Connect4 7,
 * TicTacToe 9, chess 4672 = get_flat_ndarray order).  Host functions.  For
 * chess, map the index to a move with spai_chess_index_move (get_action). */
/* Policy::normalize (connect_four.rs:96-98, chess.rs:518-520): p /= ndarray sum(p) */
int spai_policy_normalize(float *p, uint32_t n);
/* Policy::get_best_action (connect_four.rs:116-124, chess.rs:535-545): index of
 * the LAST maximum under f32::total_cmp (NaN above +inf, -0 below +0) */
int spai_policy_best_action(const float *p, uint32_t n, uint32_t *index);
/* Policy::sample (connect_four.rs:104-114, chess.rs:526-533): WeightedIndex
 * (rand 0.8) over p^temperature with f32 running totals.  u01 in [0, 1) is the
 * uniform that rand's UniformFloat<f32> draws, ((u32 >> 9) as f32) * 2^-23, so a
 * caller feeding its own rng's u32 reproduces rand's choice exactly.
 * SPAI_ERR_INVALID for an empty policy, a negative/NaN weight or all-zero weights. */
int spai_policy_sample(const float *p, uint32_t n, float temperature, float u01, uint32_t *index);

/* ------------------------------------------------------------------ search
 * Tree (mcts.rs:32-39,67-89,161-192) + Mcts::search (mcts.rs:196-332).
 * Trees live in HBM; node ids are per-tree handles (stable across
 * use_subtree; they are NOT the reference's BFS re-indexed arena offsets). */
int spai_trees_create(spai_engine *eng, uint32_t n);                                   /* n x Tree::default() */
int spai_tree_reset(spai_engine *eng, uint32_t tree, const spai_c4_state *root);       /* with_root_state; NULL = default */
/* Runs num_searches iterations over trees tree_idx[0..n).  Per tree i (A = 7):
 *   policy[i*A + a]       normalized root visit counts (Policy::normalize)
 *   child_ids[i*A + k]    node id of the k-th root child (legal-action order)
 *   child_visits[i*A + k] its visit count as f32
 *   n_children[i]
 * Any output pointer may be NULL. */
int spai_search(spai_engine *eng, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
                uint32_t *child_ids, float *child_visits, uint32_t *n_children);
/* Root exploration noise (AlphaZero's Dirichlet noise; the reference leaves it open,
 * mcts.rs:204-207), as for chess (spai_chess_set_root_noise).  OPT-IN: an engine is created
 * with epsilon = 0 and then searches exactly as the reference does, launching nothing more
 * than before.  With epsilon > 0, every keyed search call (spai_search_keyed, and the
 * searches of spai_selfplay_run / spai_selfplay_stream) mixes each searched tree's root
 * priors once, before the call's first selection at that root:
 *     P_j <- (1 - epsilon) * P_j + epsilon * eta_j,  eta ~ Dirichlet(alpha, ..., alpha)
 * over the root's children j in stored order (the legal columns, ascending), in float32
 * with 1 - epsilon rounded once and each product and the sum rounded on their own; no
 * renormalisation (both vectors sum to 1 up to rounding).  Only the children's prior words
 * are written; the evaluation cache keeps the net's own priors.  eta is a function of
 * (cfg.seed, game id, move number, number of children, alpha) alone -- the keys of
 * self-play's move draw, under a Philox key of its own; for the same values it is the draw
 * spai_chess_root_noise returns -- so a game does not depend on the window, on how games
 * are batched or split over game_id_base, on the search's chains and tail mode or on the
 * evaluation cache.  The mix is stored in the tree: a root searched twice without a move in
 * between is mixed twice.  spai_search, spai_match_run and spai_pipeline_run NEVER apply
 * noise, whatever is set here.
 * epsilon = 0 (default; alpha's default is 0.3): off.  alpha in [0.01, 100], epsilon in
 * [0, 1], else SPAI_ERR_INVALID (a NaN is out of range) */
int spai_set_root_noise(spai_engine *eng, float alpha, float epsilon);
int spai_get_root_noise(spai_engine *eng, float *alpha, float *epsilon);
/* the draws themselves, by the search's own device function: eta [count][7], entries
 * >= n_children[i] zero; n_children[i] in [1, 7]; seed = cfg.seed */
int spai_root_noise(spai_engine *eng, uint32_t count, const uint64_t *game_id, const uint32_t *move_no,
                    const uint32_t *n_children, float alpha, float *eta);
/* spai_search with root noise keyed per tree (the engine's alpha / epsilon; epsilon 0 = spai_search);
 * with epsilon > 0 a tree may be listed once only, else SPAI_ERR_INVALID */
int spai_search_keyed(spai_engine *eng, uint32_t n, const uint32_t *tree_idx, const uint64_t *game_id,
                      const uint32_t *move_no, uint32_t num_searches, float *policy, uint32_t *child_ids,
                      float *child_visits, uint32_t *n_children);
/* Tree::use_subtree(child) for a child of the root; the new root keeps N and W (quirk Q4) */
int spai_tree_use_subtree(spai_engine *eng, uint32_t tree, uint32_t child_id);
/* arena[node].state for the root or a root child; visits / value_sum of that node (may be NULL) */
int spai_tree_node(spai_engine *eng, uint32_t tree, uint32_t node_id, spai_c4_state *state, uint32_t *visits,
                   float *value_sum);
/* The root's child records, read-only, in legal-action order: node id, N, W (value_sum) and
 * the prior P of child k < n_children (the arrays hold 7; the rest are id 0xFFFFFFFF and
 * zeros).  n_children = 0 for a root not yet expanded.  Any output pointer may be NULL. */
int spai_tree_child_stats(spai_engine *eng, uint32_t tree, uint32_t *child_ids, uint32_t *visits, float *value_sums,
                          float *priors, uint32_t *n_children);
int spai_tree_size(spai_engine *eng, uint32_t tree, uint32_t *nodes);

/* ------------------------------------------------------------------ self-play
 * SelfPlayWorker::self_play (learner_concurrent.rs:169-242): n_games trees
 * from the default state, search every move, sample a root child with
 * probability proportional to N^temperature, record (root state, visit policy),
 * and when the sampled child is terminal emit the game's samples with the value
 * signed per player to move (:211-225).  The sink is called once per finished
 * game, in the reference's emission order. */
typedef void (*spai_sample_sink)(void *user, uint32_t game_id, uint32_t n, const float *encodings /* [n][3*6*7] */,
                                 const float *policies /* [n][7] */, const float *values /* [n] */,
                                 const int32_t *moves /* [n] action played at each position */);
typedef struct spai_selfplay_stats {
    double sims;        /* trees x search iterations */
    double evals;       /* leaves sent to the evaluator */
    double games;       /* finished games */
    double positions;   /* emitted samples */
    double moves;       /* search calls (plies of the longest game) */
    double seconds;     /* wall time of the call */
} spai_selfplay_stats;
int spai_selfplay_run(spai_engine *eng, uint32_t n_games, uint64_t game_id_base, spai_sample_sink sink, void *user,
                      spai_selfplay_stats *stats);
/* The same n_games games (ids game_id_base + i, i < n_games; every game's moves,
 * samples and outcome identical to spai_selfplay_run's, the draws keyed by the
 * game id and the game's own move number) played through `window` tree slots:
 * a finished game's slot takes the next game at once, so the device keeps
 * `window` games in flight until the last ones finish instead of searching
 * ever fewer trees as a lockstep batch runs out (the reference's main.rs:169-186
 * keeps the device busy with 6 concurrent workers instead).  The sink sees
 * finished games in the order they finish.  window >= n_games is
 * spai_selfplay_run; window <= max_trees. */
int spai_selfplay_stream(spai_engine *eng, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                         spai_sample_sink sink, void *user, spai_selfplay_stats *stats);

/* ------------------------------------------------------------------ evaluation cache
 * With cfg.eval == SPAI_EVAL_NET the search keeps a device-resident table from
 * the full leaf position to the net's masked priors and value, so a position
 * the net has already seen under the current weights (other games of the call,
 * transpositions inside a tree) is served from the table instead of going
 * through the forward again.  A hit returns the very bytes a forward wrote for
 * that position, so no result depends on the cache, its size or its state.
 * It is cleared by spai_engine_set_net (new weights); between search calls,
 * when it is more than 7/8 full, it is thinned to at most half its capacity
 * (SPAI_EVAL_CACHE_KEEP=<fraction> for measurements): the entries that were
 * ever hit and the newest stay (a match empties it instead).  Default capacity: 16384 entries per
 * tree slot of cfg.max_trees (64 B each, at most 1/16 of the device's total
 * memory, rounded down to a power of two of buckets); the environment
 * variable SPAI_EVAL_CACHE=<entries> overrides the default (0: off).
 * spai_selfplay_stats.evals counts served leaves (hits included);
 * spai_engine_timing_items counts the leaves the forward launches ran. */
/* entries: capacity (rounded down to a power-of-two number of 8-entry buckets, at
 * least one bucket); 0 turns the cache off.  Takes effect at the next search call
 * and overrides SPAI_EVAL_CACHE. */
int spai_eval_cache_set_capacity(spai_engine *eng, uint64_t entries);
typedef struct spai_eval_cache_stats {
    double lookups;     /* live leaves looked up (= evals while the cache is on) */
    double hits;        /* of them served from the table */
    double inserts;     /* entries written */
    double dropped;     /* inserts given up: both of the position's buckets were full */
    double clears;      /* times the table was emptied (set_net, resize, a match's fill threshold) or
                         * thinned (fill threshold, spai_eval_cache_thin): thinnings included */
    double capacity;    /* entries of the table now (0: off) */
    double thins;       /* thinnings */
    double evicted;     /* entries removed by thinnings */
    double live;        /* entries in the table now */
    double kept_hit;    /* entries a lookup had ever hit among those the latest thinning kept */
} spai_eval_cache_stats;
/* totals since the engine was created; waits for the engine's stream */
int spai_eval_cache_get_stats(spai_engine *eng, spai_eval_cache_stats *out);
/* Thin the table now to at most keep_entries entries, by the rule of the fill
 * threshold: entries that were ever hit first (at most 3/4 of keep_entries), then
 * the newest never-hit ones, in whole classes of equal age (in search calls), so
 * fewer may stay.  The survivors stay valid (no new generation).  0 empties the
 * table; a value at or above the live count evicts nothing.  For a caller that
 * wants memory pressure relieved, or the table pruned, without losing what it
 * learnt.  Waits for the engine's stream. */
int spai_eval_cache_thin(spai_engine *eng, uint64_t keep_entries);

/* ------------------------------------------------------------------ match
 * play() (main.rs:54-135) with a second evaluator in the human's seat, over
 * n_games games at once: which of two players (a net, or plain MCTS on a stub
 * evaluator) is the stronger.
 *   Game g has id game_id_base + g and belongs to pair id / 2; player A moves
 * first when the id is even, B when it is odd.  Both games of a pair start from
 * the same opening, so every opening is played once with each colour: ply
 * k < opening_plies plays the idx-th legal column in ascending order, idx =
 * min((int)(u * (float)n_legal), n_legal - 1) with u the 23-bit Philox uniform
 * of (cfg.seed, pair, k) (the uniform of self-play's move draw).
 *   Every game has one tree per player, both created at the position after the
 * opening.  The side to move searches its own tree with its own evaluator for
 * its own num_searches iterations, plays the most-visited root child (ties: the
 * last, spai_policy_best_action's rule) and re-roots its tree there
 * (use_subtree: the root keeps N and W).  The opponent's tree follows the move:
 * re-rooted at that action's child when its root is expanded, otherwise (only
 * before the second player's first search) a fresh tree at the new position.
 * A game ends on Won or Tied.  All the A-to-move trees of a ply run as one
 * search chain and all the B-to-move trees as the other, side by side.
 *   The engine's own cfg.eval, net and temperature are not used and stay as they
 * are.  The evaluation cache (above) serves each player only its own evaluations
 * and the call leaves it empty.  2 * n_games <= cfg.max_trees;
 * 1 <= num_searches <= cfg.num_searches; opening_plies <= 6 (no game ends before
 * ply 7): otherwise SPAI_ERR_INVALID.  A NaN UCB or a root without a visited
 * child (num_searches = 1) is SPAI_ERR_NAN, as in self-play. */
typedef struct spai_match_player {
    int32_t eval;            /* spai_eval */
    uint32_t num_searches;   /* simulations per move */
    spai_net *net;           /* SPAI_EVAL_NET: the player's net (bf16 or fp32); else ignored */
} spai_match_player;
typedef struct spai_match_config {
    uint32_t struct_size;    /* sizeof(spai_match_config) */
    uint32_t opening_plies;  /* 0..6 */
    uint64_t seed;           /* the openings' Philox key */
} spai_match_config;
typedef struct spai_match_game {
    uint64_t game_id;
    int8_t a_moves_first;
    int8_t result_a;         /* +1 A won, 0 draw, -1 B won */
    uint8_t n_moves;         /* plies, the opening's included */
    uint8_t moves[42];       /* the column of every ply */
} spai_match_game;
typedef struct spai_match_stats {
    double a_wins[2], draws[2], b_wins[2];   /* [0]: games A moved first, [1]: B moved first */
    double sims[2], evals[2];                /* per player (A, B): trees x iterations, live leaves */
    double seconds;
} spai_match_stats;
/* struct_size set, opening_plies 4, seed 0 */
int spai_match_config_default(spai_match_config *cfg);
/* games [n_games] and stats may be NULL.  Every return leaves the engine idle. */
int spai_match_run(spai_engine *eng, const spai_match_player *a, const spai_match_player *b, uint32_t n_games,
                   uint64_t game_id_base, const spai_match_config *cfg, spai_match_game *games,
                   spai_match_stats *stats);

/* ------------------------------------------------------------------ profiling
 * Per-kernel average device time of the last spai_selfplay_run / spai_search
 * call, measured with HIP events on each search chain's stream when enabled.
 * enabled = 1 samples every 4th search iteration; enabled = k > 1 every k-th;
 * enabled < 0 every iteration (each sampled iteration adds six event records per
 * chain). */
int spai_engine_set_timing(spai_engine *eng, int enabled);
/* ms[0] select, ms[1] evaluate (NN forward), ms[2] expand+backup; launches[3] */
int spai_engine_timing(spai_engine *eng, double *avg_ms, double *launches);
/* totals behind spai_engine_timing: summed sampled ms and the work items those
 * launches covered (trees for select/expand, evaluated leaves for the forward) */
int spai_engine_timing_items(spai_engine *eng, double *total_ms, double *items);
/* Diagnostic build-in: one forward over `count` random positions with s_memtime
 * stamps at every phase boundary of the fused kernel.  cycles[k] (k < 20) = mean
 * shader cycles from group start to stamp k (0 start, 1 stem, 2..13 residual
 * convs, 14 head conv, 15 linears, 16 end; 17/18/19 = block 0 conv1 k-loop end,
 * epilogue end, barrier passed).  Wall clock (s_memrealtime): cycles[20] = shader
 * cycles from kernel entry to the first group's start, [21] the same in ns, [22] ns
 * from the first group's start to the workgroup's end, [23] ns from the earliest
 * entry to the latest end over the launch.  cycles holds 24 doubles (48 in the
 * k-step diagnostic build, SPAI_DIAG_KSTEP: [24 + ks] after k-step ks of block 1
 * conv 1, [42] before its barrier, [43] after it, [44] its start).  Needs the
 * diagnostic build (SPAI_DIAG); the production library returns
 * SPAI_ERR_UNSUPPORTED.  Never on the timed path. */
int spai_net_phase_cycles(spai_net *net, uint32_t count, double *cycles);
/* Device time of the search's forward launch ALONE (nothing else on the GPU):
 * ms = mean over `iters` back-to-back launches on `count` random reachable
 * positions, HIP events on the engine stream.  Measurement only. */
int spai_net_bench(spai_net *net, uint32_t count, uint32_t iters, double *ms);
/* the same with the group size the search picks when `conc` search chains'
 * forwards share the CUs (conc 1 = spai_net_bench): the timed region's
 * configuration of a chain's forward, measured alone */
int spai_net_bench_conc(spai_net *net, uint32_t count, uint32_t iters, int conc, double *ms);

/* ---------------------------------------------------------------- learner
 * The training step of the C4 net on the device:
 * ModelTrainerWorker::train_batch (learner_concurrent.rs:72-85) = forward in
 * train mode (BatchNorm batch statistics, running statistics with momentum
 * 0.1), loss -(log_softmax(p)·pi).sum()/B + MSE(v, z) (model/mod.rs:128-135),
 * backward, and one Adam step (tch Adam::default(), lr 1e-3, model/mod.rs:107).
 * Parameters use spai_net_create's flat construction order, so
 * spai_learner_params() feeds spai_net_create() for the self-play replicas.
 * With a communicator (spai_learner_set_comm) each rank's mean gradient is
 * weighted by its share of the global batch (B_rank / sum B) and summed over
 * ranks with RCCL, so a step equals one step on the union of the ranks'
 * batches whatever their sizes; BatchNorm batch statistics stay per rank (DDP
 * without SyncBN) and the running statistics are averaged, so the replicas
 * stay identical. */
typedef struct spai_learner spai_learner;
/* The optimizer and train-mode BatchNorm settings of a learner (all three games).
 * spai_*_learner_create checks the ranges below, returns SPAI_ERR_INVALID with a
 * message that names the field, and leaves *out NULL; a NaN is out of every range.
 *   eps > 0 is required, not merely advised: the BatchNorm running statistics
 *   live in the parameter vector with gradient and moments 0, and they stay
 *   where the forward put them only because 0 / (0 + eps) is 0 (eps = 0: NaN).
 *   bn_eps and bn_momentum govern the train step alone.  The nets fold BatchNorm
 *   into their conv weights with a fixed 1e-5 (spai_net_create,
 *   spai_ttt_net_create / _set_params, spai_chess_net_create / _set_params), so
 *   parameters trained with another bn_eps are evaluated with 1e-5 in self-play. */
typedef struct spai_adam_config {
    float lr;            /* 1e-3;  finite, >= 0 (0: only the running statistics move) */
    float beta1, beta2;  /* 0.9, 0.999;  each in [0, 1) */
    float eps;           /* 1e-8;  finite, > 0 */
    float bn_momentum;   /* 0.1;  in [0, 1] */
    float bn_eps;        /* 1e-5;  finite, > 0 */
} spai_adam_config;
#define SPAI_COMM_ID_BYTES 128

int spai_adam_config_default(spai_adam_config *cfg);
int spai_learner_create(spai_engine *eng, int blocks, int hidden, const float *params, size_t n_params,
                        const spai_adam_config *cfg /* NULL = defaults */, spai_learner **out);
int spai_learner_destroy(spai_learner *l);
/* one optimizer step on n samples: states [n][3][6][7] (spai_encode layout),
 * policies [n][7], values [n]; loss[3] = total, policy, value (may be NULL) */
int spai_learner_train_batch(spai_learner *l, uint32_t n, const float *states, const float *policies,
                             const float *values, float *loss);
/* k consecutive train steps of n samples each (step j reads rows [j n, (j+1) n)
 * of the arrays): the same as k spai_learner_train_batch calls, with one host
 * synchronisation at the end (the next batch is staged while a step runs;
 * measured no faster than k single calls: the step is GPU-bound);
 * losses[3 k] = each step's total, policy, value (may be NULL) */
int spai_learner_train_batches(spai_learner *l, uint32_t k, uint32_t n, const float *states, const float *policies,
                               const float *values, float *losses);
/* Model::train (model/mod.rs:100-149): a fresh Adam, one random permutation of
 * the n samples (keyed by seed), then `epochs` passes of ceil(n / batch) train
 * steps (the last batch may be short); loss[3] = the last step's */
int spai_learner_train(spai_learner *l, uint32_t n, const float *states, const float *policies, const float *values,
                       uint32_t epochs, uint32_t batch, uint64_t seed, float *loss);
/* current parameters (incl. BN running statistics) / last step's gradients
 * (after the cross-rank reduction, before the 1/world scale), flat order */
int spai_learner_params(spai_learner *l, float *params, size_t n_params);
int spai_learner_grads(spai_learner *l, float *grads, size_t n_params);
/* spai_net_set_params from the learner's current device parameters, with no
 * host copy: the same kernel reads them in place, stream-ordered behind the
 * learner's latest step (learner and net share the engine's stream), so the next
 * call on the engine sees the new weights; bit-identical to
 * spai_net_set_params(net, <spai_learner_params>).  SPAI_ERR_INVALID, with the
 * mismatch named and the weights untouched, when the learner has another
 * blocks or hidden than the net or belongs to another engine. */
int spai_net_set_params_from_learner(spai_net *net, spai_learner *l);
/* the last train step's post-ReLU activations of conv layer `layer` (stem, the
 * 2*blocks residual convs, policy head, value head), [B][co][6][7]: the ReLU
 * masks the step took, for checking gradients against a float64 restatement */
int spai_learner_activation(spai_learner *l, int layer, float *out, size_t n);
/* RCCL communicator for a data-parallel learner: rank 0 makes the id
 * (spai_comm_unique_id), the host side broadcasts it, every rank joins.
 * world 1 with an id builds a 1-rank communicator (the all-reduce is then a
 * copy); world 1 with NULL drops the communicator. */
int spai_comm_unique_id(uint8_t *id /* SPAI_COMM_ID_BYTES */);
int spai_learner_set_comm(spai_learner *l, int rank, int world, const uint8_t *id);
/* A stand-alone RCCL communicator, one rank per GPU (comm.cpp).  The worker
 * fan-out it sits beside (main.rs:169-186,220-234) has no collective: the
 * sharded self-play bench reduces its per-rank work counters and step times
 * through it once per run, so an N-GPU run shows RCCL formed N ranks over
 * xGMI.  RCCL refuses two ranks on one device: such ranks use the host group.
 * spai_comm_allreduce_f64 reduces n host doubles in place (H2D, ncclAllReduce,
 * D2H on the communicator's stream; blocks until every rank has arrived). */
typedef struct spai_comm spai_comm;
enum { SPAI_REDUCE_SUM = 0, SPAI_REDUCE_MAX = 1 };
int spai_comm_create(int device, int rank, int world, const uint8_t *id /* SPAI_COMM_ID_BYTES */,
                     spai_comm **out);
int spai_comm_allreduce_f64(spai_comm *c, double *buf, size_t n, int op /* SPAI_REDUCE_* */);
int spai_comm_info(spai_comm *c, int *rank, int *world, int *device);
int spai_comm_destroy(spai_comm *c);
/* Weight refresh for self-play replicas (learner_concurrent.rs:158-159,260-264 hands the
 * trainer's weights to the self-play workers): RCCL broadcast of rank `root`'s parameters
 * to every rank of the communicator; a learner without one is left unchanged. */
int spai_learner_broadcast(spai_learner *l, int root);
/* Host collective in place of RCCL, for ranks that cannot form an RCCL
 * communicator (several ranks on one device, a host process group):
 * fn(user, buf, n) must sum the n floats of buf element-wise over the `world`
 * ranks in place (the same rank order on every rank, so the replicas stay
 * bit-identical) and return 0.  The step runs the same batch-size weighting and
 * running-statistic averaging as with RCCL; each all-reduce is staged through
 * pinned host memory and the call blocks in fn until every rank has arrived.
 * spai_learner_broadcast then sums rank `root`'s parameters with -0.0 from every
 * other rank (x + -0.0 == x for every x).  fn NULL (or world 1) drops it;
 * setting one drops an RCCL communicator and vice versa. */
typedef int (*spai_host_allreduce)(void *user, float *buf, size_t n);
int spai_learner_set_host_comm(spai_learner *l, int rank, int world, spai_host_allreduce fn, void *user);
/* the batch size of the latest train step (0 before the first); after
 * spai_learner_train it is the last minibatch's (n % batch, or batch) */
int spai_learner_last_batch(spai_learner *l, uint32_t *n);

/* ---------------------------------------------------------------- checkpoints
 * safetensors files with tch VarStore naming (VarStore::save / load,
 * learner.rs:192, main.rs:61): the flat construction-order parameters <-> one
 * F32 tensor per variable ("weight", "bias", "weight__2", ... "running_var__5"
 * ...), shapes as tch (conv [co][ci][k][k], linear [out][in]).  game = Connect4,
 * TicTacToe (hidden 64) or chess (hidden 256; the flat layout of
 * spai_chess_net_init_params).  Host-only: no device needed. */
int spai_params_save_safetensors(int game, int blocks, int hidden, const float *params, size_t n_params,
                                 const char *path);
int spai_params_load_safetensors(int game, int blocks, int hidden, const char *path, float *params,
                                 size_t n_params);

/* ---------------------------------------------------------------- replay + pipeline
 * Replay ring (learner_concurrent.rs:244-290, capacity batch_size*100 in
 * main.rs:142): pushes overwrite the oldest samples (push_iter_overwrite),
 * pops take the oldest n (pop_iter().take(n)).  Samples are one state
 * encoding [3][6][7], a policy [7] and a value.  Host memory, thread-safe. */
typedef struct spai_replay spai_replay;
int spai_replay_create(uint32_t capacity, spai_replay **out);
int spai_replay_destroy(spai_replay *r);
int spai_replay_push(spai_replay *r, uint32_t n, const float *states, const float *policies, const float *values);
/* SPAI_ERR_INVALID when fewer than n samples are buffered (non-blocking) */
int spai_replay_pop(spai_replay *r, uint32_t n, float *states, float *policies, float *values);
int spai_replay_size(spai_replay *r, uint32_t *n);
/* choose_multiple: k distinct indices of [0, n) from the Philox stream (seed, stream) */
int spai_choose_multiple(uint32_t n, uint32_t k, uint64_t seed, uint64_t stream, uint32_t *out);

/* train_concurrent (main.rs:137-235): n_selfplay self-play workers (host
 * threads, one engine each on selfplay_devices[w]) loop while training: take
 * the latest published weights, play games_per_batch games, push a random
 * sample_fraction of the positions into the replay ring.  The learner (on
 * learner_device) runs train_iters x batches_per_iter train steps of
 * batch_size popped samples, then publishes its weights and, if
 * checkpoint_dir is set, saves {checkpoint_dir}/{iter}.safetensors.
 * Reference defaults (SelfPlayArgs / TrainingArgs / C4 Args): c 2, 600 sims,
 * T 1.25, 100 games, batch 128, 20 batches x 10 iters, capacity 12800,
 * fraction 0.3, 4 blocks.
 *
 * Optional observer (cfg.observer, NULL = none): called under the replay ring's
 * lock, so the events arrive in ring order.  A PUSH event carries a worker's
 * subsample (n = (positions as f32 * fraction) as usize, learner_concurrent.rs:278)
 * and the weight version its games were played with; a POP event carries the
 * batch the trainer took for one train step and the number of weight versions
 * published so far.  Tests replay the events through a HeapRb model.  The
 * callback must not call back into the pipeline.  It runs while the ring's lock
 * is held, so every self-play worker and the trainer wait for it: it must be
 * fast and must not block (copy what it needs and return); run timings with an
 * observer are not representative. */
enum { SPAI_PIPE_PUSH = 0, SPAI_PIPE_POP = 1 };
typedef struct spai_pipeline_event {
    int32_t kind;          /* SPAI_PIPE_PUSH / SPAI_PIPE_POP */
    uint32_t worker;       /* push: worker index; pop: 0 */
    uint64_t batch;        /* push: the worker's self-play batch number; pop: train step */
    uint64_t version;      /* push: weight version played with; pop: versions published */
    uint32_t n;            /* samples pushed / popped */
    uint32_t positions;    /* push: positions of the self-play batch; pop: 0 */
    uint32_t ring_size;    /* samples buffered after the event */
    uint32_t pad;
    const float *states, *policies, *values;   /* [n][126], [n][7], [n] */
} spai_pipeline_event;
typedef void (*spai_pipeline_observer)(void *user, const spai_pipeline_event *ev);
typedef struct spai_pipeline_config {
    /* ABI guard: the caller sets struct_size = sizeof(spai_pipeline_config) before
     * spai_pipeline_config_default / spai_pipeline_run; a size the library was not
     * built with (a client compiled against another header) is refused with
     * SPAI_ERR_INVALID before anything is read or written (added in 0.2 with the
     * observer fields) */
    uint32_t struct_size;
    uint32_t n_selfplay;
    const int *selfplay_devices;   /* [n_selfplay] */
    int learner_device;
    uint32_t games_per_batch, num_searches;
    float c, temperature;
    uint32_t batch_size, batches_per_iter, train_iters, replay_capacity;
    float sample_fraction;
    int blocks;
    uint64_t seed;
    const char *checkpoint_dir;    /* NULL: no checkpoints */
    spai_pipeline_observer observer;   /* NULL: no events */
    void *observer_user;
} spai_pipeline_config;
typedef struct spai_pipeline_stats {
    double games, positions, samples_pushed, samples_overwritten, batches_trained;
    double last_loss[3];
    double weight_version_published, weight_version_used_max, seconds;
} spai_pipeline_stats;
int spai_pipeline_config_default(spai_pipeline_config *cfg);
int spai_pipeline_run(const spai_pipeline_config *cfg, const float *init_params, size_t n_params,
                      spai_pipeline_stats *stats);


/* ---------------------------------------------------------------- chess
 * game/chess.rs (the adapter over the `chess` crate 3.2.0) on the device:
 * config 4 of BASELINE.json.  A separate engine type: a position is a set of
 * bitboards, a move is a 16-bit code, the policy has 73*8*8 = 4672 entries
 * (chess.rs:252-257), the encoding is [19][8][8] (chess.rs:176-249).
 *
 * Move code: src | dst << 6 | promo << 12; squares rank*8 + file (a1 = 0);
 * promo = 1 knight, 2 bishop, 3 rook, 4 queen (chess::Piece index), 0 none.
 * Move lists are in MoveGen::new_legal enumeration order (piece type P, N, B,
 * R, Q, K; unpinned sources before pinned ones; en-passant captures after the
 * pawns; destinations ascending; promotions Q, N, R, B).  The reference's
 * repetition count compares these ordered lists (chess.rs:51-61); the device
 * compares 64-bit hashes of them. */
#define SPAI_CHESS_POLICY 4672
#define SPAI_CHESS_ENC 1216
#define SPAI_CHESS_MAX_MOVES 256

typedef struct spai_chess_state {
    uint64_t pieces[6];   /* Pawn, Knight, Bishop, Rook, Queen, King (chess::Piece order) */
    uint64_t colors[2];   /* White, Black */
    uint8_t side;         /* 0 White to move, 1 Black */
    uint8_t castle;       /* 1 white kingside, 2 white queenside, 4 black kingside, 8 black queenside */
    uint8_t ep;           /* chess::Board::en_passant: square of the pawn that just double-pushed, 64 = none */
    uint8_t status;       /* spai_status (filled by reads) */
    uint16_t fifty;       /* fifty_move_rule_halfmove_counter (chess.rs:29) */
    uint16_t made;        /* Action::MakeMove count of the Game (chess.rs:243-246) */
    uint32_t reps;        /* get_num_repetitions (chess.rs:51-61; filled by reads) */
    uint32_t pad;
} spai_chess_state;

typedef struct spai_chess spai_chess;
typedef struct spai_chess_net spai_chess_net;

/* cfg.max_moves = longest game (sizes the transposition tables).  Default 12,304: the
 * fifty-move counter (reset by pawn moves, captures and at most 4 castle-rights
 * changes) bounds a game at 12,298 plies, so the default covers every legal game. */
int spai_chess_config_default(spai_config *cfg);
int spai_chess_create(const spai_config *cfg, int device, spai_chess **out);
int spai_chess_destroy(spai_chess *e);
int spai_chess_sync(spai_chess *e);

/* rules over n engine-held slots, each with its own transposition table */
int spai_chess_games_resize(spai_chess *e, uint32_t n);                  /* n x State::default() */
int spai_chess_games_write(spai_chess *e, uint32_t first, uint32_t n, const spai_chess_state *s); /* empty table */
int spai_chess_games_read(spai_chess *e, uint32_t first, uint32_t n, spai_chess_state *s);
/* get_valid_actions (chess.rs:148): moves [n][SPAI_CHESS_MAX_MOVES], counts [n] */
int spai_chess_legal_moves(spai_chess *e, uint32_t first, uint32_t n, uint16_t *moves, uint32_t *counts);
/* get_next_state (chess.rs:108-146) in place: rc SPAI_ERR_GAME_OVER ("Game is already
 * over") or SPAI_ERR_ILLEGAL_MOVE ("Failed to make move"); the slot is unchanged on error */
int spai_chess_apply(spai_chess *e, uint32_t first, uint32_t n, const uint16_t *moves, int32_t *rc);
/* get_status (chess.rs:150-166) and get_num_repetitions; get_value_and_terminated
 * (chess.rs:168-174: Won -> +1, quirk Q7).  Any output may be NULL. */
int spai_chess_status(spai_chess *e, uint32_t first, uint32_t n, uint8_t *status, uint32_t *reps, float *value,
                      uint8_t *terminated);
/* get_encoding: out [n][19][8][8] f32 */
int spai_chess_encode(spai_chess *e, uint32_t first, uint32_t n, float *out);
/* Device time (HIP events, mean of iters launches) of the batched rules kernels
 * over slots [first, first+n): ms[0] legal move lists + counts + status,
 * ms[1] encoding.  Measurement only; slots are not modified. */
int spai_chess_rules_bench(spai_chess *e, uint32_t first, uint32_t n, uint32_t iters, double *ms);
/* perft of slot `slot`'s position on the device: counts[d-1] = the number of legal
 * move sequences of length d, d = 1..depth (<= 8), by the movegen and make-move
 * the search uses (MoveGen::new_legal / Board::make_move of the chess crate,
 * game/chess.rs:54,117-118); breadth first, one Board array per ply in HBM
 * (SPAI_ERR_CAPACITY past 2^26 positions in one ply) */
int spai_chess_perft(spai_chess *e, uint32_t slot, int depth, uint64_t *counts);
/* mask_invalid_actions (chess.rs:252-275): policy [n][len] -> out [n][4672]; len must be 4672 */
int spai_chess_mask_invalid(spai_chess *e, uint32_t first, uint32_t n, const float *policy, uint32_t len,
                            float *out);
/* Policy::get_prob / set_prob flat index of a move (get_channel, chess.rs:311-393) */
int spai_chess_move_index(int side, uint16_t move, int32_t *index);
/* Policy::get_action (chess.rs:395-493), including its knight-underpromotion bug (:442) */
int spai_chess_index_move(int side, int32_t index, uint16_t *move);

/* net: model/chess.rs:48-77 (torso = stem + `blocks` residual blocks of 256
 * channels; policy head conv1x1 256->256 + ReLU + conv1x1 256->73; value head
 * conv1x1 256->1 + ReLU + linear 64->256 + ReLU + linear 256->1 + tanh).  params
 * in tch construction order as for spai_net_create.  spai_chess_net_create builds
 * the bf16 net (bf16 MFMA, fp32 accumulate): it is spai_chess_net_create_dtype with
 * SPAI_DTYPE_BF16. */
int spai_chess_net_num_params(int blocks, size_t *count);
int spai_chess_net_init_params(int blocks, uint64_t seed, float *params);
int spai_chess_net_create(spai_chess *e, int blocks, const float *params, size_t n_params, spai_chess_net **out);
/* The same net in the arithmetic `dtype` (SPAI_DTYPE_BF16 or SPAI_DTYPE_F32; anything
 * else is SPAI_ERR_INVALID).  An fp32 net is usable wherever a chess net is: forward,
 * predict, spai_chess_set_net (search, self-play), a match player (the two players
 * may differ in dtype), spai_chess_net_set_params.  It is the parity path, about
 * 50 times slower than bf16 (profiles/chess_net_f32).  Its input planes are not rounded
 * (planes 17 and 18 are fractions), and every output element is summed in one fixed
 * order with separate multiply and add, so that a float32 restatement on the CPU
 * (tests/chess_f32_ref.py) reproduces every logit and the value's pre-activation bit
 * for bit:
 *   3x3 convs   the conv bias first, then the products input channel ascending,
 *               kernel row, kernel column; an off-board tap is skipped;
 *   BatchNorm   unfolded, ((x - mean) * inv) * gamma + beta with inv =
 *               1.0f / sqrtf(var + 1e-5f) computed on the host in float32;
 *   residual    relu(h + bn(conv(...))), the block input h as the left operand;
 *   heads       conv1x1 and linear outputs: the bias first, then the input index
 *               ascending (policy conv1x1 256->256 + ReLU, conv1x1 256->73; value
 *               conv1x1 256->1 + ReLU over the 64 cells, linear 64->256 + ReLU,
 *               linear 256->1, tanhf).
 * Only tanhf (and predict's expf) may differ from the host's libm in the last ulp.
 * A position's result does not depend on its batch slot or on the rest of the batch. */
int spai_chess_net_create_dtype(spai_chess *e, int blocks, const float *params, size_t n_params,
                                int dtype /* spai_dtype */, spai_chess_net **out);
/* the spai_dtype the net was created with */
int spai_chess_net_dtype(spai_chess_net *net, int *dtype);
int spai_chess_net_destroy(spai_chess_net *net);
/* Net::forward(x, train=false): x [n][19][8][8] -> logits [n][4672], value [n] */
int spai_chess_net_forward(spai_chess_net *net, uint32_t n, const float *x, float *logits, float *value);
/* Model::predict (model/mod.rs:36-98) over game slots [first, first+n): encoding
 * (with each slot's repetition count), forward, softmax, mask_invalid_actions ->
 * priors [n][4672], values [n]; all on the device. */
int spai_chess_predict(spai_chess_net *net, uint32_t first, uint32_t n, float *priors, float *values);
int spai_chess_set_net(spai_chess *e, spai_chess_net *net);

/* search: Tree (mcts.rs) + Mcts::search over chess trees held on the device.
 * Per tree i: policy [i][4672] normalized root visits (NULL allowed),
 * child_ids / child_visits / child_moves [i][SPAI_CHESS_MAX_MOVES], n_children [i]. */
int spai_chess_trees_create(spai_chess *e, uint32_t n);                   /* n x Tree::default() */
int spai_chess_search(spai_chess *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
                      uint32_t *child_ids, float *child_visits, uint16_t *child_moves, uint32_t *n_children);
/* Tree::use_subtree for the k-th root child (k in [0, n_children)); the new root keeps N and W */
/* Tree::with_root_state (mcts.rs:86-89): tree `tree` becomes a one-node tree rooted at the
 * state held in game slot `slot` (board, MakeMove count, fifty-move counter and the slot's
 * history of earlier positions, which the repetition rule reads) */
int spai_chess_tree_reset(spai_chess *e, uint32_t tree, uint32_t slot);
int spai_chess_tree_use_subtree(spai_chess *e, uint32_t tree, uint32_t child_index);
int spai_chess_tree_root(spai_chess *e, uint32_t tree, spai_chess_state *root, uint32_t *visits, float *value_sum);
/* use_subtree for n trees at once (child_index[i] of tree_idx[i]'s root children); status[i] /
 * reps[i] = get_status / get_num_repetitions of the new root (either may be NULL) */
int spai_chess_trees_advance(spai_chess *e, uint32_t n, const uint32_t *tree_idx, const uint32_t *child_index,
                             uint8_t *status, uint32_t *reps);

/* Root exploration noise (AlphaZero's Dirichlet noise; the reference leaves it open,
 * mcts.rs:204-207).  OPT-IN: an engine is created with epsilon = 0 and then searches
 * exactly as the reference does, launching nothing more than before.  With epsilon > 0,
 * every keyed search call (spai_chess_search_keyed, and the searches of
 * spai_chess_selfplay_run / _stream / _compact) mixes each searched tree's root priors
 * once, before the call's first selection at that root:
 *     P_j <- (1 - epsilon) * P_j + epsilon * eta_j,  eta ~ Dirichlet(alpha, ..., alpha)
 * over the root's children j in stored (MoveGen) order, in float32 with 1 - epsilon
 * rounded once and each product and the sum rounded on their own; no renormalisation
 * (both vectors sum to 1 up to rounding).  Only the children's prior words are written.
 * eta is a function of (cfg.seed, game id, move number, number of children, alpha)
 * alone -- the keys of self-play's move draw, under a Philox key of its own -- so a
 * game does not depend on how games are batched, windowed or sharded.  The mix is
 * stored in the tree: a root searched twice without a move in between is mixed twice.
 * spai_chess_search and spai_chess_match_run NEVER apply noise, whatever is set here.
 * epsilon = 0 (default): off.  alpha in [0.01, 100], epsilon in [0, 1], else SPAI_ERR_INVALID */
int spai_chess_set_root_noise(spai_chess *e, float alpha, float epsilon);
int spai_chess_get_root_noise(spai_chess *e, float *alpha, float *epsilon);
/* the draws themselves, by the search's own device function: eta [count][SPAI_CHESS_MAX_MOVES],
 * entries >= n_children[i] zero; n_children[i] in [1, 218]; seed = cfg.seed */
int spai_chess_root_noise(spai_chess *e, uint32_t count, const uint64_t *game_id, const uint32_t *move_no,
                          const uint32_t *n_children, float alpha, float *eta);
/* spai_chess_search with root noise keyed per tree (engine's alpha / epsilon; epsilon 0 = plain search);
 * with epsilon > 0 a tree may be listed once only */
int spai_chess_search_keyed(spai_chess *e, uint32_t n, const uint32_t *tree_idx, const uint64_t *game_id,
                            const uint32_t *move_no, uint32_t num_searches, float *policy, uint32_t *child_ids,
                            float *child_visits, uint16_t *child_moves, uint32_t *n_children);

/* SelfPlayWorker::self_play (learner_concurrent.rs:169-242) for chess */
typedef void (*spai_chess_sample_sink)(void *user, uint32_t game_id, uint32_t n,
                                       const float *encodings /* [n][19*64] */,
                                       const float *policies /* [n][4672] */, const float *values /* [n] */,
                                       const uint16_t *moves /* [n] move played at each position */);
int spai_chess_selfplay_run(spai_chess *e, uint32_t n_games, uint64_t game_id_base, spai_chess_sample_sink sink,
                            void *user, spai_selfplay_stats *stats);
/* The same n_games chess games played through `window` tree slots (window <=
 * max_trees), a finished game's slot taking the next game at once; every game
 * identical to spai_chess_selfplay_run's (draws keyed by game id and the game's
 * own move number), the sink sees games in the order they finish. */
int spai_chess_selfplay_stream(spai_chess *e, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                               spai_chess_sample_sink sink, void *user, spai_selfplay_stats *stats);
/* timing of the last search / self-play call, as spai_engine_timing:
 * ms[0] select + leaf rules, ms[1] net forward, ms[2] expand + backup */
int spai_chess_set_timing(spai_chess *e, int enabled);
int spai_chess_timing(spai_chess *e, double *avg_ms, double *launches, double *items);

/* weight refresh of a self-play net of either dtype in place: the array is uploaded to a
 * staging buffer the net owns (allocated by the first call) and HIP kernels restate the
 * host packing of spai_chess_net_create / _create_dtype into the same allocations
 * (BatchNorm folded in double and bf16 fragments, or the fp32 net's layout), on the
 * engine's stream behind any search still reading the old weights.  Every packed word
 * (spai_chess_net_image), and so forward afterwards, is bit-identical to a net freshly
 * created from the same parameters; padded lanes are rewritten as zero every time.
 * NaN parameters are outside that claim (sign and payload).  Returns once the weights
 * are in place: `params` is the caller's again.  A wrong n_params is SPAI_ERR_INVALID
 * with the weights untouched.  (From a learner's device parameters:
 * spai_chess_net_set_params_from_learner.) */
int spai_chess_net_set_params(spai_chess_net *net, const float *params, size_t n_params);
/* The checker's window on a net's packed weights: drains the engine's stream and copies
 * the net's weight buffers to `out` back to back, in this order:
 *   bf16 net  w_stem, w_res, w_p1, w_p2 (bf16 MFMA A fragments [ks = tap*CB + cb][ct]
 *             [lane 64][8], BatchNorm folded), then fp32 b_stem, b_res, b_p1, b_p2 (80:
 *             73 biases and 7 zeros), v_w, v_b, l1_w, l1_b, l2_w, l2_b; at blocks = 0
 *             w_res and b_res are placeholders of 8 and 4 zero elements;
 *   fp32 net  wf, the one fp32 buffer of spai_chess_net_create_dtype's layout.
 * *bytes = the image's size; out == NULL only reports it; cap < *bytes is
 * SPAI_ERR_INVALID.  Two nets whose images are equal compute the same function. */
int spai_chess_net_image(spai_chess_net *net, void *out, size_t cap, size_t *bytes);

/* Device train step of the chess net (model/chess.rs:48-70 under
 * model/mod.rs:128-141) in exact fp32 (f32 MFMA), on the engine's device and
 * stream: train-mode forward (BatchNorm batch statistics in the trunk),
 * loss = -(log_softmax(p) . pi).sum() / B + mean((v - z)^2), backward, one Adam
 * step.  Parameters are the flat vector of spai_chess_net_num_params /
 * spai_chess_net_init_params (BN running statistics included).  Deterministic:
 * the same parameters and batches give bit-identical losses, gradients and
 * parameters.  A non-finite loss returns SPAI_ERR_NAN. */
typedef struct spai_chess_learner spai_chess_learner;
int spai_chess_learner_create(spai_chess *e, int blocks, const float *params, size_t n_params,
                              const spai_adam_config *cfg /* NULL = defaults */, spai_chess_learner **out);
int spai_chess_learner_destroy(spai_chess_learner *l);
/* states [n][19*64] (spai_chess_encode layout), policies [n][4672], values [n]; loss[3] = total, policy, value (may be NULL) */
int spai_chess_learner_train_batch(spai_chess_learner *l, uint32_t n, const float *states, const float *policies,
                                   const float *values, float *loss);
/* Model::train: fresh Adam, one permutation (choose_multiple(n, n, seed, 0x7EA1B), as spai_learner_train),
 * epochs x ceil(n/batch) steps, short last batch */
int spai_chess_learner_train(spai_chess_learner *l, uint32_t n, const float *states, const float *policies,
                             const float *values, uint32_t epochs, uint32_t batch, uint64_t seed, float *loss);
int spai_chess_learner_params(spai_chess_learner *l, float *params, size_t n_params);
int spai_chess_learner_grads(spai_chess_learner *l, float *grads, size_t n_params);
/* the last train step's post-ReLU activations: layers 0 .. 2*blocks the trunk convs
 * [B][256][64], 2*blocks+1 the first policy conv [B][256][64], 2*blocks+2 the value conv
 * [B][64], 2*blocks+3 the first value linear [B][256] */
int spai_chess_learner_activation(spai_chess_learner *l, int layer, float *out, size_t n);
int spai_chess_learner_last_batch(spai_chess_learner *l, uint32_t *n);
/* The compute type of the conv GEMMs: SPAI_DTYPE_F32 (the default: the exact fp32
 * step above) or SPAI_DTYPE_BF16 (mixed precision); anything else is
 * SPAI_ERR_INVALID.  In bf16 every operand of every conv GEMM (forward, data
 * gradient, weight gradient; trunk and policy head) is rounded to bf16, nearest
 * even; the products are summed in fp32 and stored as fp32.  Bias, BatchNorm, the
 * residual add, ReLU, the losses, the value head, Adam, the master parameters and
 * every activation and gradient in device memory stay fp32; bf16 keeps fp32's
 * exponent, so there is no loss scaling.  Still deterministic to the bit.  May be
 * called between steps: drains the stream; parameters, Adam moments and step
 * count are kept. */
int spai_chess_learner_set_compute(spai_chess_learner *l, int dtype /* spai_dtype */);
int spai_chess_learner_get_compute(spai_chess_learner *l, int *dtype);
/* The checker's window, in both compute types.  With capture on (off is the default
 * and costs nothing; on changes no result) a step keeps copies of the gradients it
 * otherwise overwrites, and spai_chess_learner_gradient returns, of the last step:
 * layer 0 .. 2*blocks the gradient with respect to that trunk conv's pre-BN output
 * [B][256][64]; 2*blocks+1 the ReLU-masked gradient of the first policy conv's
 * output [B][256][64]; 2*blocks+2 the logits' gradient [B][4672].
 * SPAI_ERR_INVALID: no step yet, the last step was not captured, wrong n.
 * spai_chess_learner_logits returns the last step's logits [B][4672] (needs no
 * capture; SPAI_ERR_INVALID: no step yet, wrong n). */
int spai_chess_learner_set_capture(spai_chess_learner *l, int on);
int spai_chess_learner_gradient(spai_chess_learner *l, int layer, float *out, size_t n);
int spai_chess_learner_logits(spai_chess_learner *l, float *out, size_t n);
/* spai_chess_net_set_params from the learner's current device parameters, with no host
 * copy and no host synchronisation: the same kernels read them in place on the engine's
 * stream, behind the learner's latest step and behind every search still reading the old
 * weights, and the call returns once enqueued; the next call on the engine sees the new
 * weights.  The net holds a snapshot, not an alias: later train steps do not change it.
 * Bit-identical to spai_chess_net_set_params(net, <spai_chess_learner_params>), for
 * either net dtype and either learner compute type (the master parameters are fp32).
 * (A match's second chain runs on a stream of its own, which spai_chess_match_run
 * drains before it returns, so a refresh after a match needs no further ordering.)
 * SPAI_ERR_INVALID before anything is launched, with the mismatch named and the weights
 * untouched, when the learner belongs to another engine, has another block count or
 * holds another number of parameters than the net needs. */
int spai_chess_net_set_params_from_learner(spai_chess_net *net, spai_chess_learner *l);

/* ------------------------------------------------------------ chess match
 * play() (main.rs:54-135, whose commented-out lines are the chess variant) with
 * a second evaluator in the human's seat, over n_games chess games at once: the
 * chess form of spai_match_run ("match" above), in its wording where the games
 * allow it.
 *   Game g has id game_id_base + g and belongs to pair id / 2; player A moves
 * first (plays the first searched ply) when the id is even, B when it is odd.
 * Both games of a pair start from the same position: cfg.start[pair -
 * game_id_base / 2] when start is given (loaded with an empty transposition
 * table, as by spai_chess_games_write), otherwise State::default(), and then
 * opening_plies plies played from it: ply k plays the idx-th move of the
 * position's legal list in MoveGen order, idx = min((int)(u * (float)n_legal),
 * n_legal - 1) with u the 23-bit Philox uniform of (cfg.seed, pair, k) (the
 * uniform of self-play's move draw).  The opening's positions enter the game's
 * repetition history like any played move.
 *   Every game has one tree per player, both Tree::with_root_state of the
 * position after the opening, history included.  The side to move searches its
 * own tree with its own evaluator for its own num_searches iterations, plays the
 * most-visited root child (ties: the last) and re-roots its tree there
 * (use_subtree: the root keeps N and W, the old root's list hash joins the
 * tree's history).  The opponent's tree follows the move: advanced to the child
 * carrying that move code when its root is expanded (the same child index, both
 * roots being the same position), otherwise (only before the second player's
 * first search) a fresh one-node tree at the new position with the mover's
 * history.  After the step both trees agree on root board, repetition count and
 * history.  A game ends on Won (the mover wins) or Tied.  Adjudication: a game
 * whose n_moves reaches max_plies (0 = no limit) while still Ongoing ends as a
 * draw with adjudicated = 1.  moves receives the first min(n_moves,
 * moves_stride) move codes of each game.  All the A-to-move trees of a ply run
 * as one search chain and all the B-to-move trees as the other, side by side on
 * two streams.
 *   The engine's own cfg.eval, net, temperature and timers are neither used nor
 * changed; its trees are replaced, as spai_chess_selfplay_run replaces them.
 * SPAI_ERR_INVALID: start != NULL together with opening_plies != 0; a start
 * position that is not Ongoing, or without exactly one king per side (the rule
 * of spai_chess_games_write); a struct_size other than
 * sizeof(spai_chess_match_config); opening_plies > 3; 2 * n_games > cfg.max_trees;
 * num_searches outside 1..cfg.num_searches; NET with a null net or a net of
 * another engine; moves != NULL with moves_stride == 0.  Memory: a tree takes
 * 2 * cap * 28 B with cap = max(4 * cfg.num_searches * 218, 16384), plus
 * cfg.max_moves * 8 B of history: about 19.5 MB per tree at 400 simulations,
 * and a game holds two.  A NaN UCB or a root without a visited child
 * (num_searches = 1) is SPAI_ERR_NAN, as in self-play; arena, depth and history
 * overflows are SPAI_ERR_CAPACITY.  Every return leaves the engine idle and
 * usable. */
typedef struct spai_chess_match_player {
    int32_t eval;              /* spai_eval: NET, UNIFORM or HASH */
    uint32_t num_searches;     /* simulations per move, 1..cfg.num_searches */
    spai_chess_net *net;       /* SPAI_EVAL_NET: this player's net; else ignored */
} spai_chess_match_player;
typedef struct spai_chess_match_config {
    uint32_t struct_size;      /* sizeof(spai_chess_match_config) */
    uint32_t opening_plies;    /* 0..3 (no chess game ends before ply 4); default 2 */
    uint32_t max_plies;        /* 0 = none; see "adjudication"; default 512 */
    uint32_t moves_stride;     /* uint16 entries per game in `moves` (0 if moves == NULL) */
    uint64_t seed;             /* the openings' Philox key */
    const spai_chess_state *start;   /* NULL, or one start position per pair */
} spai_chess_match_config;
typedef struct spai_chess_match_game {
    uint64_t game_id;
    int8_t a_moves_first, result_a;   /* +1 A won, 0 draw, -1 B won */
    uint8_t status;                   /* spai_status of the final position (ONGOING iff adjudicated) */
    uint8_t adjudicated;
    uint32_t n_moves;                 /* plies played, the opening's included */
} spai_chess_match_game;
typedef struct spai_chess_match_stats {
    double a_wins[2], draws[2], b_wins[2];   /* [0] games A moved first, [1] B moved first */
    double sims[2], evals[2];                /* per player: trees x iterations, leaves evaluated */
    double adjudicated, plies, seconds;
} spai_chess_match_stats;
/* struct_size set, opening_plies 2, max_plies 512, moves_stride 0, seed 0, start NULL */
int spai_chess_match_config_default(spai_chess_match_config *cfg);
int spai_chess_match_run(spai_chess *e, const spai_chess_match_player *a, const spai_chess_match_player *b,
                         uint32_t n_games, uint64_t game_id_base, const spai_chess_match_config *cfg,
                         spai_chess_match_game *games /* [n_games] or NULL */,
                         uint16_t *moves /* [n_games][moves_stride] or NULL */,
                         spai_chess_match_stats *stats /* or NULL */);
/* Measurement only: on != 0 runs both chains of later matches in order on the
 * engine's stream instead of side by side on two (the default).  Results are the same. */
int spai_chess_match_set_one_stream(spai_chess *e, int on);
/* root children of a tree without searching it (n = 0: root not expanded):
 * moves / visits [SPAI_CHESS_MAX_MOVES], zero past n; any output may be NULL */
int spai_chess_tree_children(spai_chess *e, uint32_t tree, uint16_t *moves, uint32_t *visits, uint32_t *n);
/* the same read with each child's whole node record, in stored (MoveGen) order: move, N, W and
 * prior exactly as stored (n = 0: root not expanded).  Reads the tree's active half, so it holds
 * after a compaction; it does not search and does not change the tree.
 * moves / visits / value_sums / priors [SPAI_CHESS_MAX_MOVES], zero past n; any output may be NULL */
int spai_chess_tree_child_stats(spai_chess *e, uint32_t tree, uint16_t *moves, uint32_t *visits, float *value_sums,
                                float *priors, uint32_t *n);

/* -------------------------------------------------- chess compact samples
 * A self-play sample as self-play knows it: the searched position, the value, and
 * the root children's (move, visit count) pairs, instead of the dense [19][8][8]
 * encoding and [4672] policy row built from them (23,556 bytes a position).  The
 * children of a set of samples are stored CSR-style in two arrays, child_moves
 * (move codes, in MoveGen order as the tree stores them) and child_visits (N);
 * sample i owns entries [first, first + n_children) of both.
 *
 * The dense form of a sample is: states = the encoding of `state` with plane 16
 * = state.reps; policies = zeros with (float)N_k / sum_k (float)N_k at
 * spai_chess_move_index(state.side, move_k); values = value.
 *
 * Every entry point below that takes samples checks them on the host first, before
 * anything is uploaded or launched, and returns SPAI_ERR_INVALID (the message names
 * the sample's index and the field; a learner's parameters, moments and step count
 * are untouched) when
 *   n_children is outside 1..SPAI_CHESS_MAX_MOVES;
 *   first + n_children goes past n_children_total;
 *   the state has not exactly one king per side (spai_chess_games_write's rule);
 *   state.side > 1;
 *   a child's policy index falls outside [0, 4672);
 *   two children of the sample have the same policy index (the moves of a legal
 *     move list never do);
 *   the sample's visit counts sum to 0 or to 2^24 or more (below 2^24 every partial
 *     sum is an exact integer in fp32, so the sum does not depend on its order). */
typedef struct spai_chess_sample {
    spai_chess_state state;  /* the searched position; .reps = its repetition count (plane 16), .status ignored */
    float    value;          /* z, signed for the player to move */
    uint16_t move;           /* the move played */
    uint16_t n_children;     /* 1..SPAI_CHESS_MAX_MOVES */
    uint32_t first;          /* index of its first child in child_moves / child_visits */
    uint32_t pad;
} spai_chess_sample;         /* 96 bytes */

/* one finished game: n samples in move order, `first` relative to this call's arrays */
typedef void (*spai_chess_compact_sink)(void *user, uint32_t game_id, uint32_t n,
                                        const spai_chess_sample *samples, const uint16_t *child_moves,
                                        const uint32_t *child_visits, uint32_t n_children_total);
/* spai_chess_selfplay_run (window == 0 or >= n_games) or spai_chess_selfplay_stream
 * (otherwise) with the samples handed over compact: the same games, draws, emission
 * order and stats; spai_chess_samples_expand of a game's samples is, bit for bit,
 * what the dense sink receives for it. */
int spai_chess_selfplay_compact(spai_chess *e, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                                spai_chess_compact_sink sink, void *user, spai_selfplay_stats *stats);
/* The dense form on the host (needs no device), by the functions the dense sink's
 * arrays are made with: states [n][19*64], policies [n][4672], values [n]; any of
 * the three may be NULL. */
int spai_chess_samples_expand(uint32_t n, const spai_chess_sample *samples, const uint16_t *child_moves,
                              const uint32_t *child_visits, uint32_t n_children_total, float *states,
                              float *policies, float *values);
/* spai_chess_learner_train_batch on the samples' dense form, which a HIP kernel
 * writes on the learner's device from the uploaded records: bit-identical to
 * spai_chess_learner_train_batch on spai_chess_samples_expand's arrays. */
int spai_chess_learner_train_batch_compact(spai_chess_learner *l, uint32_t n, const spai_chess_sample *samples,
                                           const uint16_t *child_moves, const uint32_t *child_visits,
                                           uint32_t n_children_total, float *loss);
/* Model::train over n * repeat virtual samples, virtual sample j being sample j % n
 * (repeat >= 1): bit-identical to spai_chess_learner_train on the expanded arrays
 * tiled repeat times (the same permutation, choose_multiple(n * repeat, n * repeat,
 * seed, 0x7EA1B)), without building them. */
int spai_chess_learner_train_compact(spai_chess_learner *l, uint32_t n, const spai_chess_sample *samples,
                                     const uint16_t *child_moves, const uint32_t *child_visits,
                                     uint32_t n_children_total, uint32_t repeat, uint32_t epochs, uint32_t batch,
                                     uint64_t seed, float *loss);
/* The checker's window: the last train step's batch as the step read it on the
 * device, whichever route brought it there.  states [n][19*64], policies [n][4672],
 * values [n], any of them NULL; SPAI_ERR_INVALID before the first step or when n is
 * not the last step's batch size. */
int spai_chess_learner_batch(spai_chess_learner *l, float *states, float *policies, float *values, uint32_t n);


/* ---------------------------------------------------------------- tictactoe
 * game/tictactoe.rs + model/tictactoe.rs (BASELINE config 1) on the device.
 * Board = two 9-bit masks, bit row*3 + col (the flat action index of the
 * row-major 3x3 Policy, tictactoe.rs:100-102); X moves first; X to move iff
 * num_actions_played is even.  Same conventions as the Connect4 entry points;
 * the net is fp32 (hidden 64) and the policy has 9 entries. */
typedef struct spai_ttt_state {
    uint16_t x, o;
    uint8_t num_actions_played, status;
    uint8_t pad[2];
} spai_ttt_state;
typedef struct spai_ttt spai_ttt;
typedef struct spai_ttt_net spai_ttt_net;
int spai_ttt_create(const spai_config *cfg, int device, spai_ttt **out);
int spai_ttt_destroy(spai_ttt *e);
int spai_ttt_games_resize(spai_ttt *e, uint32_t n);
int spai_ttt_games_write(spai_ttt *e, uint32_t first, uint32_t n, const spai_ttt_state *s);
int spai_ttt_games_read(spai_ttt *e, uint32_t first, uint32_t n, spai_ttt_state *s);
int spai_ttt_legal_mask(spai_ttt *e, uint32_t first, uint32_t n, uint32_t *mask);        /* tictactoe.rs:169-182 */
int spai_ttt_apply(spai_ttt *e, uint32_t first, uint32_t n, const int32_t *actions, int32_t *rc);  /* :127-167 */
int spai_ttt_encode(spai_ttt *e, uint32_t first, uint32_t n, float *out);                /* [n][3][3][3], :199-216 */
int spai_ttt_mask_invalid(spai_ttt *e, uint32_t first, uint32_t n, const float *policy, uint32_t len,
                          float *out);                                                   /* :218-236, len 9 */
int spai_ttt_net_num_params(int blocks, size_t *count);
int spai_ttt_net_init_params(int blocks, uint64_t seed, float *params);
int spai_ttt_net_create(spai_ttt *e, int blocks, const float *params, size_t n_params, spai_ttt_net **out);
int spai_ttt_net_destroy(spai_ttt_net *net);
int spai_ttt_net_forward(spai_ttt_net *net, uint32_t n, const float *x, float *logits, float *value);
/* Model::predict over game slots [first, first+n) -> priors [n][9], values [n] */
int spai_ttt_predict(spai_ttt_net *net, uint32_t first, uint32_t n, float *priors, float *values);
int spai_ttt_set_net(spai_ttt *e, spai_ttt_net *net);
int spai_ttt_trees_create(spai_ttt *e, uint32_t n);
/* per tree i: policy [i][9], child_ids / child_visits [i][9], n_children [i] (any may be NULL) */
int spai_ttt_search(spai_ttt *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
                    uint32_t *child_ids, float *child_visits, uint32_t *n_children);
/* Tree::with_root_state (mcts.rs:86-89) */
int spai_ttt_tree_reset(spai_ttt *e, uint32_t tree, const spai_ttt_state *root);
int spai_ttt_tree_use_subtree(spai_ttt *e, uint32_t tree, uint32_t child_index);
/* SelfPlayWorker::self_play; the sink gets encodings [n][27], policies [n][9], values, moves */
int spai_ttt_selfplay_run(spai_ttt *e, uint32_t n_games, uint64_t game_id_base, spai_sample_sink sink, void *user,
                          spai_selfplay_stats *stats);
/* the same games through `window` tree slots (spai_selfplay_stream's contract) */
int spai_ttt_selfplay_stream(spai_ttt *e, uint32_t n_games, uint32_t window, uint64_t game_id_base,
                             spai_sample_sink sink, void *user, spai_selfplay_stats *stats);
/* weight refresh of a self-play net in place (the fold + transpose of
 * spai_ttt_net_create into the same allocations): forward afterwards is
 * bit-identical to a net freshly created from the same parameters */
int spai_ttt_net_set_params(spai_ttt_net *net, const float *params, size_t n_params);

/* Device train step of the TicTacToe net (model/tictactoe.rs:50-81 under
 * model/mod.rs:128-141) in fp32, on the engine's device and stream: the step of
 * spai_learner_* on a 3x3 board with a 9-way policy head.  Parameters are the
 * flat vector of spai_ttt_net_num_params / spai_ttt_net_init_params (BN running
 * statistics included).  Deterministic: the same parameters and batches give
 * bit-identical losses, gradients and parameters. */
typedef struct spai_ttt_learner spai_ttt_learner;
int spai_ttt_learner_create(spai_ttt *e, int blocks, const float *params, size_t n_params,
                            const spai_adam_config *cfg /* NULL = defaults */, spai_ttt_learner **out);
int spai_ttt_learner_destroy(spai_ttt_learner *l);
/* states [n][27] (spai_ttt_encode layout), policies [n][9], values [n]; loss[3] = total, policy, value (may be NULL) */
int spai_ttt_learner_train_batch(spai_ttt_learner *l, uint32_t n, const float *states, const float *policies,
                                 const float *values, float *loss);
/* Model::train: fresh Adam, one permutation (choose_multiple(n, n, seed, 0x7EA1B), as spai_learner_train),
 * epochs x ceil(n/batch) steps, short last batch */
int spai_ttt_learner_train(spai_ttt_learner *l, uint32_t n, const float *states, const float *policies,
                           const float *values, uint32_t epochs, uint32_t batch, uint64_t seed, float *loss);
int spai_ttt_learner_params(spai_ttt_learner *l, float *params, size_t n_params);
int spai_ttt_learner_grads(spai_ttt_learner *l, float *grads, size_t n_params);
/* the last train step's post-ReLU activations of conv `layer` (stem, the 2*blocks
 * residual convs, policy conv, value conv), [B][co][3][3] */
int spai_ttt_learner_activation(spai_ttt_learner *l, int layer, float *out, size_t n);
int spai_ttt_learner_last_batch(spai_ttt_learner *l, uint32_t *n);

#ifdef __cplusplus
}
#endif
#endif
