// search_internal.h — what search.hip, selfplay.hip and match.hip share: the kernels'
// views of the engine's buffers, the move record and the device pieces of a move
// step, and the host's chain launcher and per-call bookkeeping (search.hip).
#pragma once
#include "spai_internal.h"

namespace spai {

struct TreeView {
    uint4 *nodes;
    uint32_t cap;
    const uint32_t *root;
    uint32_t *next_free;
    const uint64_t *root_x, *root_o;
    const uint8_t *root_n, *root_status;
    uint32_t *path;
    uint8_t *depth;
    uint32_t *slot;   // the tree's leaf slot in the current batch, kNoSlot if terminal
    uint32_t *left;   // tail run-on mode: search iterations the tree still has to run
    uint32_t *evals;  // live leaves of this search call (the tail-mode policy's input)
};
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
// a hit of the evaluation cache: the tree's slot is in the batch's hit region (marked in T.slot)
constexpr uint32_t kHitSlot = 0x80000000u;

struct BatchView {
    uint32_t *count;
    uint32_t *more;   // tail mode: set when a tree stopped at the run cap with iterations left (else null)
    uint32_t *tree;
    uint64_t *mine, *theirs;
    float *priors;
    float *value;
    uint32_t *hits;   // evaluation cache: leaves served from it, in slots cap - 1 downwards (null: cache off)
    uint32_t cap;
};

// the evaluation cache as the kernels see it (search.hip "evaluation cache")
struct CacheView {
    uint4 *tab;      // null: off
    uint32_t mask;   // buckets - 1
    uint32_t gen;
    uint32_t *ctr;   // [0] live entries (claims since the clear or thinning + its survivors), [1] dropped inserts
    uint32_t seq;    // the search call's sequence number (chains_launch): what the entries' stamps are written with
};

struct RootsOut {
    uint32_t *root;
    uint64_t *x, *o;
    uint8_t *n, *status;
};

// ---------------------------------------------------------------- move step
// What a move step (k_advance, k_match_advance) leaves in engine.move_out, brought back by
// one copy: [0] the search call's error flags, [1] the evaluation cache's fill, one record per
// searched tree, then chain h's per-iteration leaf counts at h * stride.  A record: the root's
// children word, the child visit counts, the pick (index | action << 8 | new status << 16;
// without a move kPickNone and a reason: a weighted_index_f32 code, or kPickNoTable for a visit
// count beyond the visits^T table) and the tree's live leaves of the call.
constexpr int kMoveRec = 10;
constexpr int kRecRoot = 0, kRecVisits = 1, kRecPick = 8, kRecEvals = 9;
constexpr uint32_t kPickNone = 0x80000000u, kPickNoTable = 3u;
__host__ __device__ __forceinline__ uint32_t pick_word(int idx, int action, uint8_t status) {
    return (uint32_t)idx | (uint32_t)action << 8 | (uint32_t)status << 16;
}
inline int pick_index(uint32_t pick) { return (int)(pick & 0xFFu); }   // (without a move: the reason)
inline int pick_action(uint32_t pick) { return (int)((pick >> 8) & 0xFFu); }
inline uint8_t pick_status(uint32_t pick) { return (uint8_t)((pick >> 16) & 0xFFu); }
inline uint32_t root_children(uint32_t children_word) { return children_word == kNoChildren ? 0 : children_word >> 24; }
inline const uint32_t *move_rec(const uint32_t *out, size_t i) { return out + 2 + i * kMoveRec; }

// The host's check of a record against its own position rs: the picked index is a child, its
// action the index-th legal one, and playing it gives cs with the record's status.
inline bool move_replays(const uint32_t *rec, const c4::State &rs, c4::State &cs) {
    const uint32_t pick = rec[kRecPick], legal = c4::legal_mask(rs.x, rs.o, rs.status);
    const int idx = pick_index(pick), a = pick_action(pick);
    return (uint32_t)idx < root_children(rec[kRecRoot]) && a == c4::kth_bit(legal, idx) &&
           c4::next_state(rs, a, cs) == 0 && cs.status == pick_status(pick);
}

struct ChainCounts {
    const uint32_t *p[spai_engine::kChains];
    uint32_t n[spai_engine::kChains];   // counters of chain h (0: the chain did not run)
    uint32_t stride;
};

// tree t becomes an empty arena whose root is node 0
__device__ __forceinline__ void tree_clear(const TreeView &T, const RootsOut &R, uint32_t t) {
    T.nodes[(size_t)t * T.cap] = make_uint4(0u, 0u, 0u, kNoChildren);
    T.next_free[t] = 1;
    R.root[t] = 0;
}
// tree t's root position is s
__device__ __forceinline__ void root_position(const RootsOut &R, uint32_t t, const c4::State &s) {
    R.x[t] = s.x;
    R.o[t] = s.o;
    R.n[t] = s.n;
    R.status[t] = s.status;
}

// the words around the records: out[0], out[1], and block 0's copy of the chains' leaf counters
__device__ __forceinline__ void move_header(const uint32_t *err, const uint32_t *cache_fill, const ChainCounts &cc,
                                            uint32_t n_active, uint32_t *out) {
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        out[0] = *err;
        out[1] = cache_fill ? *cache_fill : 0u;
    }
    uint32_t *counts = out + 2 + (size_t)n_active * kMoveRec;
#pragma unroll
    for (int h = 0; h < spai_engine::kChains; ++h)
        for (uint32_t j = threadIdx.x; j < cc.n[h]; j += blockDim.x) counts[(size_t)h * cc.stride + j] = cc.p[h][j];
}

// tree t's root into its record: the children word, the child visit counts (also in
// vis) and the tree's live leaves; returns the children word
__device__ __forceinline__ uint32_t move_load_root(const TreeView &T, uint32_t t, uint32_t *rec,
                                                   uint32_t (&vis)[c4::kActions]) {
    const uint4 *nodes = T.nodes + (size_t)t * T.cap;
    const uint32_t w = nodes[T.root[t]].w;
    const uint32_t nch = w == kNoChildren ? 0 : w >> 24, first = w & 0xFFFFFFu;
#pragma unroll
    for (int k = 0; k < c4::kActions; ++k) vis[k] = (uint32_t)k < nch ? nodes[first + k].x : 0u;
    rec[kRecRoot] = w;
#pragma unroll
    for (int k = 0; k < c4::kActions; ++k) rec[kRecVisits + k] = vis[k];
    rec[kRecEvals] = T.evals[t];
    return w;
}

// play root child idx of tree t (children word w): the pick word, and for a game
// that goes on (returns true, cs the new position) the child as the tree's new root
__device__ __forceinline__ bool move_apply(const TreeView &T, const RootsOut &R, uint32_t t, uint32_t w, int idx,
                                           uint32_t *rec, c4::State &cs) {
    const c4::State rs{T.root_x[t], T.root_o[t], T.root_n[t], T.root_status[t]};
    const int a = c4::kth_bit(c4::legal_mask(rs.x, rs.o, rs.status), idx);
    cs = rs;
    (void)c4::next_state(rs, a, cs);
    rec[kRecPick] = pick_word(idx, a, cs.status);
    if (cs.status != c4::kOngoing) return false;
    R.root[t] = (w & 0xFFFFFFu) + (uint32_t)idx;
    root_position(R, t, cs);
    return true;
}

// ---------------------------------------------------------------- host, search.hip
// What search chain h runs in a call, on engine.chain_stream[h] (0: the engine stream) with engine.batch[h].
struct Chain {
    uint32_t off, cnt;   // its trees: engine.active[off .. off + cnt)
    uint32_t iters;      // search iterations
    int kind;            // evaluator (SPAI_EVAL_*), and the net when it is one
    spai_net *net;
    CacheView cache;     // tab null: none
};
// one search call's launch layout, for search_finish
struct SearchRun {
    int nchain = 1;
    uint32_t n_counts = 0;   // per-iteration leaf counters per chain
    Chain chain[spai_engine::kChains] = {};
};
constexpr uint32_t kTailChunk = 4;   // tail mode: passes per host check

// Dirichlet root noise of one search call (dirichlet.h, k_root_noise in search.hip); a
// launcher given none (null) enqueues nothing for it: spai_search, a match and an engine
// whose epsilon is 0.  The keys and the flag are per tree, not per entry of `active`.
struct RootNoise {
    float alpha, eps;
    uint64_t seed;
    const uint64_t *gid;    // device [n_trees]: each tree's game id (self-play: Trees::slot_gid)
    const uint32_t *move;   // device [n_trees]: each tree's move number (self-play: Trees::slot_move)
    uint32_t *done;         // device [n_trees]: the tree's root was mixed in this call
};
// the engine's noise over the per-tree key arrays, its flag array allocated on first use;
// on = false when its epsilon is 0 (then `out` is not to be passed on)
int root_noise_prepare(spai_engine *e, RootNoise &out, bool &on);

TreeView tree_view(spai_engine *e);
CacheView cache_view(spai_engine *e);   // the engine's cache at its current generation
inline RootsOut roots_out(spai_engine *e) {
    Trees &T = e->trees;
    return RootsOut{T.root.p, T.root_x.p, T.root_o.p, T.root_n.p, T.root_status.p};
}
int cache_prepare(spai_engine *e, bool for_net);
int cache_clear(spai_engine *e);
// Thin the table, between search calls, to at most keep_entries by the ranking of search.hip
// "thinning"; the generation stays, so the survivors stay valid.
int cache_thin(spai_engine *e, uint64_t keep_entries);
uint64_t cache_keep_budget(const EvalCache &C);   // what a thinning at the fill threshold keeps
// more than 7/8 full: time to thin it (a match: to empty it), between search calls (with two candidate buckets per
// position 0.4 % of the inserts find both full at that load; one bucket lost 7 % at 3/4)
inline bool cache_nearly_full(const EvalCache &C) { return C.buckets && (uint64_t)C.fill_seen * 8 > C.entries() * 7; }
// a call's leaves: `served` live ones, `forwarded` of them through the net; the table's fill after it
void cache_account(spai_engine *e, double served, double forwarded, uint32_t fill);
int check_device_errors(spai_engine *e, uint32_t err);
int chains_launch(spai_engine *e, const uint32_t *trees, const Chain *chains, int nchain, uint32_t grid_cap, bool timed,
                  bool tail, const RootNoise *noise = nullptr);
int search_launch(spai_engine *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, SearchRun &R,
                  const RootNoise *noise = nullptr);
int search_finish(spai_engine *e, const SearchRun &R, uint32_t num_searches, const uint32_t *ch_counts, uint32_t err,
                  uint32_t max_tree_evals, double served, uint32_t cache_fill);
int move_buffers(spai_engine *e, size_t n_words);   // selfplay.hip

// Every return of a run loop, errors included, leaves the engine's streams idle: the next move's
// search, move step and record copy may be in flight when a check fails.  fresh_trees > 0 (a
// match): also the cache emptied and that many trees as trees_create leaves them.
struct Quiesce {
    spai_engine *e;
    uint32_t fresh_trees;
    ~Quiesce() {
        (void)hipStreamSynchronize(e->stream);
        for (hipStream_t cs : e->chain_stream)
            if (cs) (void)hipStreamSynchronize(cs);
        if (!fresh_trees) return;
        (void)cache_clear(e);
        (void)trees_create(e, fresh_trees);
    }
};

// Policy::normalize: ndarray sum (sequential for 7) then divide
inline void normalize_policy(const float (&pol)[c4::kActions], float *out) {
    float s = 0.0f;
    for (int a = 0; a < c4::kActions; ++a) s = s + pol[a];
    for (int a = 0; a < c4::kActions; ++a) out[a] = pol[a] / s;
}

}  // namespace spai
