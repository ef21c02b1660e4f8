// chess_search_internal.h — what the chess search (chess_search.hip) shares with
// the chess match (chess_match.hip): the device view of the trees, the search
// chain and its launcher, and the move step of a tree (use_subtree).
#pragma once
#include "chess_engine.h"

namespace spai {
namespace chess {

constexpr int kWavesPerBlock = 4;
constexpr uint32_t kErrNan = 1, kErrDepth = 2, kErrCap = 4, kErrHist = 8;
constexpr int kMaxChildren = 218;   // most legal moves of any chess position

struct TV {
    uint4 *nodes;
    uint32_t *first;
    uint64_t *nhash;
    uint32_t *root, *fill, *half;
    Board *root_board;
    uint32_t *root_reps;
    uint64_t *hist;
    uint32_t *hist_n;
    uint32_t max_hist;
    uint32_t *path, *depth;
    uint16_t *leaf_moves;
    uint32_t *leaf_n;
    uint64_t *leaf_hash, *leaf_key;
    uint32_t cap;
};

__device__ __forceinline__ size_t tbase(const TV &T, uint32_t t) {
    return (size_t)t * 2 * T.cap + (size_t)T.half[t] * T.cap;
}

inline uint32_t blocks_for(uint32_t n) { return (n + kWavesPerBlock - 1) / kWavesPerBlock; }

// get_status (chess.rs:150-166) of a position from its move generation and repetition count
__device__ __forceinline__ int status_from(const GenOut &g, uint32_t reps, const Board &b) {
    if (g.n == 0) return g.in_check ? SPAI_WON : SPAI_TIED;
    return (reps >= 3 || b.fifty >= 100) ? SPAI_TIED : SPAI_ONGOING;
}

// tree t as a one-node tree whose root is b (lane 0 of the wave calls it); the history is the caller's
__device__ __forceinline__ void tree_one_node(const TV &T, uint32_t t, const Board &b, uint32_t reps, uint32_t hist_n) {
    const size_t base = (size_t)t * 2 * T.cap;
    T.nodes[base] = make_uint4(0u, 0u, 0u, 0u);
    T.first[base] = kNone;
    T.nhash[base] = 0;
    T.root[t] = 0;
    T.fill[t] = 1;
    T.half[t] = 0;
    T.root_board[t] = b;
    T.root_reps[t] = reps;
    T.hist_n[t] = hist_n;
}

// The move step of one tree by one wave: Tree::use_subtree(child) + the child's
// get_status (learner_concurrent.rs:194-197,234).  The root's list hash joins the
// game's transposition table, root child `pick` becomes the root (keeping N and W).
// b / reps = the new root position, status in b.status.  False (and kErrHist in
// *err): the table is full and the tree is unchanged.
__device__ __forceinline__ bool advance_step(const TV &T, uint32_t t, uint32_t pick, int lane, uint32_t *err, Board &b,
                                             uint32_t &reps) {
    const size_t base = tbase(T, t);
    const uint32_t r = T.root[t];
    const uint32_t child = T.first[base + r] + pick;
    b = T.root_board[t];
    const uint64_t rh = T.nhash[base + r];
    const uint32_t hn = T.hist_n[t];
    if (hn >= T.max_hist) {
        if (lane == 0) atomicOr(err, kErrHist);
        return false;
    }
    apply_move(b, (int)(T.nodes[base + child].w & 0xFFFFu));
    const GenOut g = wave_movegen(b, nullptr, lane);
    const uint64_t *hist = T.hist + (size_t)t * T.max_hist;
    uint32_t hits = lane == 0 && rh == g.hash ? 1u : 0u;
    for (uint32_t i = lane; i < hn; i += 64) hits += hist[i] == g.hash;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    reps = 1 + hits;
    b.status = (uint8_t)status_from(g, reps, b);
    if (lane == 0) {
        T.hist[(size_t)t * T.max_hist + hn] = rh;
        T.hist_n[t] = hn + 1;
        T.root[t] = child;
        T.root_board[t] = b;
        T.root_reps[t] = reps;
    }
    return true;
}

// One search chain: `n` trees (the device list `active`) searched for `sims`
// iterations with one evaluator, all of it in order on one stream, with its own
// leaf batch, per-iteration leaf counters and error word.  Self-play and
// spai_chess_search run the engine's own chain; a match runs two side by side.
struct Chain {
    hipStream_t stream = nullptr;
    const uint32_t *active = nullptr;   // device: the chain's trees
    uint32_t n = 0;
    Batch *batch = nullptr;             // cap >= n
    uint32_t *err = nullptr;            // device error word
    int kind = SPAI_EVAL_HASH;          // spai_eval
    spai_chess_net *net = nullptr;      // kind == SPAI_EVAL_NET
    uint32_t sims = 0;
    KernelTimer *timer = nullptr;       // null: nothing is sampled
    // Dirichlet root noise (dirichlet.h), off unless noise_eps > 0: a match builds its
    // chains without these fields and so never searches with noise
    float noise_eps = 0.0f, noise_alpha = 0.0f;
    uint64_t noise_seed = 0;
    const uint64_t *noise_gid = nullptr;    // device [n], parallel to active: each tree's game id
    const uint32_t *noise_move = nullptr;   // device [n], parallel to active: each tree's move number
    uint32_t *noise_done = nullptr;         // device [n]: the tree's root was noised in this call
};

TV view(spai_chess *e);
// the engine's own chain over the first n entries of e->active
Chain engine_chain(spai_chess *e, uint32_t n, uint32_t sims);
// enqueue the chain's whole search (compaction, then sims x leaf / forward / expand); n == 0 launches nothing.
// With noise_eps > 0 each tree's root children are mixed with a Dirichlet draw once in the call
// (k_croot_noise): after the compaction where the root has children on entry, else after iteration 0
int chain_launch(spai_chess *e, const Chain &C);
// wait for the chain, read its error word and leaf counters (evals = leaves evaluated), account its timer
int chain_finish(spai_chess *e, const Chain &C, double *evals);
// the SPAI_ERR_* of a device error word (0 -> SPAI_OK), with the message set
int err_code(spai_chess *e, uint32_t flags);

}  // namespace chess
}  // namespace spai
