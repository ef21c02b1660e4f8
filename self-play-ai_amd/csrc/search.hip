// search.hip — device-resident MCTS (mcts.rs): the tree kernels, the evaluation
// cache, the chain and tail-mode policies, the chain launcher (also self-play's,
// selfplay.hip, and a match's, match.hip; shared declarations: search_internal.h)
// and a call's bookkeeping, spai_search and the tree API.
//
// Trees live in HBM as per-tree arenas of 16-B node records (spai_internal.h).
// One search iteration (mcts.rs:214-285) is two launches per search chain:
//   evaluate        the fused ResNet forward (net_c4.hip) or a stub evaluator
//                   over this iteration's leaf batch;
//   k_expand_select per tree, 8 lanes (one per board column): expand the tree's
//                   leaf of this iteration if it had one (legal moves by
//                   ballot, children packed by a prefix count, priors written,
//                   value backed up along the recorded path, lanes splitting
//                   the levels), then the NEXT iteration's PUCT descent from
//                   the root (state replayed on bitboards, leaf terminal check;
//                   terminal leaves backed up in place, live leaves appended to
//                   the next batch).
// Trees are independent, so expanding tree t and selecting tree t again in one
// launch is the reference's per-tree order (expand+backprop of iteration i,
// then select of i+1) and the results are those of separate launches; the
// fusion removes one kernel boundary from every iteration's critical path.
// The first iteration starts with k_select alone, the last ends with k_expand.
// Leaf batches are double-buffered by iteration parity, and every iteration
// has its own slot counter (zeroed once per search call).
// Opt-in Dirichlet root noise (spai_set_root_noise; k_root_noise, chains_launch): with
// epsilon > 0 a keyed search or self-play call mixes every root's priors once, before
// the first selection at it, for which the call's first iteration runs unfused
// (k_expand, k_root_noise, k_select); with epsilon 0 nothing of it is enqueued.
// The host only sees the trees between moves: root visit counts come back once
// per search call, or the record of a move step that ran on the device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dirichlet.h"
#include "search_internal.h"

namespace spai {
namespace {

constexpr int kLanesPerTree = 8;
constexpr int kBlock = 64;   // threads per tree-kernel workgroup (kBlock / 8 trees)
constexpr int kTreesPerBlock = kBlock / kLanesPerTree;
constexpr uint32_t kErrNan = 1u, kErrCapacity = 2u, kErrDepth = 4u;

// ---------------------------------------------------------------- evaluation cache
// A hash table in HBM from a leaf's full position (mine, theirs) to what the
// evaluator wrote for it: the 7 masked priors and the value.  The evaluator's
// output for a position depends on nothing but the position and the weights, so
// a cached result is the recomputed one bit for bit.
//
// Layout: buckets of 8 ways (one per lane of a tree's group), 64 B per entry:
//   word 0  mine   | gen << 49      the claim word (0: empty)
//   word 1  theirs | gen << 49
//   word 2  p0 p1 | word 3  p2 p3 | word 4  p4 p5 | word 5  p6 value
// Every 8-byte word carries a non-zero mark: the generation (1..32767) above
// the 49 board bits of the key words, the sign bit of the even prior (priors are
// >= +0; an entry whose priors are not is never inserted) in the payload words.
// A position has two candidate buckets (cache_buckets): a lookup reads both in
// one round trip, an insert takes a way of the emptier one, so that a bucket
// fills up only when both do (at 3/4 load 7 % of the keys find their one bucket
// full, 0.001 % both of two: scripts/eval_cache_hitrate.py, bucket_loss).  The
// same position in both buckets (two writers at once) is a harmless duplicate.
// The entry's last quarter holds two stamps that no lookup ever reads, sequence
// numbers of search calls (CacheView::seq):
//   word 6 low   born: the call in which the entry was claimed (the claimer's store)
//   word 6 high  hit:  the latest call in which a lookup accepted it, 0 if none
//                (one plain 4-byte store by the lane that holds the matching way;
//                every writer of one call stores the same value)
// They rank the entries when the table is thinned ("thinning", below).
//
// Protocol (no fence anywhere): an entry is claimed by one agent-scope CAS of
// word 0 from empty and then written once, by the claimer alone; its six key
// and payload words are not overwritten until the table is cleared or thinned,
// and that happens only in stream order while no search kernel runs (a memset,
// or the sweep that zeroes whole entries).  So whatever a reader sees
// of an entry -- its L1 is per CU, the L2s per XCD, the other chain may be
// writing it right now -- is a subset of the entry's final words, the rest
// zero.  The reader accepts only when all six words are marked and both key
// words equal its own (full position and generation): then it holds exactly
// the bytes one forward wrote for exactly this position.  Anything less reads
// as a miss, and the leaf goes through the forward as before.
constexpr uint32_t kPriorMark = 0x80000000u;
constexpr int kGenShift = 49;

// PUCT score, mcts.rs:91-100, evaluated in the reference's operation order
// (no contraction: built with -ffp-contract=off; sqrt and / correctly rounded).
// sqrt_np = sqrtf(parent visits), computed while the children's records load.
// The quotient is computed for every child and selected (an unvisited child has
// q = 0): under a branch the compiler sank the load of the record's value sum
// into it, which put a second dependent memory round trip on every level.
__device__ __forceinline__ float ucb(float sqrt_np, const uint4 &ch, float c) {
    const uint32_t n = ch.x;
    const float w = __uint_as_float(ch.y), prior = __uint_as_float(ch.z);
    const float qv = ((-w / (float)(n == 0 ? 1u : n)) + 1.0f) / 2.0f;
    const float q = n == 0 ? 0.0f : qv;
    float u = c * prior;
    u = u * sqrt_np;
    u = u / (1.0f + (float)n);
    return q + u;
}

// backprop (mcts.rs:145-159) over path[0..d]: level d is the leaf (+v), signs
// alternate upward; lane l of the 8-lane group updates the levels == l (mod 8)
// (at most kMaxDepth / 8 = 6 per lane).  The nodes of a path are distinct, so a
// lane loads all of its levels' records first and then stores them: one memory
// round trip, where a load-add-store per level (the compiler cannot reorder a
// level's load above the previous level's store) paid one per level.
constexpr int kLevelsPerLane = kMaxDepth / kLanesPerTree;
// (The loads are unconditional -- levels past d read the path's root, whose node
// exists -- so that no branch separates them: hipcc waits vmcnt(0) at each one.)
__device__ __forceinline__ void backup_load(const uint4 *nodes, const uint32_t (&node)[kLevelsPerLane], int d,
                                            int lane8, uint2 (&r)[kLevelsPerLane]) {
#pragma unroll
    for (int j = 0; j < kLevelsPerLane; ++j) r[j] = *(const uint2 *)(nodes + (lane8 + 8 * j <= d ? node[j] : node[0]));
}
__device__ __forceinline__ void backup_store(uint4 *nodes, const uint32_t (&node)[kLevelsPerLane], int d, float v,
                                             int lane8, const uint2 (&r)[kLevelsPerLane]) {
#pragma unroll
    for (int j = 0; j < kLevelsPerLane; ++j) {
        const int lvl = lane8 + 8 * j;
        if (lvl <= d) {
            const float sign = ((d - lvl) & 1) ? -1.0f : 1.0f;
            *(uint2 *)(nodes + node[j]) = make_uint2(r[j].x + 1u, __float_as_uint(__uint_as_float(r[j].y) + sign * v));
        }
    }
}
__device__ __forceinline__ void backup_nodes(uint4 *nodes, const uint32_t (&node)[kLevelsPerLane], int d, float v,
                                             int lane8) {
    uint2 r[kLevelsPerLane];
    backup_load(nodes, node, d, lane8, r);
    backup_store(nodes, node, d, v, lane8, r);
}

// this lane's bit of its tree's 8-lane group in a wave-wide ballot
__device__ __forceinline__ uint32_t group_bits(uint64_t ball) {
    return (uint32_t)(ball >> (threadIdx.x & 63 & ~(kLanesPerTree - 1))) & 0xFFu;
}

// has_line without the early exits (no branch on the descent's chain)
__device__ __forceinline__ bool has_line_flat(uint64_t b) {
    const uint64_t h = b & (b >> 7), v = b & (b >> 1), g = b & (b >> 8);
    return ((h & (h >> 14)) | (v & (v >> 2)) | (g & (g >> 16))) != 0ull;
}

// A non-NaN score as an unsigned key in the same order, -0 and +0 equal (the
// reference compares f32 with partial_cmp, where they tie).
__device__ __forceinline__ uint32_t score_key(float u) {
    const uint32_t b = __float_as_uint(u + 0.0f);   // -0 + 0 = +0 (not folded: signed zeros are kept)
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// a tree's best child so far in the argmax over its 8 lanes: the 64-bit key
// (score, then column: ties go to the last child, i.e. the highest column) with
// the child index in the key's low bits, and the child record's visit count and
// children word (what the next level needs)
struct Cand {
    uint32_t hi, lo, n, w;
};
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
// one butterfly step: take the partner lane's candidate if its key is larger
template <int CTRL>
__device__ __forceinline__ void cand_step(Cand &c) {
    const Cand o{dpp_mov<CTRL>(c.hi), dpp_mov<CTRL>(c.lo), dpp_mov<CTRL>(c.n), dpp_mov<CTRL>(c.w)};
    const bool take = (((uint64_t)o.hi << 32) | o.lo) > (((uint64_t)c.hi << 32) | c.lo);
    c.hi = take ? o.hi : c.hi;
    c.lo = take ? o.lo : c.lo;
    c.n = take ? o.n : c.n;
    c.w = take ? o.w : c.w;
}

// a tree's root for this search call: node id and position (constant while it
// runs), and its record's visit count and children word, kept current in
// registers (each iteration's backup adds one visit; an expansion of the root
// sets its children), so a descent starts without reloading it
struct RootInfo {
    uint32_t node;
    uint64_t x, o;
    uint8_t n, status;
    uint32_t rn, rw;
};
__device__ __forceinline__ RootInfo load_root(const TreeView &T, uint32_t t) {
    const uint32_t node = T.root[t];
    const uint4 r = T.nodes[(size_t)t * T.cap + node];
    return RootInfo{node, T.root_x[t], T.root_o[t], T.root_n[t], T.root_status[t], r.x, r.w};
}

// One PUCT descent of tree t (mcts.rs:235-250) by its 8 lanes.  A terminal leaf
// is backed up in place (mcts.rs:245-247) and kTerminal returned; a live leaf is
// returned as kLive with its position in (x, o, n) and its path recorded (T.path,
// T.depth); kError after a NaN UCB or an over-deep path (flag set in err).
//
// Lane c of the tree's 8 stands for board column c: a node's children are its
// position's open columns in ascending order (expand_leaf), so column c's child
// is number popcount(open columns below c).  Per level: one 16-B record load,
// the UCB, and the argmax with ties to the LAST child (Iterator::max_by,
// mcts.rs:110-113) as a butterfly of DPP moves over the 8 lanes on a 64-bit key
// (score, column), carrying the child index, visit count and children word --
// no lane shuffle through the LDS crossbar and no branch on the chain.
enum Descent { kTerminal = 0, kLive = 1, kError = 2 };
__device__ __forceinline__ Descent descend(const TreeView &T, uint32_t t, const RootInfo &root, int lane8, float c,
                                           uint32_t *err, uint64_t &x, uint64_t &o, uint8_t &n) {
    uint4 *nodes = T.nodes + (size_t)t * T.cap;
    uint32_t *path = T.path + (size_t)t * kMaxDepth;
    uint32_t node = root.node;
    x = root.x;
    o = root.o;
    n = root.n;
    uint8_t status = root.status;
    uint32_t rn = root.rn, rw = root.rw;   // the current node's visit count and children word
    // path levels == lane8 (mod 8) kept in this lane's registers (kMaxDepth = 6 x 8)
    uint32_t pr[kLevelsPerLane] = {node, 0u, 0u, 0u, 0u, 0u};
    const int top = 7 * lane8 + 5;   // this column's top cell (lane 7: none)
    int d = 0;
    if (lane8 == 0) path[0] = node;
    while (rw != kNoChildren) {                             // while node.is_fully_expanded()
        const uint32_t first = rw & 0xFFFFFFu;
        const uint64_t occ = x | o;
        const bool open = lane8 < c4::kActions && !((occ >> top) & 1ull);
        const uint32_t k = c4::popc32(group_bits(__ballot(open)) & ((1u << lane8) - 1u));
        const uint4 ch = nodes[first + (open ? k : 0u)];
        const float sq = sqrtf((float)rn);
        const float u = ucb(sq, ch, c);
        Cand w{open ? score_key(u) : 0u, ((uint32_t)lane8 << 3) | k, ch.x, ch.w};
        cand_step<0xB1>(w);    // quad_perm [1,0,3,2]: lane ^ 1
        cand_step<0x4E>(w);    // quad_perm [2,3,0,1]: lane ^ 2
        cand_step<0x141>(w);   // row_half_mirror: lane i <-> 7 - i of the 8, across the two quads
        // a NaN on ANY child panics in the reference (partial_cmp().unwrap(),
        // mcts.rs:106-109): OR over the tree's 8 lanes and stop the whole group,
        // so lanes never split onto different children.  Tested after the argmax
        // (whose result is then dropped): before it, the branch made the compiler
        // split the record load and sink the children word's half past it.
        if (group_bits(__ballot(open && u != u))) {
            if (lane8 == 0) atomicOr(err, kErrNan);
            return kError;
        }
        rn = w.n;
        rw = w.w;
        // replay the child's action on the bitboards
        const int a = (int)(w.lo >> 3);
        const uint64_t bit = c4::drop_bit(occ, a);
        const bool xm = c4::x_to_move(n);
        x = xm ? x | bit : x;
        o = xm ? o : o | bit;
        n = (uint8_t)(n + 1);
        status = has_line_flat(xm ? x : o) ? c4::kWon : (n == c4::kCells ? c4::kTied : c4::kOngoing);
        node = first + (w.lo & 7u);
        ++d;
        if (d >= kMaxDepth) {
            if (lane8 == 0) atomicOr(err, kErrDepth);
            return kError;
        }
        const bool mine = (d & 7) == lane8;
        if (mine) path[d] = node;
#pragma unroll
        for (int j = 0; j < kLevelsPerLane; ++j) pr[j] = mine && (d >> 3) == j ? node : pr[j];
    }
    if (lane8 == 0) T.depth[t] = (uint8_t)d;
    if (status != c4::kOngoing) {                           // terminal leaf: backprop(leaf, value), mcts.rs:245-247
        backup_nodes(nodes, pr, d, c4::terminal_value(status), lane8);
        return kTerminal;
    }
    return kLive;
}

// The position's two candidate buckets: the high and the low half of one hash, and
// first ^ 1 where the halves agree.  A one-bucket table has a single candidate
// (b1 == b0).
struct CacheBuckets {
    uint32_t b0, b1;
};
__device__ __forceinline__ CacheBuckets cache_buckets(const CacheView &C, uint64_t mine, uint64_t theirs) {
    const uint64_t h = c4::splitmix64(mine ^ (theirs * 0x9E3779B97F4A7C15ull));
    const uint32_t b0 = (uint32_t)(h >> 32) & C.mask, b1 = (uint32_t)h & C.mask;
    return CacheBuckets{b0, b1 == b0 ? (b0 ^ 1u) & C.mask : b1};
}
__device__ __forceinline__ uint4 *cache_way(const CacheView &C, uint32_t bucket, int way) {
    return C.tab + ((size_t)bucket * EvalCache::kWays + (uint32_t)way) * 4;
}

// what cache_claim found
enum Claim { kClaimFull, kClaimDone, kClaimSame };
// lane 0's part of an insert into one bucket: claim, by compare-and-swap from 0, the
// first way that is still empty, starting at the first one the tree's lanes saw empty
// (`empty`, none: the bucket is full) and going on to the next when another writer got
// there first; then write the entry.  A way that holds this position's word 0 by now
// ends it (kClaimSame).
__device__ __forceinline__ Claim cache_claim(uint4 *bucket, uint32_t empty, uint64_t k0, uint64_t k1, const uint4 &e1,
                                             const uint4 &e2, uint32_t seq) {
    for (int w = empty ? __ffs(empty) - 1 : (int)EvalCache::kWays; w < (int)EvalCache::kWays; ++w) {
        uint4 *e = bucket + 4 * w;
        const unsigned long long old = atomicCAS((unsigned long long *)e, 0ull, (unsigned long long)k0);
        if (old == 0ull) {
            ((uint64_t *)e)[1] = k1;
            e[1] = e1;
            e[2] = e2;
            *(uint32_t *)(e + 3) = seq;   // born (4 bytes: the hit stamp beside it may be a reader's already)
            return kClaimDone;
        }
        if (old == k0) return kClaimSame;
    }
    return kClaimFull;
}

// Insert the evaluated leaf in slot s of batch B, by its tree's 8 lanes: each
// reads one way's claim word in both of the position's buckets; a way that
// already holds this position's word 0 ends it (the same position, or one that
// shares `mine` in these buckets: only an insert is lost); else lane 0 claims the
// first empty way of the bucket with more empty ways (ties: the first bucket),
// and when other writers have filled that bucket in the meantime, of the other
// one.  Both buckets full drops the insert.  No entry is ever overwritten.
// Returns true in lane 0 when an entry was claimed.
__device__ __forceinline__ bool cache_insert(const CacheView &C, const BatchView &B, uint32_t s, int lane8) {
    const uint64_t mine = B.mine[s], theirs = B.theirs[s];
    const uint64_t gen = (uint64_t)C.gen << kGenShift;
    const uint64_t k0 = mine | gen, k1 = theirs | gen;
    const CacheBuckets cb = cache_buckets(C, mine, theirs);
    uint4 *bk0 = cache_way(C, cb.b0, 0), *bk1 = cache_way(C, cb.b1, 0);
    const uint64_t seen0 = *(const uint64_t *)(bk0 + 4 * lane8);
    const uint64_t seen1 = *(const uint64_t *)(bk1 + 4 * lane8);
    const float4 pa = *(const float4 *)(B.priors + (size_t)s * kPriorStride);
    const float4 pb = *(const float4 *)(B.priors + (size_t)s * kPriorStride + 4);
    const float value = B.value[s];
    const uint32_t same = group_bits(__ballot(seen0 == k0 || seen1 == k0));
    const uint32_t empty0 = group_bits(__ballot(seen0 == 0ull));
    const uint32_t empty1 = cb.b1 != cb.b0 ? group_bits(__ballot(seen1 == 0ull)) : 0u;
    if (same || lane8 != 0) return false;
    const uint32_t p0 = __float_as_uint(pa.x), p2 = __float_as_uint(pa.z), p4 = __float_as_uint(pb.x),
                   p6 = __float_as_uint(pb.z);
    if (((p0 | p2 | p4 | p6) & kPriorMark) != 0u) return false;   // (a marked prior cannot be stored)
    const uint4 e1 = make_uint4(p0 | kPriorMark, __float_as_uint(pa.y), p2 | kPriorMark, __float_as_uint(pa.w));
    const uint4 e2 = make_uint4(p4 | kPriorMark, __float_as_uint(pb.y), p6 | kPriorMark, __float_as_uint(value));
    const bool second = c4::popc32(empty1) > c4::popc32(empty0);
    Claim r = cache_claim(second ? bk1 : bk0, second ? empty1 : empty0, k0, k1, e1, e2, C.seq);
    if (r == kClaimFull && cb.b1 != cb.b0)
        r = cache_claim(second ? bk0 : bk1, second ? empty0 : empty1, k0, k1, e1, e2, C.seq);
    if (r == kClaimFull) atomicAdd(C.ctr + 1, 1u);
    return r == kClaimDone;
}
// the fill counter, one atomic per wave: the wave's claims (lane 0 of each tree's group)
__device__ __forceinline__ void cache_count(const CacheView &C, bool claimed) {
    const uint64_t b = __ballot(claimed);
    if (b && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)__ballot(true)) - 1u)
        atomicAdd(C.ctr, (uint32_t)c4::popc64(b));
}

// the acceptance test of a lookup: both key words are the position's at this
// generation, and all four payload marks are there (the entry is complete)
__device__ __forceinline__ bool cache_holds(const uint4 &q0, const uint4 &q1, const uint4 &q2, uint64_t k0, uint64_t k1) {
    return (((uint64_t)q0.y << 32) | q0.x) == k0 && (((uint64_t)q0.w << 32) | q0.z) == k1 &&
           (q1.x & q1.z & q2.x & q2.z & kPriorMark) != 0u;
}

// live leaf -> batch slot (mcts.rs:249-250).  With the evaluation cache, the
// tree's 8 lanes first read the 8 ways of the position's two buckets (one round
// trip): when a way holds the position, complete, the leaf is served from it
// -- a slot from the top of the batch (cap - 1 downwards, counted in B.hits),
// with the position, priors and value the forward would have written there --
// and the forward never sees it.  A chain's leaves of one iteration, hits and
// misses together, are at most its trees (<= cap), so the two regions never meet.
__device__ __forceinline__ void slot_leaf(const TreeView &T, const BatchView &B, const CacheView &C, uint32_t t,
                                          int lane8, uint64_t x, uint64_t o, uint8_t n) {
    const bool xm = c4::x_to_move(n);
    const uint64_t mine = xm ? x : o, theirs = xm ? o : x;
    if (lane8 == 0)
        __hip_atomic_fetch_add(T.evals + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // result unused: no wait
    if (C.tab) {
        // both buckets' loads go out together: one round trip, as with one bucket
        const CacheBuckets cb = cache_buckets(C, mine, theirs);
        const uint4 *ea = cache_way(C, cb.b0, lane8), *eb = cache_way(C, cb.b1, lane8);
        const uint4 a0 = ea[0], a1 = ea[1], a2 = ea[2], b0 = eb[0], b1 = eb[1], b2 = eb[2];
        const uint64_t gen = (uint64_t)C.gen << kGenShift;
        const uint64_t k0 = mine | gen, k1 = theirs | gen;
        const bool match_a = cache_holds(a0, a1, a2, k0, k1), match_b = cache_holds(b0, b1, b2, k0, k1);
        const bool match = match_a || match_b;
        const uint4 q1 = match_a ? a1 : b1, q2 = match_a ? a2 : b2;
        const uint32_t hit = group_bits(__ballot(match));
        if (hit) {
            // lane 0 takes the slot and records it (T.slot is lane 0's word: select_tree's
            // kNoSlot store came from it too); the lane that holds the entry gets the slot
            // from it and writes the payload
            uint32_t slot = 0;
            if (lane8 == 0) {
                slot = B.cap - 1u - atomicAdd(B.hits, 1u);
                T.slot[t] = slot | kHitSlot;
                B.tree[slot] = t;
                B.mine[slot] = mine;
                B.theirs[slot] = theirs;
            }
            slot = (uint32_t)__shfl((int)slot, 0, kLanesPerTree);
            if (lane8 == __ffs(hit) - 1) {
                float4 *pr = (float4 *)(B.priors + (size_t)slot * kPriorStride);
                pr[0] = make_float4(__uint_as_float(q1.x & ~kPriorMark), __uint_as_float(q1.y),
                                    __uint_as_float(q1.z & ~kPriorMark), __uint_as_float(q1.w));
                pr[1] = make_float4(__uint_as_float(q2.x & ~kPriorMark), __uint_as_float(q2.y),
                                    __uint_as_float(q2.z & ~kPriorMark), 0.f);
                B.value[slot] = __uint_as_float(q2.w);
                // the entry's hit stamp: a plain store, nothing waits for it
                ((uint32_t *)((match_a ? ea : eb) + 3))[1] = C.seq;
            }
            return;
        }
    }
    if (lane8 == 0) {
        const uint32_t slot = atomicAdd(B.count, 1u);
        T.slot[t] = slot;
        B.tree[slot] = t;
        B.mine[slot] = mine;
        B.theirs[slot] = theirs;
    }
}

// One search iteration's selection for tree t: a live leaf gets a slot in batch
// B (recorded in T.slot[t]), a terminal leaf is backed up in place.
//
// RUN_ON (tail mode, search()): the tree runs its remaining iterations (T.left)
// in this launch for as long as they end on terminal leaves -- each is backed
// up, then the next descent starts -- and stops at the first live leaf, which
// goes to the batch, or after run_cap descents (B.more set: the next pass goes
// on).  The tree's iterations keep the reference's order (select, backprop,
// select, ...), so the results equal one descent per launch.  The cap keeps a
// pass from lasting a solved tree's whole run while a tree that still evaluates
// waits for the next one.
template <bool RUN_ON>
__device__ __forceinline__ void select_tree(const TreeView &T, const BatchView &B, const CacheView &C, uint32_t t,
                                            RootInfo &root, int lane8, float c, uint32_t *err, uint32_t run_cap) {
    if (lane8 == 0) T.slot[t] = kNoSlot;
    uint64_t x, o;
    uint8_t n;
    if (!RUN_ON) {
        if (descend(T, t, root, lane8, c, err, x, o, n) == kLive) slot_leaf(T, B, C, t, lane8, x, o, n);
        return;
    }
    uint32_t left = T.left[t];
    for (uint32_t run = 0; left > 0; ++run) {
        if (run == run_cap) {
            if (lane8 == 0) atomicOr(B.more, 1u);
            break;
        }
        --left;
        const Descent r = descend(T, t, root, lane8, c, err, x, o, n);
        if (r == kLive) slot_leaf(T, B, C, t, lane8, x, o, n);
        if (r != kTerminal) break;
        root.rn += 1;   // the backup's visit of the root
        // the next descent reads records the other lanes of this tree just backed
        // up: one wave, so a wavefront-scope fence (as in k_expand_select)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (lane8 == 0) T.left[t] = left;
}

// What an expansion needs of the tree itself (not of its leaf): loaded with the
// tree's slot, before the slot is known to hold a leaf.
struct LeafPath {
    int d;                                 // the leaf's depth
    uint32_t lv[kLevelsPerLane];           // this lane's path levels (stale past the depth)
    uint32_t first;                        // the arena fill: the new children's first id
};
__device__ __forceinline__ LeafPath load_leaf_path(const TreeView &T, uint32_t t, int lane8) {
    LeafPath L;
    const uint32_t *path = T.path + (size_t)t * kMaxDepth;
    L.d = T.depth[t];
#pragma unroll
    for (int j = 0; j < kLevelsPerLane; ++j) L.lv[j] = path[lane8 + 8 * j];
    L.first = T.next_free[t];
    return L;
}

// expand leaf slot s of batch B (mcts.rs:116-143) and back its value up (:145-159).
// One memory round trip after the slot: the leaf's position, this lane's prior
// and the value, together with the records of the path levels this lane backs up
// (the new children are past the arena fill, never on the path); then only
// stores.  The leaf is path[d], which lane d & 7 holds.  The root's visit count
// and children word in `root` are brought up to date.
__device__ __forceinline__ void expand_leaf(const TreeView &T, const BatchView &B, uint32_t t, uint32_t s, int lane8,
                                            uint32_t *err, const LeafPath &L, RootInfo &root) {
    uint4 *nodes = T.nodes + (size_t)t * T.cap;
    const int d = L.d;
    uint32_t node[kLevelsPerLane];   // this lane's levels of the path; 0 (a valid dummy) past the depth
#pragma unroll
    for (int j = 0; j < kLevelsPerLane; ++j) node[j] = lane8 + 8 * j <= d ? L.lv[j] : 0u;
    const uint64_t occ = B.mine[s] | B.theirs[s];
    const float prior = B.priors[(size_t)s * kPriorStride + lane8];   // lane 7: the stride's padding
    const float value = B.value[s];
    uint2 r[kLevelsPerLane];
    backup_load(nodes, node, d, lane8, r);
    // legal actions of the (live) leaf; children in ascending action order (mcts.rs:116-143)
    const bool legal = lane8 < c4::kActions && !((occ >> (7 * lane8 + 5)) & 1ull);
    const uint32_t grp = group_bits(__ballot(legal));
    const uint32_t nch = c4::popc32(grp);
    const uint32_t idx = c4::popc32(grp & ((1u << lane8) - 1u));
    const uint32_t first = L.first;
    if (first + nch > T.cap) {
        if (lane8 == 0) atomicOr(err, kErrCapacity);
        return;
    }
    if (legal) nodes[first + idx] = make_uint4(0u, 0u, __float_as_uint(prior), kNoChildren);
    if (lane8 == 0) T.next_free[t] = first + nch;
    if (lane8 == (d & 7)) {
        uint32_t leaf = node[0];
#pragma unroll
        for (int j = 1; j < kLevelsPerLane; ++j) leaf = (d >> 3) == j ? node[j] : leaf;
        nodes[leaf].w = first | (nch << 24);
    }
    backup_store(nodes, node, d, value, lane8, r);
    root.rn += 1;
    if (d == 0) root.rw = first | (nch << 24);
}

template <bool RUN_ON>
__global__ __launch_bounds__(kBlock) void k_select(TreeView T, BatchView B, CacheView C,
                                                   const uint32_t *__restrict__ active, uint32_t n_active, float c,
                                                   uint32_t *err, uint32_t run_cap) {
    const uint32_t gi = (blockIdx.x * blockDim.x + threadIdx.x) / kLanesPerTree;
    if (gi >= n_active) return;
    const uint32_t t = active[gi];
    RootInfo root = load_root(T, t);
    select_tree<RUN_ON>(T, B, C, t, root, threadIdx.x & (kLanesPerTree - 1), c, err, run_cap);
}

// expand this iteration's leaf of every tree (batch `cur`), then select the next
// iteration's leaf into batch `nxt`.  A tree's lanes are one group of 8 in one
// wave, so its expand stores are seen by its own select loads in program order:
// a wavefront-scope fence (no instruction; it keeps the compiler from moving the
// loads above the stores), not a workgroup-scope one (s_waitcnt vmcnt(0): a
// store round trip on every iteration's critical path).
template <bool RUN_ON>
__global__ __launch_bounds__(kBlock) void k_expand_select(TreeView T, BatchView cur, BatchView nxt, CacheView C,
                                                          const uint32_t *__restrict__ active, uint32_t n_active,
                                                          float c, uint32_t *err, uint32_t run_cap) {
    const uint32_t gi = (blockIdx.x * blockDim.x + threadIdx.x) / kLanesPerTree;
    if (gi >= n_active) return;
    const int lane8 = threadIdx.x & (kLanesPerTree - 1);
    const uint32_t t = active[gi];
    const uint32_t s = T.slot[t];
    RootInfo root = load_root(T, t);                      // loaded with the slot, off the chain
    const LeafPath L = load_leaf_path(T, t, lane8);       // likewise (unused when the tree has no leaf)
    // the root's and the path's loads retire here: used first (or, with no leaf,
    // never) after the expansion's branch, whose join would otherwise make the
    // compiler wait for the expansion's stores too (in-order vmcnt, merged
    // conservatively over both paths)
    asm volatile("" ::"v"(root.rn), "v"(root.rw), "v"((uint32_t)root.x), "v"((uint32_t)(root.x >> 32)),
                 "v"((uint32_t)root.o), "v"((uint32_t)(root.o >> 32)), "v"((uint32_t)root.n), "v"((uint32_t)root.status));
    asm volatile("" ::"v"(L.d), "v"(L.first), "v"(L.lv[0]), "v"(L.lv[1]), "v"(L.lv[2]), "v"(L.lv[3]), "v"(L.lv[4]),
                 "v"(L.lv[5]));
    if (s != kNoSlot) expand_leaf(T, cur, t, s & ~kHitSlot, lane8, err, L, root);
    // the select reads records this tree's lanes just wrote: lanes of one wave,
    // whose memory operations are performed in order (no wait for the stores)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    select_tree<RUN_ON>(T, nxt, C, t, root, lane8, c, err, run_cap);
    // off the chain, after the select: the leaf the forward evaluated for this tree
    // goes into the cache (a leaf served from it is there already)
    if (C.tab) {
        const bool claimed = s != kNoSlot && !(s & kHitSlot) && cache_insert(C, cur, s, lane8);
        cache_count(C, claimed);
    }
}

// tail mode: every active tree has all `iters` iterations of this search call ahead
__global__ void k_set_left(TreeView T, const uint32_t *__restrict__ active, uint32_t n, uint32_t iters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) T.left[active[i]] = iters;
}

// Dirichlet root noise (dirichlet.h), once per tree per search call, one wave per active
// tree: the prior word of every root child becomes (1 - eps) * P + eps * eta, eta drawn
// under the tree's key (gid[t], move[t]); lanes < n_children write, no other field and no
// other node is written, no renormalisation.  Launched twice per call.  entry = 1 (after the
// call's setup, before its first selection): the trees whose root has children are mixed, and
// done[t] records for every active tree whether it was.  entry = 0 (behind the unfused
// k_expand of iteration 0, before the first selection at a root it expanded): the trees not
// mixed yet whose root has children now.  A root that stays without children is never mixed.
constexpr int kNoiseWaves = 4;   // waves (trees) per workgroup of the two noise kernels
__global__ __launch_bounds__(64 * kNoiseWaves) void k_root_noise(TreeView T, const uint32_t *__restrict__ active,
                                                                uint32_t n_active,
                                                                const uint64_t *__restrict__ gid,
                                                                const uint32_t *__restrict__ move, uint32_t *done,
                                                                int entry, uint64_t seed, float alpha,
                                                                float one_minus_eps, float eps) {
    const int lane = threadIdx.x & 63;
    const uint32_t gi = blockIdx.x * kNoiseWaves + (threadIdx.x >> 6);
    if (gi >= n_active) return;            // (per wave: every lane of a wave that goes on reaches the draw)
    const uint32_t t = active[gi];
    if (!entry && done[t]) return;
    uint4 *nodes = T.nodes + (size_t)t * T.cap;
    const uint32_t w = nodes[T.root[t]].w;
    const uint32_t nch = w == kNoChildren ? 0u : w >> 24, first = w & 0xFFFFFFu;
    if (nch == 0 || nch > (uint32_t)c4::kActions || first + nch > T.cap) {
        if (entry && lane == 0) done[t] = 0;
        return;
    }
    float eta[4];
    wave_dirichlet(seed, gid[t], move[t], nch, alpha, lane, eta);
    if ((uint32_t)lane < nch) {
        uint32_t *rec = (uint32_t *)(nodes + first + lane);
        rec[2] = __float_as_uint(dirichlet_mix(__uint_as_float(rec[2]), eta[0], one_minus_eps, eps));
    }
    if (lane == 0) done[t] = 1;
}

// spai_root_noise: the draws themselves, one wave per key; eta [count][7], zero past n[i]
__global__ __launch_bounds__(64 * kNoiseWaves) void k_noise_draws(uint32_t count, const uint64_t *__restrict__ gid,
                                                                 const uint32_t *__restrict__ move,
                                                                 const uint32_t *__restrict__ n, uint64_t seed,
                                                                 float alpha, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * kNoiseWaves + (threadIdx.x >> 6);
    if (i >= count) return;
    float eta[4];
    wave_dirichlet(seed, gid[i], move[i], n[i], alpha, lane, eta);
    if (lane < c4::kActions) out[(size_t)i * c4::kActions + lane] = eta[0];
}

// a keyed search's keys [n], parallel to `active`, into the per-tree key arrays
__global__ void k_noise_keys(const uint32_t *__restrict__ active, uint32_t n, const uint64_t *__restrict__ gid,
                             const uint32_t *__restrict__ move, uint64_t *__restrict__ tree_gid,
                             uint32_t *__restrict__ tree_move) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tree_gid[active[i]] = gid[i];
    tree_move[active[i]] = move[i];
}

__global__ __launch_bounds__(kBlock) void k_eval_stub(BatchView B, uint32_t max_n, int kind) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= max_n || s >= *B.count) return;
    // hash evaluator keys on absolute X/O stones: recover them from the player-to-move view
    const uint32_t n = (uint32_t)c4::popc64(B.mine[s] | B.theirs[s]);
    const bool xm = (n & 1u) == 0;
    const uint64_t x = xm ? B.mine[s] : B.theirs[s], o = xm ? B.theirs[s] : B.mine[s];
    float pr[c4::kActions], v;
    c4::stub_eval(kind, x, o, (uint8_t)n, pr, &v);
    for (int a = 0; a < c4::kActions; ++a) B.priors[(size_t)s * kPriorStride + a] = pr[a];
    B.value[s] = v;
}

// the last iteration's expansion, per leaf: the forwarded leaves in slots [0, count),
// then those served from the evaluation cache in slots cap - 1 downwards
__global__ __launch_bounds__(kBlock) void k_expand(TreeView T, BatchView B, CacheView C, uint32_t max_n,
                                                   uint32_t *err) {
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / kLanesPerTree;
    if (i >= max_n) return;
    const uint32_t count = *B.count, hits = B.hits ? *B.hits : 0u;
    if (i >= count + hits) return;
    const bool fwd = i < count;
    const uint32_t s = fwd ? i : B.cap - 1u - (i - count);
    const int lane8 = threadIdx.x & (kLanesPerTree - 1);
    const uint32_t t = B.tree[s];
    RootInfo root{};   // (the root's record is not needed after the last expansion)
    expand_leaf(T, B, t, s, lane8, err, load_leaf_path(T, t, lane8), root);
    if (C.tab) {
        const bool claimed = fwd && cache_insert(C, B, s, lane8);
        cache_count(C, claimed);
    }
}

// per active tree: [0] = root first|nch<<24 (children word), [1..7] child visit counts;
// max_evals[0]: the most live leaves one tree evaluated in this search call, [1]: their sum over the trees
__global__ void k_root_stats(TreeView T, const uint32_t *__restrict__ active, uint32_t n_active, uint32_t *out,
                             uint32_t *max_evals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_active) return;
    const uint32_t t = active[i];
    atomicMax(max_evals, T.evals[t]);
    atomicAdd(max_evals + 1, T.evals[t]);
    const uint4 *nodes = T.nodes + (size_t)t * T.cap;
    const uint4 r = nodes[T.root[t]];
    out[i * 8] = r.w;
    const uint32_t nch = r.w == kNoChildren ? 0 : r.w >> 24, first = r.w & 0xFFFFFFu;
    for (uint32_t k = 0; k < 7; ++k) out[i * 8 + 1 + k] = k < nch ? nodes[first + k].x : 0u;
}

__global__ void k_trees_init(TreeView T, RootsOut R, uint32_t first_tree, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tree_clear(T, R, first_tree + i);
}

// ---------------------------------------------------------------- thinning
// Between search calls (no search kernel runs: cache_thin), a table past its fill
// threshold is thinned, not emptied: the entries that earned their place stay, at
// the same generation, and the others are zeroed whole, which leaves their ways
// empty for cache_claim.  An entry's class is whether a lookup ever accepted it
// (hit stamp non-zero), its age the search calls since its latest stamp (the hit
// stamp, else the born stamp), at most kAges - 1.
//
// Both passes are grid-stride over the table's 16-B quarters, four lanes per
// entry (lanes 4k .. 4k + 3 of a wave: coalesced), the claim words taken from
// the first lane of the four and the stamps from the last.
struct ThinEntry {
    bool live;      // claimed (between search calls: complete)
    uint32_t cls;   // 0 never hit, 1 hit
    uint32_t age;
};
__device__ __forceinline__ ThinEntry thin_entry(const uint4 &q, uint32_t now) {
    const uint32_t c0 = (uint32_t)__shfl((int)q.x, 0, 4), c1 = (uint32_t)__shfl((int)q.y, 0, 4);
    const uint32_t born = (uint32_t)__shfl((int)q.x, 3, 4), hit = (uint32_t)__shfl((int)q.y, 3, 4);
    const uint32_t age = now - (hit ? hit : born);
    return ThinEntry{(c0 | c1) != 0u, hit ? 1u : 0u, age < EvalCache::kAges - 1 ? age : EvalCache::kAges - 1};
}

// pass 1: hist[cls * kAges + age] += the live entries of that bin (workgroup bins in
// LDS, one global atomic per non-empty bin)
__global__ __launch_bounds__(256) void k_thin_count(const uint4 *__restrict__ tab, size_t quarters, uint32_t now,
                                                    uint32_t *hist) {
    __shared__ uint32_t bins[2 * EvalCache::kAges];
    for (uint32_t b = threadIdx.x; b < 2 * EvalCache::kAges; b += blockDim.x) bins[b] = 0u;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < quarters; i += stride) {
        const ThinEntry te = thin_entry(tab[i], now);
        if ((i & 3) == 0 && te.live) atomicAdd(&bins[te.cls * EvalCache::kAges + te.age], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < 2 * EvalCache::kAges; b += blockDim.x)
        if (bins[b]) atomicAdd(hist + b, bins[b]);
}

// pass 2: zero every live entry whose age is at or past its class's cutoff
// (cut[cls]: 0 drops the class, kAges keeps it), and add the survivors to *live
// (zeroed before the launch), one atomic per wave
__global__ __launch_bounds__(256) void k_thin_sweep(uint4 *__restrict__ tab, size_t quarters, uint32_t now,
                                                    uint32_t cut_fresh, uint32_t cut_hit, uint32_t *live) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint32_t kept = 0;   // of this wave (the same in all its lanes that ran the iteration)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < quarters; i += stride) {
        const ThinEntry te = thin_entry(tab[i], now);
        const bool drop = te.live && te.age >= (te.cls ? cut_hit : cut_fresh);
        if (drop) tab[i] = make_uint4(0u, 0u, 0u, 0u);
        kept += (uint32_t)c4::popc64(__ballot((i & 3) == 0 && te.live && !drop));
    }
    // (the table is a multiple of 32 quarters: a wave's lanes run the same iterations
    // but for the lanes past the end of a one-bucket table; lane 0 runs them all)
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(live, kept);
}
}  // namespace

TreeView tree_view(spai_engine *e) {
    Trees &T = e->trees;
    return TreeView{T.nodes.p, T.cap, T.root.p, T.next_free.p, T.root_x.p, T.root_o.p, T.root_n.p, T.root_status.p,
                    T.path.p, T.depth.p, T.slot.p, T.left.p, T.evals.p};
}

// chain `chain`'s leaf batch of search iteration `it`: buffers by parity, counter per iteration
// (cached: the chain looks its leaves up in the evaluation cache)
static BatchView batch_view(spai_engine *e, int chain, uint32_t it, bool cached) {
    Batch &B = e->batch[chain];
    const size_t h = (size_t)(it & 1u) * B.cap;
    return BatchView{B.iter_counts.p + it, B.iter_more.p ? B.iter_more.p + it : nullptr, B.tree.p + h, B.mine.p + h, B.theirs.p + h,
                     B.priors.p + h * kPriorStride, B.value.p + h,
                     cached ? B.iter_hits.p + it : nullptr, B.cap};
}

CacheView cache_view(spai_engine *e) {
    EvalCache &C = e->cache;
    if (!C.buckets) return CacheView{nullptr, 0u, 0u, nullptr, 0u};
    return CacheView{C.table.p, C.buckets - 1u, C.gen, C.ctr.p, C.seq};
}

// Empty the table on the engine stream: every search call's chains are joined to it
// before the call returns and forked from it when the next one starts, so no search
// kernel runs while the memset does.  A new generation goes with every clear.
int cache_clear(spai_engine *e) {
    EvalCache &C = e->cache;
    if (!C.buckets) return SPAI_OK;
    uint32_t fill = 0;
    SPAI_HIP(hipMemcpyAsync(&fill, C.ctr.p, 4, hipMemcpyDeviceToHost, e->stream));
    SPAI_HIP(hipStreamSynchronize(e->stream));
    C.inserts_cleared += fill;
    SPAI_HIP(hipMemsetAsync(C.table.p, 0, C.table.n * sizeof(uint4), e->stream));
    SPAI_HIP(hipMemsetAsync(C.ctr.p, 0, 4, e->stream));
    C.gen = C.gen % 32767u + 1u;
    C.fill_seen = 0;
    C.clears += 1;
    return SPAI_OK;
}

// The ranking of a thinning (kernels: "thinning"): hit entries before never-hit
// ones, then younger before older, in whole bins of the histogram -- a bin that
// would cross its budget is dropped whole, so no more than `keep` entries stay.
// The hit class takes at most kHitShare of `keep` (its youngest bins); what it
// leaves of `keep`, at least the rest of the share, goes to the newest never-hit
// entries: on a table small against its traffic the hit entries alone exceed the
// budget, and without the guard no fresh entry would survive a thinning
// (scripts/eval_cache_hitrate.py, ThinTable).  cut[cls]: the first age dropped.
constexpr uint64_t kHitShareNum = 3, kHitShareDen = 4;
struct ThinCut {
    uint32_t cut[2];
    uint64_t kept[2], seen[2];
};
static ThinCut thin_cutoff(const uint32_t *hist, uint64_t keep) {
    ThinCut t{{0u, 0u}, {0, 0}, {0, 0}};
    for (uint32_t cls = 0; cls < 2; ++cls)
        for (uint32_t a = 0; a < EvalCache::kAges; ++a) t.seen[cls] += hist[cls * EvalCache::kAges + a];
    if (t.seen[0] + t.seen[1] <= keep) {   // nothing to evict
        t.cut[0] = t.cut[1] = EvalCache::kAges;
        t.kept[0] = t.seen[0];
        t.kept[1] = t.seen[1];
        return t;
    }
    for (int cls = 1; cls >= 0; --cls) {
        const uint64_t budget = cls ? keep * kHitShareNum / kHitShareDen : keep - t.kept[1];
        const uint32_t *h = hist + cls * EvalCache::kAges;
        while (t.cut[cls] < EvalCache::kAges && t.kept[cls] + h[t.cut[cls]] <= budget) t.kept[cls] += h[t.cut[cls]++];
    }
    return t;
}

// what a thinning at the fill threshold keeps: 1/2 of the capacity
// (SPAI_EVAL_CACHE_KEEP=<fraction> for A/B measurements)
uint64_t cache_keep_budget(const EvalCache &C) {
    const char *v = std::getenv("SPAI_EVAL_CACHE_KEEP");
    const double f = v ? std::min(1.0, std::max(0.0, std::atof(v))) : 0.5;
    return (uint64_t)((double)C.entries() * f);
}

// Thin the table to at most `keep` entries, on the engine stream like cache_clear
// (no search kernel runs meanwhile).  The generation stays: the survivors are
// served on.  ctr[0] becomes the survivors' count, so the fill threshold goes by
// live entries; `inserts` stays "entries ever claimed".  Ages count from the
// latest search call.  (SPAI_EVAL_CACHE_THIN_LOG=1: one line per thinning on stderr.)
int cache_thin(spai_engine *e, uint64_t keep) {
    EvalCache &C = e->cache;
    if (!C.buckets) return SPAI_OK;
    hipStream_t st = e->stream;
    const size_t quarters = C.table.n;
    int n_cu = 0;
    SPAI_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device));
    const uint32_t grid = (uint32_t)std::min<size_t>((quarters + 255) / 256, (size_t)std::max(1, n_cu) * 8);
    uint32_t *hist = C.ctr.p + 2;
    uint32_t h[2 * EvalCache::kAges];
    SPAI_HIP(hipMemsetAsync(hist, 0, sizeof(h), st));
    k_thin_count<<<grid, 256, 0, st>>>(C.table.p, quarters, C.seq, hist);
    SPAI_HIP(hipGetLastError());
    SPAI_HIP(hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    const ThinCut t = thin_cutoff(h, keep);
    const uint64_t seen = t.seen[0] + t.seen[1], kept = t.kept[0] + t.kept[1];
    if (kept == seen) return SPAI_OK;   // the table holds no more than `keep`: nothing evicted, not a thinning
    SPAI_HIP(hipMemsetAsync(C.ctr.p, 0, 4, st));
    k_thin_sweep<<<grid, 256, 0, st>>>(C.table.p, quarters, C.seq, t.cut[0], t.cut[1], C.ctr.p);
    SPAI_HIP(hipGetLastError());
    C.inserts_cleared += (double)(seen - kept);
    C.evicted += (double)(seen - kept);
    C.kept_hit = (double)t.kept[1];
    C.fill_seen = (uint32_t)kept;
    C.thins += 1;
    C.clears += 1;
    const char *log = std::getenv("SPAI_EVAL_CACHE_THIN_LOG");
    if (log && std::atoi(log))
        std::fprintf(stderr, "eval cache thin %.0f: call %u, keep %llu of %llu live: hit %llu kept %llu (age < %u), "
                             "never hit %llu kept %llu (age < %u)\n",
                     C.thins, C.seq, (unsigned long long)keep, (unsigned long long)seen, (unsigned long long)t.seen[1],
                     (unsigned long long)t.kept[1], t.cut[1], (unsigned long long)t.seen[0],
                     (unsigned long long)t.kept[0], t.cut[0]);
    return SPAI_OK;
}

// Resolve the capacity (spai_eval_cache_set_capacity, else SPAI_EVAL_CACHE=<entries>, else
// kEntriesPerTree per tree slot of max_trees, at most 1 / kDefaultDeviceShare of the device's
// memory; either way rounded down to a power of two of buckets) and allocate the table, on the first search
// call after a change; on for the net evaluator only.  The counters outlive a resize:
// the old table's claims are added to the host's total and the device count starts again.
// (for_net: a net evaluates in the coming call -- cfg.eval for search and self-play, either
// player of a match)
int cache_prepare(spai_engine *e, bool for_net) {
    EvalCache &C = e->cache;
    if (C.ready && C.for_net == for_net) return SPAI_OK;
    C.for_net = for_net;
    uint64_t want = 0;
    if (for_net) {
        const char *v = std::getenv("SPAI_EVAL_CACHE");
        if (C.user_set) want = C.requested;
        else if (v) want = std::strtoull(v, nullptr, 10);
        else {
            // (the total, not what is free now: the size does not depend on what else is allocated)
            size_t free_bytes = 0, total_bytes = 0;
            SPAI_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
            want = std::min<uint64_t>(EvalCache::kEntriesPerTree * std::max(1u, e->cfg.max_trees),
                                      total_bytes / EvalCache::kDefaultDeviceShare / EvalCache::kEntryBytes);
        }
    }
    uint32_t buckets = 0;
    if (want) {
        buckets = 1;
        while ((uint64_t)buckets * 2 * EvalCache::kWays <= want && buckets < (1u << 28)) buckets *= 2;
    }
    if (buckets != C.buckets) {
        SPAI_HIP(hipStreamSynchronize(e->stream));
        if (C.buckets) {   // the old table's claims leave with it
            uint32_t fill = 0;
            SPAI_HIP(hipMemcpy(&fill, C.ctr.p, 4, hipMemcpyDeviceToHost));
            C.inserts_cleared += fill;
        }
        C.buckets = 0;
        if (C.ctr.p) SPAI_HIP(hipMemsetAsync(C.ctr.p, 0, 4, e->stream));
        // the default size is a wish: where the device has no room for it the table is
        // halved until it fits, and below kMinDefaultBuckets the cache stays off (the
        // search does not need it).  A size the caller asked for fits or is an error.
        const bool by_default = !C.user_set && !std::getenv("SPAI_EVAL_CACHE");
        int rc = C.table.alloc((size_t)buckets * EvalCache::kWays * 4);
        while (rc != SPAI_OK && by_default) {
            (void)hipGetLastError();
            buckets = buckets / 2 >= EvalCache::kMinDefaultBuckets ? buckets / 2 : 0;
            rc = C.table.alloc((size_t)buckets * EvalCache::kWays * 4);
        }
        SPAI_TRY(rc);
        if (buckets) {
            if (!C.ctr.p) {
                SPAI_TRY(C.ctr.alloc(EvalCache::kCtrWords));
                SPAI_HIP(hipMemsetAsync(C.ctr.p, 0, 8, e->stream));
            }
            C.buckets = buckets;
            SPAI_TRY(cache_clear(e));   // (the claim counter is zero: nothing added to the host's total)
        }
    }
    C.ready = true;
    return SPAI_OK;
}

// Number of search chains for n trees: two halves when each half still fills
// a useful batch.  Late in a game most trees are solved and an iteration
// evaluates almost nothing; then the second chain only doubles the launches,
// so one chain is used when the previous search call averaged fewer than
// kMinChainLeaves leaves per iteration.  (SPAI_CHAINS=k forces up to k chains,
// for A/B measurements.)  The split never changes results: trees are independent.
constexpr double kMinChainLeaves = 64;
// Tail mode (select_tree RUN_ON): a search call runs as passes, one per live leaf
// of its busiest tree (and at least iterations / kTailRun), each lasting as long
// as its longest terminal run, at most kTailRun descents (~2.5 us each); the host
// checks for the end every kTailChunk passes.  So it pays when every tree needs
// few evaluations: it is chosen when in the previous search call no tree
// evaluated kTailTreeEvals leaves or more, or the call averaged fewer than
// kTailLeaves leaves per iteration.  (By the average alone, at 34 and
// 6.6 leaves per iteration -- moves 36 and 37 of a bench step, where some trees
// still evaluate most iterations -- it took 114 and 49 ms against ~25 and ~18 ms
// for one launch pair per iteration: profiles/r04/tail.)
constexpr double kTailLeaves = 0.05;
constexpr uint32_t kTailTreeEvals = 160;
constexpr uint32_t kTailRun = 128;   // terminal descents per tree and pass
static int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v ? std::atoi(v) : dflt;
}
// Mid-game policy (tuning knobs, off by default): when the previous search call
// averaged fewer than SPAI_MID_LEAVES leaves per iteration (but at least
// kMinChainLeaves), run SPAI_MID_CHAINS chains whose forwards are capped at
// SPAI_MID_GRID workgroups, so that small per-chain batches run as larger groups
// side by side on disjoint CUs instead of one after the other over all CUs.
struct ChainPolicy {
    int chains;
    uint32_t grid_cap;   // 0: no cap
};
static ChainPolicy chains_for(uint32_t n, double last_evals_per_iter) {
    static const int forced = std::max(0, std::min(spai_engine::kChains, env_int("SPAI_CHAINS", 0)));
    static const int mid_leaves = env_int("SPAI_MID_LEAVES", 0);
    static const int mid_chains = std::max(1, std::min(spai_engine::kChains, env_int("SPAI_MID_CHAINS", 2)));
    static const uint32_t mid_grid = (uint32_t)std::max(0, env_int("SPAI_MID_GRID", 0));
    static const double min_chain_leaves = env_int("SPAI_MIN_CHAIN_LEAVES", (int)kMinChainLeaves);   // A/B knob
    // A/B knob: one chain at or above this many leaves per iteration (a fresh set
    // of trees counts as one leaf per tree)
    static const int hi_leaves = env_int("SPAI_HI_LEAVES", 0);
    if (forced) return {std::max(1, std::min<int>(forced, (int)(n / 64))), 0u};
    if (hi_leaves > 0 && (last_evals_per_iter < 0 ? (double)n : last_evals_per_iter) >= hi_leaves) return {1, 0u};
    if (last_evals_per_iter >= 0 && last_evals_per_iter < min_chain_leaves) return {1, 0u};
    if (last_evals_per_iter >= 0 && last_evals_per_iter < mid_leaves)
        return {std::max(1, std::min<int>(mid_chains, (int)(n / 64))), mid_grid};
    return {std::max(1, std::min<int>(2, (int)(n / 64))), 0u};
}

// upload host root bookkeeping for trees [t0, t0+n)
static int upload_roots(spai_engine *e, uint32_t t0, uint32_t n) {
    Trees &T = e->trees;
    std::vector<uint64_t> x(n), o(n);
    std::vector<uint8_t> nn(n), st(n);
    for (uint32_t i = 0; i < n; ++i) {
        const c4::State &s = T.h_root_state[t0 + i];
        x[i] = s.x;
        o[i] = s.o;
        nn[i] = s.n;
        st[i] = s.status;
    }
    hipStream_t s = e->stream;
    SPAI_HIP(hipMemcpyAsync(T.root.p + t0, T.h_root.data() + t0, n * 4, hipMemcpyHostToDevice, s));
    SPAI_HIP(hipMemcpyAsync(T.root_x.p + t0, x.data(), n * 8, hipMemcpyHostToDevice, s));
    SPAI_HIP(hipMemcpyAsync(T.root_o.p + t0, o.data(), n * 8, hipMemcpyHostToDevice, s));
    SPAI_HIP(hipMemcpyAsync(T.root_n.p + t0, nn.data(), n, hipMemcpyHostToDevice, s));
    SPAI_HIP(hipMemcpyAsync(T.root_status.p + t0, st.data(), n, hipMemcpyHostToDevice, s));
    SPAI_HIP(hipStreamSynchronize(s));
    return SPAI_OK;
}

static int timer_record(spai_engine *e, int which, uint32_t iter, bool begin, hipStream_t st, int chain) {
    KernelTimer &K = e->timer;
    if (!K.enabled) return SPAI_OK;
    if (begin) {
        if (K.used + 2 > K.ev.size()) {
            for (int i = 0; i < 64; ++i) {
                hipEvent_t ev;
                SPAI_HIP(hipEventCreate(&ev));
                K.ev.push_back(ev);
            }
        }
        K.which.push_back(which);
        K.iter.push_back(iter);
        K.chain.push_back(chain);
        SPAI_HIP(hipEventRecord(K.ev[K.used], st));
    } else {
        SPAI_HIP(hipEventRecord(K.ev[K.used + 1], st));
        K.used += 2;
    }
    return SPAI_OK;
}

// fold the sampled event pairs of one search call into the totals
// ch_counts [chain][num_searches] leaves per iteration
static int timer_collect(spai_engine *e, const uint32_t *ch_counts, uint32_t num_searches, const Chain *chains) {
    KernelTimer &K = e->timer;
    if (!K.enabled) return SPAI_OK;
    for (size_t i = 0; i < K.which.size(); ++i) {
        float ms = 0;
        SPAI_HIP(hipEventElapsedTime(&ms, K.ev[2 * i], K.ev[2 * i + 1]));
        const int w = K.which[i], h = K.chain[i];
        K.total_ms[w] += ms;
        K.launches[w] += 1;
        K.items[w] += w == 0 ? chains[h].cnt : ch_counts[(size_t)h * num_searches + K.iter[i]];
    }
    K.used = 0;
    K.which.clear();
    K.iter.clear();
    K.chain.clear();
    return SPAI_OK;
}

int trees_create(spai_engine *e, uint32_t n) {
    SPAI_CHECK(n > 0 && n <= e->cfg.max_trees, SPAI_ERR_INVALID, "trees_create: n=%u exceeds max_trees=%u", n,
               e->cfg.max_trees);
    Trees &T = e->trees;
    // worst case: one expansion of <= 7 children per search iteration for every ply of the game
    const uint64_t cap = 1ull + (uint64_t)c4::kActions * e->cfg.num_searches * std::max(1u, e->cfg.max_moves);
    SPAI_CHECK(cap < (1ull << 24), SPAI_ERR_CAPACITY, "node arena of %llu nodes per tree exceeds 2^24",
               (unsigned long long)cap);
    if (T.n_trees != n || T.cap != cap) {
        T.n_trees = 0;
        SPAI_TRY(T.nodes.alloc((size_t)n * cap));
        SPAI_TRY(T.root.alloc(n));
        SPAI_TRY(T.next_free.alloc(n));
        SPAI_TRY(T.root_x.alloc(n));
        SPAI_TRY(T.root_o.alloc(n));
        SPAI_TRY(T.root_n.alloc(n));
        SPAI_TRY(T.root_status.alloc(n));
        SPAI_TRY(T.path.alloc((size_t)n * kMaxDepth));
        SPAI_TRY(T.depth.alloc(n));
        SPAI_TRY(T.slot.alloc(n));
        SPAI_TRY(T.left.alloc(n));
        SPAI_TRY(T.evals.alloc(n + 2));   // [n], [n + 1]: the search call's max and sum over trees (k_root_stats)
        SPAI_TRY(T.slot_gid.alloc(n));
        SPAI_TRY(T.slot_move.alloc(n));
        SPAI_TRY(T.refill.alloc(2 * (size_t)n));
        SPAI_TRY(e->active.alloc(n));
        SPAI_TRY(e->stats.alloc((size_t)n * 8));
        for (Batch &B : e->batch) {   // one double-buffered leaf batch per search chain
            SPAI_TRY(B.tree.alloc(2 * (size_t)n));
            SPAI_TRY(B.mine.alloc(2 * (size_t)n));
            SPAI_TRY(B.theirs.alloc(2 * (size_t)n));
            SPAI_TRY(B.priors.alloc(2 * (size_t)n * kPriorStride));
            SPAI_TRY(B.value.alloc(2 * (size_t)n));
            B.cap = n;
        }
        T.n_trees = n;
        T.cap = (uint32_t)cap;
    }
    e->last_evals_per_iter = -1;   // a fresh set of trees: no per-iteration statistics yet
    e->last_served_per_iter = -1;
    e->last_max_tree_evals = ~0u;
    T.h_root.assign(n, 0);
    T.h_root_state.assign(n, c4::State{0, 0, 0, c4::kOngoing});
    T.h_root_first.assign(n, 0);
    T.h_root_nch.assign(n, 0);
    k_trees_init<<<(n + 255) / 256, 256, 0, e->stream>>>(tree_view(e), roots_out(e), 0, n);
    SPAI_HIP(hipGetLastError());
    return upload_roots(e, 0, n);
}

int tree_reset(spai_engine *e, uint32_t t, const spai_c4_state *root) {
    Trees &T = e->trees;
    SPAI_CHECK(t < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", t);
    c4::State s{0, 0, 0, c4::kOngoing};
    if (root) {
        SPAI_CHECK(!(root->x & root->o) && !((root->x | root->o) & ~c4::kBoard) && root->status <= c4::kWon,
                   SPAI_ERR_INVALID, "root is not a Connect4 bitboard");
        s = from_abi(*root);
    }
    T.h_root[t] = 0;
    T.h_root_state[t] = s;
    T.h_root_first[t] = 0;
    T.h_root_nch[t] = 0;
    k_trees_init<<<1, 64, 0, e->stream>>>(tree_view(e), roots_out(e), t, 1);
    SPAI_HIP(hipGetLastError());
    return upload_roots(e, t, 1);
}

// the chain's evaluator over batch bv on stream st: the net's forward, or a stub
static int evaluate(const Chain &c, hipStream_t st, const BatchView &bv, uint32_t grid_cap, int conc) {
    if (c.kind == SPAI_EVAL_NET)
        return net_eval_batch(c.net, st, bv.count, c.cnt, bv.mine, bv.theirs, bv.priors, bv.value, grid_cap, conc);
    k_eval_stub<<<(c.cnt + kBlock - 1) / kBlock, kBlock, 0, st>>>(bv, c.cnt, c.kind);
    return SPAI_OK;
}

// k_root_noise over the n trees of act on stream st (entry: see the kernel)
static int root_noise_launch(spai_engine *e, const RootNoise &N, hipStream_t st, const uint32_t *act, uint32_t n,
                             int entry) {
    if (!n) return SPAI_OK;
    k_root_noise<<<(n + kNoiseWaves - 1) / kNoiseWaves, 64 * kNoiseWaves, 0, st>>>(
        tree_view(e), act, n, N.gid, N.move, N.done, entry, N.seed, N.alpha, 1.0f - N.eps, N.eps);
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

int root_noise_prepare(spai_engine *e, RootNoise &out, bool &on) {
    on = e->noise_eps > 0.0f;
    if (!on) return SPAI_OK;
    Trees &T = e->trees;
    if (e->noise_done.n < T.n_trees) SPAI_TRY(e->noise_done.alloc(T.n_trees));
    out = RootNoise{e->noise_alpha, e->noise_eps, e->cfg.seed, T.slot_gid.p, T.slot_move.p, e->noise_done.p};
    return SPAI_OK;
}

// Enqueue one search call of `nchain` chains over `trees`, up to the join on the
// engine stream.  Per chain: select(0); then per iteration: evaluate(it),
// expand(it)+select(it+1) fused, and expand alone after the last evaluation.  A
// chain without trees launches nothing and is neither forked nor joined; one with
// fewer iterations than another stops early.  timed: the engine's timers, when on,
// sample every stride-th iteration: kind 0 the select-bearing launch (k_select /
// k_expand_select), 1 the evaluator, 2 the last k_expand.  tail: only the setup,
// with the counters of the tail passes, which the caller runs.
//
// noise (root_noise_launch; null: nothing of this is enqueued): the roots that have
// children on entry are mixed by one launch over all the call's trees behind the setup,
// before the fork.  A fresh root gets its children from iteration 0's expansion, and
// k_expand_select would select iteration 1 at it in the same launch, from priors not
// mixed yet; so iteration 0 of every chain runs unfused: evaluate(0), k_expand, the mix
// of the chain's roots still unmixed, k_select into batch 1, and the loop goes on at
// evaluate(1).  k_expand then k_select is what k_expand_select does per tree; the
// cache's inserts of iteration 0 only land before iteration 1's lookups, which changes
// hit counts, never results.
int chains_launch(spai_engine *e, const uint32_t *trees, const Chain *chains, int nchain, uint32_t grid_cap, bool timed,
                  bool tail, const RootNoise *noise) {
    hipStream_t st = e->stream;
    // the call's sequence number, from 1: the stamp of the cache entries it claims and hits
    const uint32_t seq = e->cache.seq = e->cache.seq + 1u ? e->cache.seq + 1u : 1u;
    uint32_t n = 0, iters = 0;
    int conc = 0;   // chains whose forwards share the CUs
    for (int h = 0; h < nchain; ++h) {   // per-iteration leaf counters (also the batch slot counters)
        const Chain &c = chains[h];
        if (!c.cnt) continue;
        n += c.cnt;
        iters = std::max(iters, c.iters);
        conc += c.kind == SPAI_EVAL_NET;
        Batch &B = e->batch[h];
        // at least one counter, so the memset never sees a null buffer on a fresh engine;
        // tail mode runs up to iters + 1 passes in chunks of kTailChunk
        const uint32_t nc = std::max<uint32_t>(c.iters, 1) + (tail ? kTailChunk + 1 : 0);
        DevBuf<uint32_t> *ctr[3] = {&B.iter_counts, c.cache.tab ? &B.iter_hits : nullptr,
                                    tail ? &B.iter_more : nullptr};
        for (DevBuf<uint32_t> *b : ctr) {   // (hits: the leaves served from the cache; more: capped tail passes)
            if (!b) continue;
            if (b->n < nc) SPAI_TRY(b->alloc(nc));
            SPAI_HIP(hipMemsetAsync(b->p, 0, (size_t)nc * 4, st));
        }
    }
    SPAI_HIP(hipMemcpyAsync(e->active.p, trees, (size_t)n * 4, hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemsetAsync(e->err.p, 0, 4, st));
    SPAI_HIP(hipMemsetAsync(e->trees.evals.p, 0, ((size_t)e->trees.n_trees + 2) * 4, st));
    if (noise && !tail) SPAI_TRY(root_noise_launch(e, *noise, st, e->active.p, n, 1));   // (tail: behind k_set_left)
    // fork: the chains 1.. that have trees start after the setup on the engine stream
    if (n > chains[0].cnt) SPAI_HIP(hipEventRecord(e->ev_fork, st));
    for (int h = 1; h < nchain; ++h)
        if (chains[h].cnt) SPAI_HIP(hipStreamWaitEvent(e->chain_stream[h], e->ev_fork, 0));
    const TreeView tv = tree_view(e);
    timed = timed && e->timer.enabled;
    for (uint32_t it = 0; it < (tail ? 0u : iters); ++it) {
        for (int h = 0; h < nchain; ++h) {
            const Chain &c = chains[h];
            if (!c.cnt || it >= c.iters) continue;
            const hipStream_t sh = e->chain_stream[h];
            const BatchView bv = batch_view(e, h, it, c.cache.tab);
            CacheView cache = c.cache;
            cache.seq = seq;
            const uint32_t nh = c.cnt, g8 = (nh + kTreesPerBlock - 1) / kTreesPerBlock;
            const uint32_t *act = e->active.p + c.off;
            const bool sample = timed && (it % e->timer.stride == 0);
            if (it == 0) {
                if (sample) SPAI_TRY(timer_record(e, 0, it, true, sh, h));
                k_select<false><<<g8, kBlock, 0, sh>>>(tv, bv, cache, act, nh, e->cfg.c, e->err.p, 0u);
                if (sample) SPAI_TRY(timer_record(e, 0, it, false, sh, h));
            }
            if (sample) SPAI_TRY(timer_record(e, 1, it, true, sh, h));
            SPAI_TRY(evaluate(c, sh, bv, grid_cap, std::max(conc, 1)));
            if (sample) SPAI_TRY(timer_record(e, 1, it, false, sh, h));
            if (noise && it == 0) {   // unfused, the fresh roots mixed between the expansion and the selection
                k_expand<<<g8, kBlock, 0, sh>>>(tv, bv, cache, nh, e->err.p);
                SPAI_TRY(root_noise_launch(e, *noise, sh, act, nh, 0));
                if (c.iters > 1) {
                    const bool s2 = timed && (1 % e->timer.stride == 0);
                    if (s2) SPAI_TRY(timer_record(e, 0, 1, true, sh, h));
                    k_select<false><<<g8, kBlock, 0, sh>>>(tv, batch_view(e, h, 1, c.cache.tab), cache, act, nh,
                                                          e->cfg.c, e->err.p, 0u);
                    if (s2) SPAI_TRY(timer_record(e, 0, 1, false, sh, h));
                }
            } else if (it + 1 < c.iters) {
                const bool s2 = timed && ((it + 1) % e->timer.stride == 0);
                if (s2) SPAI_TRY(timer_record(e, 0, it + 1, true, sh, h));
                k_expand_select<false><<<g8, kBlock, 0, sh>>>(tv, bv, batch_view(e, h, it + 1, c.cache.tab), cache,
                                                              act, nh, e->cfg.c, e->err.p, 0u);
                if (s2) SPAI_TRY(timer_record(e, 0, it + 1, false, sh, h));
            } else {
                if (sample) SPAI_TRY(timer_record(e, 2, it, true, sh, h));
                k_expand<<<g8, kBlock, 0, sh>>>(tv, bv, cache, nh, e->err.p);
                if (sample) SPAI_TRY(timer_record(e, 2, it, false, sh, h));
            }
        }
    }
    SPAI_HIP(hipGetLastError());
    for (int h = 1; h < nchain; ++h) {   // join
        if (!chains[h].cnt) continue;
        SPAI_HIP(hipEventRecord(e->ev_join[h], e->chain_stream[h]));
        SPAI_HIP(hipStreamWaitEvent(st, e->ev_join[h], 0));
    }
    return SPAI_OK;
}

// Enqueue one search call over n >= 1 validated trees (mcts.rs:214-285 per tree),
// up to the join of its chains on the engine stream.  Only tail mode waits (once
// per chunk of passes, for its stop condition).
int search_launch(spai_engine *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, SearchRun &R,
                  const RootNoise *noise) {
    const int kind = (int)e->cfg.eval;
    hipStream_t st = e->stream;
    // evaluation cache: allocated on first use; thinned here, between search calls
    // (no chain runs), once it is more than 7/8 full: the entries that were hit and
    // the newest stay, so a long stream keeps hitting what it was hitting
    SPAI_TRY(cache_prepare(e, kind == SPAI_EVAL_NET));
    if (cache_nearly_full(e->cache)) SPAI_TRY(cache_thin(e, cache_keep_budget(e->cache)));
    // tail mode (select_tree RUN_ON, one chain): late in a game, when in the previous
    // search call of these trees no tree evaluated SPAI_TAIL_TREE_EVALS leaves or
    // more (a pass per live leaf of the busiest tree: few passes), or the call
    // averaged fewer than SPAI_TAIL_LEAVES leaves per iteration.  Both read per
    // call (tests set them per case); 0 turns a criterion off.
    const char *tl_env = std::getenv("SPAI_TAIL_LEAVES");
    const char *tt_env = std::getenv("SPAI_TAIL_TREE_EVALS");
    const double tail_leaves = tl_env ? std::atof(tl_env) : kTailLeaves;
    const uint32_t tail_tree = tt_env ? (uint32_t)std::max(0, std::atoi(tt_env)) : kTailTreeEvals;
    // (a tree's passes are its live leaves, whether the forward or the evaluation cache
    // answers them: the served leaves decide here, the forwarded ones in chains_for)
    const bool tail = num_searches > 0 && e->last_served_per_iter >= 0 &&
                      (e->last_served_per_iter < tail_leaves || e->last_max_tree_evals < tail_tree);
    // the run cap; after a call that evaluated nothing (every tree solved: no tree
    // to keep waiting) none, and a check after every pass -- normally one
    const bool solved = e->last_served_per_iter == 0.0;
    const char *tr_env = std::getenv("SPAI_TAIL_RUN");
    const uint32_t tail_run =
        tr_env ? (uint32_t)std::max(1, std::atoi(tr_env)) : (solved ? std::max(num_searches, 1u) : kTailRun);
    const uint32_t tail_chunk = solved ? 1u : kTailChunk;
    // chain h searches an even share of the trees, in order
    const ChainPolicy pol = tail ? ChainPolicy{1, 0u} : chains_for(n, e->last_evals_per_iter);
    const int nchain = R.nchain = pol.chains;
    CacheView cv = cache_view(e);
    for (int h = 0; h < nchain; ++h) {
        const uint32_t off = (uint32_t)((uint64_t)n * h / nchain);
        R.chain[h] = Chain{off, (uint32_t)((uint64_t)n * (h + 1) / nchain) - off, num_searches, kind, e->net, cv};
    }
    SPAI_TRY(chains_launch(e, tree_idx, R.chain, nchain, pol.grid_cap, true, tail, noise));
    cv.seq = e->cache.seq;   // (the tail passes below are this call's too)
    R.n_counts = num_searches;   // leaf counters to read back per chain
    if (tail) {
        // passes on the engine stream: select(0), then per pass p: evaluate(p),
        // expand(p) + select(p + 1), each select running its trees on through
        // terminal leaves (at most tail_run per pass).  A pass whose select slots
        // no leaf and caps no tree leaves no tree with iterations to run (a tree
        // stops a launch only at a live leaf or the cap), so the host checks every
        // tail_chunk passes and stops there.
        const TreeView tv = tree_view(e);
        const uint32_t g8 = (n + kTreesPerBlock - 1) / kTreesPerBlock;
        const uint32_t *act = e->active.p;
        k_set_left<<<(n + 255) / 256, 256, 0, st>>>(tv, act, n, num_searches);
        if (noise) SPAI_TRY(root_noise_launch(e, *noise, st, act, n, 1));
        k_select<true><<<g8, kBlock, 0, st>>>(tv, batch_view(e, 0, 0, cv.tab), cv, act, n, e->cfg.c, e->err.p, tail_run);
        uint32_t p = 0, next = 1, more = 0, next_hits = 0;
        if (noise) {
            // pass 0 unfused (chains_launch): select<true> runs on through terminal children, so a
            // fresh root must be mixed before the first selection at it, not after the pass
            const BatchView bv = batch_view(e, 0, 0, cv.tab);
            SPAI_TRY(evaluate(R.chain[0], st, bv, 0u, 1));
            k_expand<<<g8, kBlock, 0, st>>>(tv, bv, cv, n, e->err.p);
            SPAI_TRY(root_noise_launch(e, *noise, st, act, n, 0));
            k_select<true><<<g8, kBlock, 0, st>>>(tv, batch_view(e, 0, 1, cv.tab), cv, act, n, e->cfg.c, e->err.p,
                                                 tail_run);
            p = 1;
        }
        for (;;) {
            for (uint32_t q = 0; q < tail_chunk; ++q, ++p) {
                const BatchView bv = batch_view(e, 0, p, cv.tab);
                SPAI_TRY(evaluate(R.chain[0], st, bv, 0u, 1));
                k_expand_select<true><<<g8, kBlock, 0, st>>>(tv, bv, batch_view(e, 0, p + 1, cv.tab), cv, act, n,
                                                             e->cfg.c, e->err.p, tail_run);
            }
            SPAI_HIP(hipGetLastError());
            SPAI_HIP(hipMemcpyAsync(&next, e->batch[0].iter_counts.p + p, 4, hipMemcpyDeviceToHost, st));
            SPAI_HIP(hipMemcpyAsync(&more, e->batch[0].iter_more.p + p, 4, hipMemcpyDeviceToHost, st));
            if (cv.tab)   // a leaf served from the evaluation cache stops its tree's pass like a forwarded one
                SPAI_HIP(hipMemcpyAsync(&next_hits, e->batch[0].iter_hits.p + p, 4, hipMemcpyDeviceToHost, st));
            SPAI_HIP(hipStreamSynchronize(st));
            next += next_hits;
            if (next == 0 && more == 0) break;   // pass p has nothing to evaluate and no tree was capped: all done
            SPAI_CHECK(p <= num_searches + 1, SPAI_ERR_INVALID, "internal: tail passes exceed the iterations");
            // this chunk's counters are read back below; the next chunk's are fresh
        }
        R.n_counts = p;
    }
    e->last_tail_passes = tail ? R.n_counts : 0;
    return SPAI_OK;
}

int check_device_errors(spai_engine *e, uint32_t err) {
    SPAI_CHECK(!(err & kErrCapacity), SPAI_ERR_CAPACITY, "node arena full (cap %u per tree)", e->trees.cap);
    SPAI_CHECK(!(err & kErrDepth), SPAI_ERR_CAPACITY, "tree deeper than %d", kMaxDepth);
    SPAI_CHECK(!(err & kErrNan), SPAI_ERR_NAN, "NaN UCB in select (reference: partial_cmp().unwrap() panics)");
    return SPAI_OK;
}

void cache_account(spai_engine *e, double served, double forwarded, uint32_t fill) {
    if (!e->cache.buckets) return;
    e->cache.lookups += served;
    e->cache.hits += served - forwarded;
    e->cache.fill_seen = fill;
}

// The call's bookkeeping once its counters [chain][n_counts], error flags and
// largest per-tree leaf count are on the host: timers, the device errors, and the
// statistics the next call's chain and tail policies read.
// `served`: the call's live leaves, those answered by the evaluation cache included
// (the statistic `evals`); the counters hold the leaves the forward ran, which is what
// the launches cost and so what the chain and group-size policies go by.  The tail-mode
// policy goes by the served leaves: a tree's tail passes are its live leaves, whoever
// answers them.
int search_finish(spai_engine *e, const SearchRun &R, uint32_t num_searches, const uint32_t *ch_counts, uint32_t err,
                  uint32_t max_tree_evals, double served, uint32_t cache_fill) {
    SPAI_TRY(timer_collect(e, ch_counts, R.n_counts, R.chain));
    double s = 0;
    for (int h = 0; h < R.nchain; ++h)
        for (uint32_t i = 0; i < R.n_counts; ++i) s += ch_counts[(size_t)h * R.n_counts + i];
    SPAI_TRY(check_device_errors(e, err));
    cache_account(e, served, s, cache_fill);
    e->last_evals_per_iter = num_searches ? s / num_searches : -1;
    e->last_served_per_iter = num_searches ? served / num_searches : -1;
    e->last_max_tree_evals = max_tree_evals;
    return SPAI_OK;
}

int search(spai_engine *e, uint32_t n, const uint32_t *tree_idx, uint32_t num_searches, float *policy,
           uint32_t *child_ids, float *child_visits, uint32_t *n_children, double *evals_out,
           const uint64_t *game_id, const uint32_t *move_no) {
    Trees &T = e->trees;
    SPAI_CHECK(T.n_trees > 0, SPAI_ERR_INVALID, "no trees: call spai_trees_create first");
    SPAI_CHECK(n <= T.n_trees, SPAI_ERR_INVALID, "search over %u trees, %u exist", n, T.n_trees);
    for (uint32_t i = 0; i < n; ++i) SPAI_CHECK(tree_idx[i] < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", tree_idx[i]);
    const int kind = (int)e->cfg.eval;
    SPAI_CHECK(kind != SPAI_EVAL_NET || e->net, SPAI_ERR_INVALID, "eval = NET but no net set (spai_engine_set_net)");
    if (n == 0) return SPAI_OK;
    hipStream_t st = e->stream;
    SearchRun R;
    RootNoise noise{};
    bool keyed = false;
    if (game_id && move_no) SPAI_TRY(root_noise_prepare(e, noise, keyed));
    if (keyed) {
        // a tree listed twice would be mixed twice in one call, by two waves at once
        std::vector<char> seen(T.n_trees, 0);
        for (uint32_t i = 0; i < n; ++i) {
            SPAI_CHECK(!seen[tree_idx[i]], SPAI_ERR_INVALID, "keyed search: tree %u listed twice", tree_idx[i]);
            seen[tree_idx[i]] = 1;
        }
        // the keys go into the per-tree arrays self-play keeps its own in (k_slots_start
        // resets those at the start of every self-play call)
        if (e->noise_gid.n < n) SPAI_TRY(e->noise_gid.alloc(T.n_trees));
        if (e->noise_move.n < n) SPAI_TRY(e->noise_move.alloc(T.n_trees));
        SPAI_HIP(hipMemcpyAsync(e->active.p, tree_idx, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SPAI_HIP(hipMemcpyAsync(e->noise_gid.p, game_id, (size_t)n * 8, hipMemcpyHostToDevice, st));
        SPAI_HIP(hipMemcpyAsync(e->noise_move.p, move_no, (size_t)n * 4, hipMemcpyHostToDevice, st));
        k_noise_keys<<<(n + 255) / 256, 256, 0, st>>>(e->active.p, n, e->noise_gid.p, e->noise_move.p, T.slot_gid.p,
                                                     T.slot_move.p);
        SPAI_HIP(hipGetLastError());
    }
    SPAI_TRY(search_launch(e, n, tree_idx, num_searches, R, keyed ? &noise : nullptr));
    const TreeView tv = tree_view(e);
    const int nchain = R.nchain;
    const uint32_t n_counts = R.n_counts;
    k_root_stats<<<(n + 255) / 256, 256, 0, st>>>(tv, e->active.p, n, e->stats.p, T.evals.p + T.n_trees);
    SPAI_HIP(hipGetLastError());
    std::vector<uint32_t> stats((size_t)n * 8), ch_counts((size_t)nchain * n_counts);
    uint32_t err = 0, tree_evals[2] = {0, 0}, cache_fill = 0;   // the trees' max and sum
    SPAI_HIP(hipMemcpyAsync(stats.data(), e->stats.p, stats.size() * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipMemcpyAsync(tree_evals, T.evals.p + T.n_trees, 8, hipMemcpyDeviceToHost, st));
    if (e->cache.buckets) SPAI_HIP(hipMemcpyAsync(&cache_fill, e->cache.ctr.p, 4, hipMemcpyDeviceToHost, st));
    if (n_counts)
        for (int h = 0; h < nchain; ++h)
            SPAI_HIP(hipMemcpyAsync(ch_counts.data() + (size_t)h * n_counts, e->batch[h].iter_counts.p,
                                    n_counts * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipMemcpyAsync(&err, e->err.p, 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    SPAI_TRY(search_finish(e, R, num_searches, ch_counts.data(), err, tree_evals[0], tree_evals[1], cache_fill));
    if (evals_out) *evals_out = (double)tree_evals[1];
    // root visit policy (mcts.rs:310-331)
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t t = tree_idx[i];
        const uint32_t w = stats[i * 8];
        const uint32_t nch = w == kNoChildren ? 0 : w >> 24, first = w & 0xFFFFFFu;
        T.h_root_first[t] = first;
        T.h_root_nch[t] = (uint8_t)nch;
        const c4::State &rs = T.h_root_state[t];
        const uint32_t legal = c4::legal_mask(rs.x, rs.o, rs.status);
        float pol[c4::kActions] = {0, 0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < nch; ++k) {
            const float v = (float)stats[i * 8 + 1 + k];
            pol[c4::kth_bit(legal, (int)k)] = v;
            if (child_ids) child_ids[(size_t)i * 7 + k] = first + k;
            if (child_visits) child_visits[(size_t)i * 7 + k] = v;
        }
        for (uint32_t k = nch; k < 7; ++k) {
            if (child_ids) child_ids[(size_t)i * 7 + k] = kNoChildren;
            if (child_visits) child_visits[(size_t)i * 7 + k] = 0.f;
        }
        if (n_children) n_children[i] = nch;
        if (policy) normalize_policy(pol, policy + (size_t)i * 7);
    }
    return SPAI_OK;
}

int root_noise_draws(spai_engine *e, uint32_t count, const uint64_t *game_id, const uint32_t *move_no,
                     const uint32_t *n_children, float alpha, float *eta) {
    if (!count) return SPAI_OK;
    for (uint32_t i = 0; i < count; ++i)
        SPAI_CHECK(n_children[i] >= 1 && n_children[i] <= (uint32_t)c4::kActions, SPAI_ERR_INVALID,
                   "root noise: n_children[%u] = %u not in [1, %d]", i, n_children[i], c4::kActions);
    DevBuf<uint64_t> d_gid;
    DevBuf<uint32_t> d_move, d_n;
    DevBuf<float> d_eta;
    int rc = d_gid.alloc(count);
    if (rc == SPAI_OK) rc = d_move.alloc(count);
    if (rc == SPAI_OK) rc = d_n.alloc(count);
    if (rc == SPAI_OK) rc = d_eta.alloc((size_t)count * c4::kActions);
    auto run = [&]() -> int {
        hipStream_t st = e->stream;
        SPAI_HIP(hipMemcpyAsync(d_gid.p, game_id, 8ull * count, hipMemcpyHostToDevice, st));
        SPAI_HIP(hipMemcpyAsync(d_move.p, move_no, 4ull * count, hipMemcpyHostToDevice, st));
        SPAI_HIP(hipMemcpyAsync(d_n.p, n_children, 4ull * count, hipMemcpyHostToDevice, st));
        k_noise_draws<<<(count + kNoiseWaves - 1) / kNoiseWaves, 64 * kNoiseWaves, 0, st>>>(
            count, d_gid.p, d_move.p, d_n.p, e->cfg.seed, alpha, d_eta.p);
        SPAI_HIP(hipGetLastError());
        SPAI_HIP(hipMemcpyAsync(eta, d_eta.p, 4ull * count * c4::kActions, hipMemcpyDeviceToHost, st));
        SPAI_HIP(hipStreamSynchronize(st));
        return SPAI_OK;
    };
    if (rc == SPAI_OK) rc = run();
    d_gid.release();
    d_move.release();
    d_n.release();
    d_eta.release();
    return rc;
}

int tree_use_subtree(spai_engine *e, uint32_t t, uint32_t child) {
    Trees &T = e->trees;
    SPAI_CHECK(t < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", t);
    const uint32_t first = T.h_root_first[t], nch = T.h_root_nch[t];
    SPAI_CHECK(nch > 0 && child >= first && child < first + nch, SPAI_ERR_INVALID,
               "node %u is not a child of tree %u's root (run spai_search first)", child, t);
    const c4::State &rs = T.h_root_state[t];
    c4::State ns;
    const int a = c4::kth_bit(c4::legal_mask(rs.x, rs.o, rs.status), (int)(child - first));
    SPAI_CHECK(c4::next_state(rs, a, ns) == 0, SPAI_ERR_INVALID, "internal: root child replay failed");
    T.h_root[t] = child;
    T.h_root_state[t] = ns;
    T.h_root_nch[t] = 0;
    return upload_roots(e, t, 1);
}

int tree_node(spai_engine *e, uint32_t t, uint32_t node, spai_c4_state *st, uint32_t *visits, float *w) {
    Trees &T = e->trees;
    SPAI_CHECK(t < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", t);
    c4::State s = T.h_root_state[t];
    if (node != T.h_root[t]) {
        const uint32_t first = T.h_root_first[t], nch = T.h_root_nch[t];
        SPAI_CHECK(nch > 0 && node >= first && node < first + nch, SPAI_ERR_INVALID,
                   "node %u: only the root and its children are addressable", node);
        const int a = c4::kth_bit(c4::legal_mask(s.x, s.o, s.status), (int)(node - first));
        c4::State ns;
        c4::next_state(s, a, ns);
        s = ns;
    }
    if (st) *st = to_abi(s);
    if (visits || w) {
        uint4 rec;
        SPAI_HIP(hipMemcpy(&rec, T.nodes.p + (size_t)t * T.cap + node, 16, hipMemcpyDeviceToHost));
        if (visits) *visits = rec.x;
        if (w) memcpy(w, &rec.y, 4);
    }
    return SPAI_OK;
}

// The root's child records as they stand on the device: read-only, the root taken from the
// device's own table (a move step re-roots there), bounds checked before the second read.
int tree_child_stats(spai_engine *e, uint32_t t, uint32_t *child_ids, uint32_t *visits, float *value_sums,
                     float *priors, uint32_t *n_children) {
    Trees &T = e->trees;
    SPAI_CHECK(t < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", t);
    SPAI_HIP(hipStreamSynchronize(e->stream));
    uint32_t r = 0;
    SPAI_HIP(hipMemcpy(&r, T.root.p + t, 4, hipMemcpyDeviceToHost));
    SPAI_CHECK(r < T.cap, SPAI_ERR_INVALID, "internal: root %u past the arena", r);
    const uint4 *nodes = T.nodes.p + (size_t)t * T.cap;
    uint4 rec;
    SPAI_HIP(hipMemcpy(&rec, nodes + r, 16, hipMemcpyDeviceToHost));
    const uint32_t nch = root_children(rec.w), first = rec.w & 0xFFFFFFu;
    SPAI_CHECK(nch <= (uint32_t)c4::kActions, SPAI_ERR_INVALID, "internal: root with %u children", nch);
    uint4 ch[c4::kActions];
    if (nch) {
        SPAI_CHECK((uint64_t)first + nch <= T.cap, SPAI_ERR_INVALID, "internal: children [%u, %u) past the arena",
                   first, first + nch);
        SPAI_HIP(hipMemcpy(ch, nodes + first, 16ull * nch, hipMemcpyDeviceToHost));
    }
    if (n_children) *n_children = nch;
    for (uint32_t k = 0; k < (uint32_t)c4::kActions; ++k) {
        const uint4 c = k < nch ? ch[k] : make_uint4(0, 0, 0, 0);
        if (child_ids) child_ids[k] = k < nch ? first + k : kNoChildren;
        if (visits) visits[k] = c.x;
        if (value_sums) memcpy(value_sums + k, &c.y, 4);
        if (priors) memcpy(priors + k, &c.z, 4);
    }
    return SPAI_OK;
}

int tree_size(spai_engine *e, uint32_t t, uint32_t *nodes) {
    Trees &T = e->trees;
    SPAI_CHECK(t < T.n_trees, SPAI_ERR_INVALID, "tree %u out of range", t);
    SPAI_HIP(hipMemcpy(nodes, T.next_free.p + t, 4, hipMemcpyDeviceToHost));
    return SPAI_OK;
}


int eval_cache_set_capacity(spai_engine *e, uint64_t entries) {
    e->cache.user_set = true;
    e->cache.requested = entries;
    e->cache.ready = false;   // resolved, and the table resized, at the next search call
    return SPAI_OK;
}

int eval_cache_clear(spai_engine *e) { return cache_clear(e); }

int eval_cache_thin(spai_engine *e, uint64_t keep_entries) { return cache_thin(e, keep_entries); }

int eval_cache_stats(spai_engine *e, spai_eval_cache_stats *out) {
    EvalCache &C = e->cache;
    uint32_t ctr[2] = {0, 0};
    SPAI_HIP(hipStreamSynchronize(e->stream));
    if (C.ctr.p) SPAI_HIP(hipMemcpy(ctr, C.ctr.p, 8, hipMemcpyDeviceToHost));
    out->lookups = C.lookups;
    out->hits = C.hits;
    out->inserts = C.inserts_cleared + ctr[0];
    out->dropped = ctr[1];
    out->clears = C.clears;
    out->capacity = (double)C.entries();
    out->thins = C.thins;
    out->evicted = C.evicted;
    out->live = C.buckets ? (double)ctr[0] : 0.0;
    out->kept_hit = C.kept_hit;
    return SPAI_OK;
}

}  // namespace spai
