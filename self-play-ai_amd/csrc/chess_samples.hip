// chess_samples.hip — compact chess self-play samples (spai_chess_sample in
// include/spai.h): what self-play knows about a searched position (its 72-byte
// board, its repetition count, the root children's moves and visit counts)
// instead of the dense [19][8][8] encoding and [4672] policy row built from it.
//
//  * samples_validate: the host check every consumer runs before it reads a
//    child array or launches anything.
//  * spai_chess_samples_expand: the dense form on the host, by encode_host and
//    dense_policy themselves (what self-play's dense sink hands over).
//  * k_samples_expand: the same dense form written on the learner's device,
//    straight into its batch_in [x: B*1216 | pi: B*4672 | z: B], bit for bit.
//    One workgroup (4 waves) per sample.  Planes: every wave computes
//    encode_cell for its lane's cell and stores the planes p = wave (mod 4), a
//    store being 64 consecutive floats.  Policy: the row is built in LDS (zero
//    fill, barrier, one child per thread scattered as (float)N / total) and
//    leaves as 16-byte stores of consecutive lanes.  The total is a wave
//    shuffle sum and four partials: the visit counts are integers whose sum is
//    below 2^24 (validated), so every partial sum is exact in fp32 and the order
//    does not matter; the one rounding is the divide, which is correctly
//    rounded on both sides.  Two children of one sample never share an index
//    (validated), so the scatter has no race.
#include <algorithm>
#include <vector>

#include "chess_engine.h"

static_assert(sizeof(spai_chess_sample) == 96, "spai_chess_sample is 96 bytes");

namespace spai {
namespace chess {
namespace {

constexpr int kEnc = kPlanes * 64;   // 1216
constexpr int kExpandThreads = 256;
static_assert(kExpandThreads >= kMaxMoves, "one child per thread");
static_assert(kPolicy % 4 == 0 && kEnc % 4 == 0, "rows are whole 16-byte groups");

__global__ __launch_bounds__(kExpandThreads) void k_samples_expand(const spai_chess_sample *__restrict__ samples,
                                                                   const uint32_t *__restrict__ visits,
                                                                   const uint16_t *__restrict__ moves,
                                                                   uint32_t n_children_total, float *__restrict__ x,
                                                                   float *__restrict__ pi, float *__restrict__ z) {
    __shared__ __attribute__((aligned(16))) float row[kPolicy];
    __shared__ float part[kExpandThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t s = blockIdx.x;
    const spai_chess_sample &r = samples[s];
    Board b;
#pragma unroll
    for (int p = 0; p < 6; ++p) b.pc[p] = r.state.pieces[p];
    b.col[WHITE] = r.state.colors[0];
    b.col[BLACK] = r.state.colors[1];
    b.side = r.state.side;
    b.castle = r.state.castle;
    b.ep = r.state.ep;
    b.status = 0;
    b.fifty = r.state.fifty;
    b.made = r.state.made;
    for (int j = t; j < kPolicy; j += kExpandThreads) row[j] = 0.0f;
    // the planes: wave w stores planes w, w + 4, ...
    float v[kPlanes];
    encode_cell(b, r.state.reps, lane, v);
    float *xs = x + s * kEnc;
#pragma unroll
    for (int p = 0; p < kPlanes; ++p)
        if ((p & 3) == wave) xs[p * 64 + lane] = v[p];
    // the policy row: child t of the sample (validated on the host; the guards keep a
    // record that was not from reading or writing out of bounds)
    const uint32_t nch = min((uint32_t)r.n_children, (uint32_t)kMaxMoves), first = r.first;
    float fv = 0.0f;
    int idx = -1;
    if ((uint32_t)t < nch && (uint64_t)first + (uint32_t)t < n_children_total) {
        fv = (float)visits[first + t];
        idx = policy_index(b.side, moves[first + t]);
    }
    float tot = fv;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane == 0) part[wave] = tot;
    __syncthreads();   // the partials are there, and the zero fill is complete
    tot = (part[0] + part[1]) + (part[2] + part[3]);
    if ((unsigned)idx < (unsigned)kPolicy) row[idx] = fv / tot;
    __syncthreads();
    float4 *dst = reinterpret_cast<float4 *>(pi + s * kPolicy);
    const float4 *src = reinterpret_cast<const float4 *>(row);
    for (int j = t; j < kPolicy / 4; j += kExpandThreads) dst[j] = src[j];
    if (t == 0) z[s] = r.value;
}

}  // namespace

int samples_validate(uint32_t n, const spai_chess_sample *samples, const uint16_t *child_moves,
                     const uint32_t *child_visits, uint32_t n_children_total) {
    std::vector<uint32_t> seen(kPolicy, 0xFFFFFFFFu);   // the last sample that set each index
    for (uint32_t i = 0; i < n; ++i) {
        const spai_chess_sample &r = samples[i];
        SPAI_CHECK(r.n_children >= 1 && r.n_children <= kMaxMoves, SPAI_ERR_INVALID,
                   "sample %u: n_children %u outside 1..%d", i, r.n_children, kMaxMoves);
        SPAI_CHECK((uint64_t)r.first + r.n_children <= n_children_total, SPAI_ERR_INVALID,
                   "sample %u: first %u + n_children %u goes past n_children_total %u", i, r.first, r.n_children,
                   n_children_total);
        const spai_chess_state &st = r.state;
        SPAI_CHECK(popc(st.pieces[KING] & st.colors[0]) == 1 && popc(st.pieces[KING] & st.colors[1]) == 1,
                   SPAI_ERR_INVALID, "sample %u: state: each side needs exactly one king", i);
        SPAI_CHECK(st.side <= 1, SPAI_ERR_INVALID, "sample %u: state.side %u is neither 0 nor 1", i, st.side);
        uint64_t tot = 0;
        for (uint32_t k = 0; k < r.n_children; ++k) {
            const int idx = policy_index(st.side, child_moves[r.first + k]);
            SPAI_CHECK(idx >= 0 && idx < kPolicy, SPAI_ERR_INVALID,
                       "sample %u: child_moves[%u] = %u has policy index %d outside [0, %d)", i, r.first + k,
                       child_moves[r.first + k], idx, kPolicy);
            SPAI_CHECK(seen[idx] != i, SPAI_ERR_INVALID,
                       "sample %u: child_moves[%u] = %u shares policy index %d with an earlier child", i, r.first + k,
                       child_moves[r.first + k], idx);
            seen[idx] = i;
            tot += child_visits[r.first + k];
        }
        SPAI_CHECK(tot >= 1 && tot < (1ull << 24), SPAI_ERR_INVALID,
                   "sample %u: child_visits sum to %llu, outside [1, 2^24)", i, (unsigned long long)tot);
    }
    return SPAI_OK;
}

void samples_expand_host(uint32_t n, const spai_chess_sample *samples, const uint16_t *child_moves,
                         const uint32_t *child_visits, float *states, float *policies, float *values) {
    for (uint32_t i = 0; i < n; ++i) {
        const spai_chess_sample &r = samples[i];
        if (states) encode_host(from_abi(r.state), r.state.reps, states + (size_t)i * kEnc);
        if (policies)
            dense_policy(r.state.side, r.n_children, child_visits + r.first, child_moves + r.first,
                         policies + (size_t)i * kPolicy);
        if (values) values[i] = r.value;
    }
}

int samples_expand_device(const spai_chess_sample *d_samples, const uint32_t *d_visits, const uint16_t *d_moves,
                          uint32_t n_children_total, uint32_t B, float *batch_in, hipStream_t st) {
    float *x = batch_in, *pi = x + (size_t)B * kEnc, *z = pi + (size_t)B * kPolicy;
    k_samples_expand<<<B, kExpandThreads, 0, st>>>(d_samples, d_visits, d_moves, n_children_total, x, pi, z);
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

}  // namespace chess
}  // namespace spai

using namespace spai;
using namespace spai::chess;

extern "C" int spai_chess_samples_expand(uint32_t n, const spai_chess_sample *samples, const uint16_t *child_moves,
                                         const uint32_t *child_visits, uint32_t n_children_total, float *states,
                                         float *policies, float *values) {
    if (!n) return SPAI_OK;
    SPAI_PTR(samples);
    SPAI_PTR(child_moves);
    SPAI_PTR(child_visits);
    SPAI_TRY(samples_validate(n, samples, child_moves, child_visits, n_children_total));
    samples_expand_host(n, samples, child_moves, child_visits, states, policies, values);
    return SPAI_OK;
}
