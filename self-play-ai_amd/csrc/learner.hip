// learner.hip — the training step of the C4 policy/value ResNet on the device
// (SURVEY.md §8f.1): ModelTrainerWorker::train_batch (learner_concurrent.rs:72-85)
// = Net::forward(x, train=true) (model/mod.rs:152-184, model/connect_four.rs:50-81),
// loss -(log_softmax(p)·π).sum()/B + MSE(v, z) (model/mod.rs:128-135), and
// tch's Adam::default() step (β1 0.9, β2 0.999, eps 1e-8, no weight decay,
// lr 1e-3; model/mod.rs:107).  BatchNorm runs in train mode: batch statistics
// over (B, 6, 7), running statistics updated with momentum 0.1 and the
// unbiased batch variance (tch/libtorch batch_norm semantics).
//
// Data-parallel learner: with a communicator set, the flat gradient is summed
// over ranks with RCCL (ncclAllReduce over xGMI) and scaled by 1/world before
// Adam, and the BN running statistics are averaged, so every rank holds the
// same parameters after every step.
//
// Layout: fp32 NCHW activations [B][C][42].  The convs (forward, data and
// weight gradients) run on the exact-f32 MFMA; every reduction has a fixed
// order and there are no float atomics, so a step is deterministic.
// Parameters, gradients and Adam moments share the flat construction-order
// layout of spai_net_create (conv w, b, BN γ, β, μ, σ²; linears w, b).
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "learner_common.h"

namespace spai {
namespace {

constexpr int kCells = 42, kCols = 7;
constexpr int kPlane = 73;        // LDS stride of a (6+2) x (7+2) zero-padded plane (odd, so channels spread over the banks)
constexpr int kThreads = 256;

// ------------------------------------------------------------------ conv 3x3 on f32 MFMA
// Every conv of the step is a GEMM on v_mfma_f32_16x16x4_f32 (exact f32: an
// fmaf chain per output element; 157 TF/s peak, the f32 vector rate).  The
// reduction index is tap-major, k = tap * cinp + c (cinp = input channels
// rounded up to 4), so one k-step of 4 stays inside one tap and a lane's LDS
// address is its position's tap offset plus the channel.
//   forward:  out[b][n][p] = bias[n] + sum_k X[b][p][k] * Wk[k][n]
//   data grad: the same with X = dz and Wk built from the flipped, transposed
//              weights (w'[ci][co][8 - tap] = w[co][ci][tap])
//   weight grad: part[b][n][k] = sum_p dz[b][n][p] * X[b][p][k], then a
//              fixed-order sum over the batch (deterministic, no atomics)
typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int round4(int c) { return (c + 3) & ~3; }
__host__ __device__ inline int round16(int c) { return (c + 15) & ~15; }

// tap offset inside a zero-padded 8 x 9 plane
__device__ __forceinline__ int tap_off(int tap) { return (tap / 3 - 1) * 9 + (tap % 3 - 1); }

// stage a sample's input planes [c][kPlane], zero-padded (rows -1..6, cols -1..7),
// channels >= cin zero, without per-element index math: thread t < 252 owns cell t % 42
// of channels t / 42 + 6j (source and LDS offsets are the thread's base plus
// immediates), thread t < 240 zeroes border cell t % 30 of channels t / 30 + 8j;
// the two sets are disjoint, so one barrier after the call covers both.
template <int CINP>
__device__ __forceinline__ void stage_planes_fast(const float *__restrict__ xb, int cin, float *xs) {
    const int t = threadIdx.x;
    if (t < 252) {
        const int c0 = t / kCells, cell = t - c0 * kCells;
        float *dst = xs + c0 * kPlane + (cell / kCols + 1) * 9 + cell % kCols + 1;
        const float *src = xb + t;
        float v[(CINP + 5) / 6];
#pragma unroll
        for (int j = 0; j < (CINP + 5) / 6; ++j) v[j] = c0 + 6 * j < cin ? src[252 * j] : 0.f;
#pragma unroll
        for (int j = 0; j < (CINP + 5) / 6; ++j)
            if (c0 + 6 * j < CINP) dst[6 * kPlane * j] = v[j];
    }
    if (t < 240) {
        const int c0 = t / 30, bi = t - c0 * 30;
        const int k = bi - 18;
        const int off = bi < 9 ? bi : bi < 18 ? 63 + bi - 9 : 9 * (1 + k / 2) + ((k & 1) ? 8 : 0);
        float *dst = xs + c0 * kPlane + off;
#pragma unroll
        for (int j = 0; j < (CINP + 7) / 8; ++j)
            if (c0 + 8 * j < CINP) dst[8 * kPlane * j] = 0.f;
    }
}

// Wk[(tap * cinp + c) * coutp + n]: forward Wk = w[n][c][tap]; data gradient Wk = w[c][n][8 - tap].
// Every conv's forward and data-gradient matrices are packed in one launch per
// step (blockIdx.y = entry of the table built at learner_create):
//   desc[8 y ..] = {param offset, cin, cout, cinp, coutp, dgrad, packed offset, 0}
constexpr int kPackDesc = 8;
__global__ void k_pack_all(const float *__restrict__ P, const uint32_t *__restrict__ desc, float *__restrict__ wall) {
    const uint32_t *d = desc + kPackDesc * blockIdx.y;
    const int cin = (int)d[1], cout = (int)d[2], cinp = (int)d[3], coutp = (int)d[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * cinp * coutp) return;
    const float *w = P + d[0];
    const int n = i % coutp, k = i / coutp, tap = k / cinp, c = k - tap * cinp;
    float v = 0.f;
    if (c < cin && n < cout)
        v = d[5] ? w[((size_t)c * cout + n) * 9 + (8 - tap)] : w[((size_t)n * cin + c) * 9 + tap];
    wall[d[6] + i] = v;
}

// workgroup (sample, slice): 3 position tiles (48 rows, 42 real) x NT channel
// tiles of output channels [16 NT slice, 16 NT (slice + 1)); wave w owns channel
// tile w % NT and K part w / NT (KS = 4/NT parts, summed in LDS in a fixed
// order).  CINP (input channels padded to 4) and NT are compile-time, so the
// k-loop unrolls fully and the weight loads of a whole part are in flight
// together.  coutp_all = the packed matrix's row length (all output channels).
template <int CINP, int NT>
__global__ __launch_bounds__(kThreads) void k_conv_mfma(const float *__restrict__ in, int cin,
                                                        const float *__restrict__ wk, const float *__restrict__ bias,
                                                        int cout, int coutp_all, float *__restrict__ out,
                                                        int accumulate) {
    constexpr int KS = 4 / NT, CSN = CINP / 4, KSTEPS = 9 * CSN, PER = KSTEPS / KS;
    static_assert(4 % NT == 0 && KSTEPS % KS == 0, "4 waves: NT channel tiles x KS whole K parts");
    extern __shared__ float sm[];
    float *xs = sm;                          // [CINP][kPlane]
    float *red = sm + CINP * kPlane;         // K-split partials [3 parts][3 mt][64 lanes][4] per channel tile
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nt = wave % NT, part = wave / NT;
    const int s0 = part * PER;
    const int row = lane & 15, kq = lane >> 4;
    // this wave's weights first: their loads are in flight while the planes stage
    const int co0 = 16 * NT * (int)blockIdx.y;
    const float *wl = wk + (size_t)(4 * s0 + kq) * coutp_all + co0 + nt * 16 + row;
    float bq[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) bq[i] = wl[(size_t)i * 4 * coutp_all];
    stage_planes_fast<CINP>(in + (size_t)b * cin * kCells, cin, xs);
    __syncthreads();
    // per-lane A base of each position tile, biased by the most negative tap
    // offset (-10) so every k-step's offset is a non-negative immediate.  Rows past
    // the 42 cells read cell 0: D row i depends only on A row i, and those rows are
    // never stored, so the k-loop has no select (a per-MFMA exec branch kept the
    // scheduler from running LDS reads ahead: one exposed LDS round trip per MFMA)
    const float *xb[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int p = mt * 16 + row;
        const int pp = p < kCells ? p : 0;
        xb[mt] = xs + kq * kPlane + (pp / kCols + 1) * 9 + pp % kCols + 1 - 10;
    }
    f32x4 acc[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the wave's K part as a compile-time constant: every LDS offset is an immediate
    auto kloop = [&](auto part_c) {
        constexpr int s0c = decltype(part_c)::value * PER;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int s = s0c + i, tap = s / CSN, cs = s % CSN;
            const int off = 4 * cs * kPlane + tap_off(tap) + 10;
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[mt][off], bq[i], acc[mt], 0, 0, 0);
        }
    };
    if constexpr (KS == 1) {
        kloop(std::integral_constant<int, 0>{});
    } else if constexpr (KS == 2) {
        if (part == 0) kloop(std::integral_constant<int, 0>{});
        else kloop(std::integral_constant<int, 1>{});
    } else {
        if (part == 0) kloop(std::integral_constant<int, 0>{});
        else if (part == 1) kloop(std::integral_constant<int, 1>{});
        else if (part == 2) kloop(std::integral_constant<int, 2>{});
        else kloop(std::integral_constant<int, 3>{});
    }
    if (KS > 1) {   // fixed-order sum of the K parts
        if (part > 0) {
            float *dst = red + (((part - 1) * 3) * 64 + lane) * 4 + nt * (3 * 3 * 64 * 4);
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[mt * 64 * 4 + r] = acc[mt][r];
        }
        __syncthreads();
        if (part == 0)
#pragma unroll
        for (int q = 1; q < KS; ++q) {
            const float *src = red + (((q - 1) * 3) * 64 + lane) * 4 + nt * (3 * 3 * 64 * 4);
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mt][r] += src[mt * 64 * 4 + r];
        }
    }
    const int n = co0 + nt * 16 + row;   // D[row = 4 kq + r][col = lane & 15]: col = channel, row = position
    // the waves that hold a finished tile (part 0).  A named flag: written into the `if`,
    // the short-circuit becomes control flow and the K-split kernels compile to other
    // code (the kernel's bytes are pinned, profiles/learner_bn_fuse_retirement)
    const bool live = (KS == 1 || part == 0) && n < cout;
    if (live) {
        const float bv = bias ? bias[n] : 0.f;
        float *ob = out + ((size_t)b * cout + n) * kCells;
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = mt * 16 + 4 * kq + r;
                if (p < kCells) {
                    const float v = acc[mt][r] + bv;
                    ob[p] = accumulate ? ob[p] + v : v;
                }
            }
    }
}

// weight-gradient partials: workgroup (chunk, group) accumulates, over the
// kWgSamples samples of its chunk, the output tiles of its tile group:
//   part[chunk][n][k] = sum_{b in chunk} sum_p dz[b][n][p] * X[b][p][k]   (k tap-major over CINP)
// (the conv bias gradient, sum dz, comes out of the BN backward, k_bn_bwd)
// GEMM rows = output channels (coutp/16 tiles), columns = k (round16(9 CINP)/16
// tiles), reduction = each sample's 42 positions (11 k-steps of 4).
constexpr int kWgSamples = 4;
constexpr int kWgMaxTiles = 3;   // tiles per wave (144 tiles / 12 groups / 4 waves at 64 x 64: 384 workgroups at B = 128)
template <int CINP>
__global__ __launch_bounds__(kThreads) void k_wgrad_mfma(const float *__restrict__ x, int cin,
                                                         const float *__restrict__ dz, int cout, int B, int groups,
                                                         float *__restrict__ part) {
    constexpr int K = 9 * CINP, Kp = (K + 15) & ~15, NK = Kp / 16;
    extern __shared__ float sm[];
    const int coutp = round16(cout), NTo = coutp / 16, ntiles = NTo * NK;
    float *xs = sm;                        // [CINP][kPlane]
    float *ds = sm + CINP * kPlane;        // [coutp][44], zero past 42 and past cout
    // the end of the LDS in use, computed here: with coutp * 44 first evaluated in the
    // zero fill below, the compiler orders the prologue's scalar code differently
    // (the kernel's bytes are pinned, profiles/learner_bn_fuse_retirement)
    const float *sm_end = ds + coutp * 44;
    const int chunk = blockIdx.x, group = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, kq = lane >> 4;
    // this wave's tiles: group's range [t0, t1), wave-strided
    const int t0 = ntiles * group / groups, t1 = ntiles * (group + 1) / groups;
    // positions past the 42 cells read cell 0's plane entry: their dz (A) is zero
    // in ds, so the products are exact zeros, and the k-loop needs no select
    int pb[11];
#pragma unroll
    for (int s = 0; s < 11; ++s) {
        const int p = 4 * s + kq;
        const int pp = p < kCells ? p : 0;
        pb[s] = (pp / kCols + 1) * 9 + pp % kCols + 1;
    }
    f32x4 acc[kWgMaxTiles];
#pragma unroll
    for (int j = 0; j < kWgMaxTiles; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int b0 = chunk * kWgSamples, b1 = min(B, b0 + kWgSamples);
    // Staging: the zero borders of the planes, the padding channels and the dz
    // padding (positions 42, 43, rows >= cout) are written once; each sample then
    // copies only its cin x 42 inputs and cout x 42 dz values, both contiguous in
    // memory (coalesced loads at immediate offsets), to LDS destinations computed
    // once per workgroup.  The next sample's values are loaded into registers
    // while the current sample's MFMAs run.
    constexpr int NX = (CINP * kCells + kThreads - 1) / kThreads;   // 11 at 64 channels
    constexpr int ND = (64 * kCells + kThreads - 1) / kThreads;     // cout <= 64
    const int nx = cin * kCells, nd = cout * kCells;
    for (int i = threadIdx.x; i < (int)(sm_end - sm); i += kThreads) sm[i] = 0.f;
    int dx[NX], dd[ND];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        const int i = threadIdx.x + j * kThreads, c = i / kCells, cell = i - c * kCells;
        dx[j] = i < nx ? c * kPlane + (cell / kCols + 1) * 9 + cell % kCols + 1 : 0;   // 0: a border cell (gets 0)
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        const int i = threadIdx.x + j * kThreads, n = i / kCells, p = i - n * kCells;
        dd[j] = i < nd ? CINP * kPlane + n * 44 + p : CINP * kPlane + kCells;   // a zero pad (gets 0)
    }
    float vx[NX], vd[ND];
    auto load = [&](int b) {
        const float *xb = x + (size_t)b * nx, *db = dz + (size_t)b * nd;
#pragma unroll
        for (int j = 0; j < NX; ++j) vx[j] = threadIdx.x + j * kThreads < nx ? xb[threadIdx.x + j * kThreads] : 0.f;
#pragma unroll
        for (int j = 0; j < ND; ++j) vd[j] = threadIdx.x + j * kThreads < nd ? db[threadIdx.x + j * kThreads] : 0.f;
    };
    load(b0);
    __syncthreads();   // the zero fill lands before any sample's values
    for (int b = b0; b < b1; ++b) {
#pragma unroll
        for (int j = 0; j < NX; ++j) sm[dx[j]] = vx[j];   // past the inputs: a 0 into a zero cell
#pragma unroll
        for (int j = 0; j < ND; ++j) sm[dd[j]] = vd[j];
        __syncthreads();
        if (b + 1 < b1) load(b + 1);
#pragma unroll
        for (int j = 0; j < kWgMaxTiles; ++j) {
            const int t = t0 + wave + 4 * j;
            if (t >= t1) break;
            const int mt = t / NK, kt = t - mt * NK;
            const float *arow = ds + (mt * 16 + row) * 44;    // A[m = channel][kk = position]
            const int k = kt * 16 + row;                      // B[kk = position][n = k]
            const bool kval = k < K;
            const int tap = k / CINP, c = k % CINP;           // CINP: compile-time
            // a padding column (k >= K) reads position data too: its D column is never stored
            const float *xcol = xs + (kval ? c * kPlane + tap_off(tap) : 0);
#pragma unroll
            for (int s = 0; s < 11; ++s) {
                const float av = arow[4 * s + kq];
                const float bv = xcol[pb[s]];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();   // xs / ds are restaged for the next sample
    }
#pragma unroll
    for (int j = 0; j < kWgMaxTiles; ++j) {
        const int t = t0 + wave + 4 * j;
        if (t >= t1) break;
        const int mt = t / NK, kt = t - mt * NK;
        const int k = kt * 16 + row;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = mt * 16 + 4 * kq + r;
            if (n < cout && k < K) part[((size_t)chunk * cout + n) * K + k] = acc[j][r];
        }
    }
}

// dW[n][c][tap] = sum_chunk part[chunk][n][tap * cinp + c]  (fixed order).  At
// batch 128 there are 32 chunks: all 32 loads in flight at once, and 64-thread
// workgroups (576 of them for 64 x 64, instead of 144 of 256 threads on 256 CUs)
constexpr int kWgReduceBatch = 32, kWgReduceThreads = 64;
__global__ void k_wgrad_reduce(const float *__restrict__ part, int B, int cin, int cout, float *__restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int cinp = round4(cin), K = 9 * cinp;
    if (i < cout * K) {   // i = n * K + k: consecutive threads read consecutive partials (coalesced)
        const int n = i / K, k = i - n * K, tap = k / cinp, c = k - tap * cinp;
        if (c < cin) {
            const float *src = part + i;
            const size_t stride = (size_t)cout * K;
            float s = 0.f;
            for (int b0 = 0; b0 < B; b0 += kWgReduceBatch) {   // kWgReduceBatch loads in flight, summed in batch order
                float v[kWgReduceBatch];
#pragma unroll
                for (int j = 0; j < kWgReduceBatch; ++j) v[j] = b0 + j < B ? src[(size_t)(b0 + j) * stride] : 0.f;
#pragma unroll
                for (int j = 0; j < kWgReduceBatch; ++j)
                    if (b0 + j < B) s += v[j];
            }
            dw[((size_t)n * cin + c) * 9 + tap] = s;
        }
    }
}

// ------------------------------------------------------------------ batch norm
// One workgroup of kBn threads per channel.  A channel's B x 42 values are read
// once into registers (kBnPer per thread; batches past kBn * kBnPer = 6144
// values, B > 146, re-read the rest from memory), so the two-pass statistics
// and the output cost one memory pass.  Sums: fixed-order wave shuffles, then
// the 16 wave partials in order (deterministic).
constexpr int kBn = 1024, kBnPer = 6;
__device__ __forceinline__ float bn_block_sum(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kBn / 64; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ size_t bn_at(int i, int c, int c_n) {
    return ((size_t)(i / kCells) * c_n + c) * kCells + i % kCells;
}

// forward in train mode, per channel: batch mean and biased variance over
// (B, 42) (two passes over the registers), invstd = 1/sqrt(var + eps); running
// stats r = (1 - m) r + m * stat (unbiased var); a = relu(gamma * (z - mean) *
// invstd + beta [+ res])
__global__ __launch_bounds__(kBn) void k_bn_fwd(const float *__restrict__ z, int c_n, int B, float eps,
                                                float momentum, float *__restrict__ mean, float *__restrict__ invstd,
                                                float *__restrict__ run_mean, float *__restrict__ run_var,
                                                const float *__restrict__ gamma, const float *__restrict__ beta,
                                                const float *__restrict__ res, float *__restrict__ a) {
    __shared__ float red[2][kBn / 64];
    const int c = blockIdx.x, n = B * kCells;
    float v[kBnPer];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kBnPer; ++j) {
        const int i = threadIdx.x + j * kBn;
        v[j] = i < n ? z[bn_at(i, c, c_n)] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kBnPer; ++j) s += v[j];
    for (int i = threadIdx.x + kBnPer * kBn; i < n; i += kBn) s += z[bn_at(i, c, c_n)];
    const float mu = bn_block_sum(s, red[0]) / (float)n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < kBnPer; ++j)
        if (threadIdx.x + j * kBn < n) q += (v[j] - mu) * (v[j] - mu);
    for (int i = threadIdx.x + kBnPer * kBn; i < n; i += kBn) {
        const float d = z[bn_at(i, c, c_n)] - mu;
        q += d * d;
    }
    const float var = bn_block_sum(q, red[1]) / (float)n;
    const float is = 1.0f / sqrtf(var + eps);
    if (threadIdx.x == 0) {
        mean[c] = mu;
        invstd[c] = is;
        run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mu;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (n > 1 ? var * (float)n / (float)(n - 1) : var);
    }
    const float ga = gamma[c], be = beta[c];
    auto out = [&](int i, float zi) {
        const size_t k = bn_at(i, c, c_n);
        float y = ga * ((zi - mu) * is) + be;
        if (res) y += res[k];
        a[k] = fmaxf(y, 0.f);
    };
#pragma unroll
    for (int j = 0; j < kBnPer; ++j)
        if (threadIdx.x + j * kBn < n) out(threadIdx.x + j * kBn, v[j]);
    for (int i = threadIdx.x + kBnPer * kBn; i < n; i += kBn) out(i, z[bn_at(i, c, c_n)]);
}

// backward of a = relu(bn(z) [+ res]): dy = da * (a > 0); per channel
// dbeta = sum dy, dgamma = sum dy * xhat;  dz = gamma*invstd/N * (N dy - dbeta - xhat dgamma);
// the conv bias gradient dbias = sum dz (zero up to rounding: the conv feeds the BN);
// dy_out (optional) = dy, the residual block's skip-path gradient.  dz may be z
// itself (every element is read and written by the same thread)
__global__ __launch_bounds__(kBn) void k_bn_bwd(const float *__restrict__ da, const float *__restrict__ a,
                                                const float *z, int c_n, int B,
                                                const float *__restrict__ mean, const float *__restrict__ invstd,
                                                const float *__restrict__ gamma, float *__restrict__ dgamma,
                                                float *__restrict__ dbeta, float *__restrict__ dbias, float *dz,
                                                float *__restrict__ dy_out) {
    __shared__ float red[3][kBn / 64];
    const int c = blockIdx.x, n = B * kCells;
    const float mu = mean[c], is = invstd[c];
    float dy[kBnPer], xh[kBnPer];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < kBnPer; ++j) {
        const int i = threadIdx.x + j * kBn;
        const bool ok = i < n;
        const size_t k = ok ? bn_at(i, c, c_n) : 0;
        const float vd = ok ? da[k] : 0.f, va = ok ? a[k] : 0.f, vz = ok ? z[k] : mu;
        dy[j] = va > 0.f ? vd : 0.f;
        xh[j] = (vz - mu) * is;
    }
#pragma unroll
    for (int j = 0; j < kBnPer; ++j) {
        s1 += dy[j];
        s2 += dy[j] * xh[j];
    }
    for (int i = threadIdx.x + kBnPer * kBn; i < n; i += kBn) {
        const size_t k = bn_at(i, c, c_n);
        const float d = a[k] > 0.f ? da[k] : 0.f;
        s1 += d;
        s2 += d * ((z[k] - mu) * is);
    }
    const float sb = bn_block_sum(s1, red[0]), sg = bn_block_sum(s2, red[1]);
    const float g = gamma[c] * is / (float)n;
    float s3 = 0.f;
    auto out = [&](int i, float d, float x) {
        const size_t k = bn_at(i, c, c_n);
        const float v = g * ((float)n * d - sb - x * sg);
        dz[k] = v;
        if (dy_out) dy_out[k] = d;
        s3 += v;
    };
#pragma unroll
    for (int j = 0; j < kBnPer; ++j)
        if (threadIdx.x + j * kBn < n) out(threadIdx.x + j * kBn, dy[j], xh[j]);
    for (int i = threadIdx.x + kBnPer * kBn; i < n; i += kBn) {
        const size_t k = bn_at(i, c, c_n);
        out(i, a[k] > 0.f ? da[k] : 0.f, (z[k] - mu) * is);
    }
    const float sz = bn_block_sum(s3, red[2]);
    if (threadIdx.x == 0) {
        dbeta[c] = sb;
        dgamma[c] = sg;
        dbias[c] = sz;
    }
}

// ------------------------------------------------------------------ heads + loss

// one workgroup per sample: policy logits (1344 -> 7), value (126 -> 1, tanh),
// loss terms and the output gradients
//   dlogits = (softmax * sum(pi) - pi) / B,  dpre = 2 (v - z) / B * (1 - v^2)
__global__ __launch_bounds__(kThreads) void k_heads_loss(const float *__restrict__ rp, const float *__restrict__ rv,
                                                         const float *__restrict__ wp, const float *__restrict__ bp,
                                                         const float *__restrict__ wv, const float *__restrict__ bv,
                                                         const float *__restrict__ pi, const float *__restrict__ zv,
                                                         int B, float *__restrict__ dlogits, float *__restrict__ dpre,
                                                         float *__restrict__ loss_terms) {
    __shared__ float part[kThreads / 64][8];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *xp = rp + (size_t)b * 32 * kCells, *xv = rv + (size_t)b * 3 * kCells;
    // one pass over the features: 7 policy logits and the value pre-activation at
    // once; wave sums by shuffles, then the 4 wave partials in order
    float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = threadIdx.x; k < 32 * kCells; k += kThreads) {
        const float xk = xp[k];
#pragma unroll
        for (int o = 0; o < 7; ++o) acc8[o] += xk * wp[o * 32 * kCells + k];
    }
    for (int k = threadIdx.x; k < 3 * kCells; k += kThreads) acc8[7] += xv[k] * wv[k];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) acc8[o] += __shfl_xor(acc8[o], sh, 64);
    }
    if (lane == 0)
#pragma unroll
        for (int o = 0; o < 8; ++o) part[wave][o] = acc8[o];
    __syncthreads();
    float lg[7];
#pragma unroll
    for (int o = 0; o < 7; ++o) lg[o] = ((part[0][o] + part[1][o]) + part[2][o]) + part[3][o] + bp[o];
    const float pre = ((part[0][7] + part[1][7]) + part[2][7]) + part[3][7] + bv[0];
    if (threadIdx.x == 0) {
        float mx = lg[0];
        for (int o = 1; o < 7; ++o) mx = fmaxf(mx, lg[o]);
        float se = 0.f;
        for (int o = 0; o < 7; ++o) se += expf(lg[o] - mx);
        const float lse = mx + logf(se);
        float nll = 0.f, spi = 0.f;
        for (int o = 0; o < 7; ++o) {
            nll += (lg[o] - lse) * pi[b * 7 + o];
            spi += pi[b * 7 + o];
        }
        for (int o = 0; o < 7; ++o) dlogits[b * 7 + o] = (expf(lg[o] - lse) * spi - pi[b * 7 + o]) / (float)B;
        const float v = tanhf(pre), d = v - zv[b];
        dpre[b] = 2.0f * d / (float)B * (1.0f - v * v);
        loss_terms[2 * b] = -nll;      // policy term of sample b
        loss_terms[2 * b + 1] = d * d; // value term
    }
}

// linear backward, out features O, in features K:
//   dW[o][k] = sum_b dy[b][o] x[b][k];  db[o] = sum_b dy[b][o];  dx[b][k] = sum_o dy[b][o] W[o][k]
// dw[o][k] = sum_b dy[b][o] x[b][k], db[o] = sum_b dy[b][o].  A workgroup owns 64
// outputs; its 4 waves take a quarter of the batch each (16 loads in flight),
// and the quarters are added in order through LDS.
__global__ __launch_bounds__(kThreads) void k_linear_bwd_w(const float *__restrict__ x, const float *__restrict__ dy,
                                                           int B, int O, int K, float *__restrict__ dw,
                                                           float *__restrict__ db) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int bq0 = B * q / 4, bq1 = B * (q + 1) / 4;
    float s = 0.f;
    if (i < O * K) {
        const int o = i / K, k = i - o * K;
        for (int b0 = bq0; b0 < bq1; b0 += 16) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = b0 + j < bq1 ? x[(size_t)(b0 + j) * K + k] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (b0 + j < bq1) s += dy[(b0 + j) * O + o] * v[j];
        }
    }
    part[q][lane] = s;
    __syncthreads();
    if (q == 0 && i < O * K) dw[i] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    if (blockIdx.x == 0 && q == 1 && lane < O) {   // db: 16 loads in flight, summed in batch order
        float t = 0.f;
        for (int b0 = 0; b0 < B; b0 += 16) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = b0 + j < B ? dy[(b0 + j) * O + lane] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) t += v[j];
        }
        db[lane] = t;
    }
}
__global__ void k_linear_bwd_x(const float *__restrict__ dy, const float *__restrict__ w, int B, int O, int K,
                               float *__restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * K) return;
    const int b = (int)(i / K), k = (int)(i - (size_t)b * K);
    float s = 0.f;
    for (int o = 0; o < O; ++o) s += dy[b * O + o] * w[o * K + k];
    dx[i] = s;
}

// ------------------------------------------------------------------ Adam (torch semantics)
// m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
// p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)      (g scaled by gscale)
// bc = {1 - b1^t, sqrt(1 - b2^t)} for this step (host-computed, staged with the batch)
__global__ void k_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                       float *__restrict__ v, size_t n, float gscale, float lr, float b1, float b2, float eps,
                       const float *__restrict__ bc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float bc1 = bc[0], bc2_sqrt = bc[1];
    const float gi = g[i] * gscale;
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

// data-parallel weighting: this rank's mean gradient times B_rank / sum over ranks of B
__global__ void k_weight_grad(float *__restrict__ g, size_t n, float b_local, const float *__restrict__ b_sum) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g[i] *= b_local / b_sum[0];
}

__global__ void k_set1(float *__restrict__ dst, float v) { *dst = v; }

// running stats gathered into / scattered from a packed buffer (cross-rank average)
__global__ void k_gather(const float *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t n,
                         float *__restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
__global__ void k_scatter_scaled(const float *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t n,
                                 float scale, float *__restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[idx[i]] = src[i] * scale;
}

inline unsigned blocks_of(size_t n, int t = kThreads) { return (unsigned)((n + t - 1) / t); }

}  // namespace
}  // namespace spai

// ---------------------------------------------------------------------- host
namespace spai {
namespace {

int learner_alloc_batch(spai_learner *L, uint32_t B) {
    if (B <= L->max_batch) return SPAI_OK;
    const size_t act = (size_t)B * std::max(L->hidden, 32) * kCells;   // also the 32-channel policy head
    SPAI_TRY(L->batch_in.alloc((size_t)B * (3 * kCells + 8) + 2));
    for (float **h : {&L->stage, &L->stage_b}) {
        if (*h) (void)hipHostFree(*h);
        *h = nullptr;
        if (hipHostMalloc((void **)h, ((size_t)B * (3 * kCells + 10) + 2) * sizeof(float), hipHostMallocDefault) !=
            hipSuccess) {
            *h = nullptr;
            set_error("learner: pinned staging allocation failed");
            return SPAI_ERR_DEVICE;
        }
    }
    for (size_t l = 0; l < L->convs.size(); ++l) {
        SPAI_TRY(L->z[l].alloc((size_t)B * L->convs[l].co * kCells));
        SPAI_TRY(L->a[l].alloc((size_t)B * L->convs[l].co * kCells));
    }
    SPAI_TRY(L->d0.alloc(act));
    SPAI_TRY(L->d1.alloc(act));
    SPAI_TRY(L->dlogits.alloc((size_t)B * 7));
    SPAI_TRY(L->dpre.alloc(B));
    SPAI_TRY(L->loss_terms.alloc((size_t)B * 2));
    const size_t cmax = (size_t)std::max(L->hidden, 32);
    for (auto &w : L->wpart_side)   // weight-gradient partials per chunk (one buffer per side stream)
        SPAI_TRY(w.alloc((size_t)((B + kWgSamples - 1) / kWgSamples) * cmax * 9 * round4(L->hidden)));
    L->max_batch = B;
    return SPAI_OK;
}

// out (+)= conv(in) on f32 MFMA with a packed weight matrix wk (forward or
// data-gradient orientation, k_pack_all).  The learner's shapes: input channels
// 3 (-> 4), 32 or 64; output 3 (1 tile), 32 (2) or 64 (4).  Where the k-steps
// split into 4 whole parts (32 and 64 input channels) every 16-channel tile is
// its own workgroup with the K split over its 4 waves (grid B x coutp/16: 4x
// the workgroups of one per sample); the stem's input (4 padded channels, 9
// k-steps) keeps one workgroup per sample with a wave per channel tile.
// (Two samples per workgroup on one set of weight registers was measured slower:
// 12.7 against 10.9 us per conv, 181k against 189k samples/s -- its 272 registers
// leave one workgroup per CU, whose staging, k-loop and K-part sum then run back to
// back instead of overlapping another workgroup's; profiles/r05/learner/spw.)

template <int CINP>
int launch_conv_t(int B, hipStream_t st, const float *in, int cin, const float *wk, const float *bias, int cout,
                  float *out, int acc) {
    constexpr int ks = 9 * CINP / 4;
    const size_t lds = ((size_t)CINP * kPlane + 2 * 2304) * sizeof(float);
    const int nt = round16(cout) / 16;
    if constexpr (ks % 4 == 0) {
        k_conv_mfma<CINP, 1><<<dim3(B, nt), kThreads, lds, st>>>(in, cin, wk, bias, cout, 16 * nt, out, acc);
        return SPAI_OK;
    } else {
        if (nt == 4) {
            k_conv_mfma<CINP, 4><<<dim3(B), kThreads, lds, st>>>(in, cin, wk, bias, cout, 64, out, acc);
            return SPAI_OK;
        }
        set_error("learner conv: %d input / %d output channels not built", cin, cout);
        return SPAI_ERR_UNSUPPORTED;
    }
}

int launch_conv(const float *in, int cin, const float *wk, const float *bias, int cout, float *out, int B, bool acc,
                hipStream_t st) {
    const int a = acc ? 1 : 0;
    switch (round4(cin)) {
    case 4: return launch_conv_t<4>(B, st, in, cin, wk, bias, cout, out, a);
    case 32: return launch_conv_t<32>(B, st, in, cin, wk, bias, cout, out, a);
    case 64: return launch_conv_t<64>(B, st, in, cin, wk, bias, cout, out, a);
    default: set_error("learner conv: %d input channels not built", cin); return SPAI_ERR_UNSUPPORTED;
    }
}

// dW of one conv: chunk partials on f32 MFMA, then a fixed-order sum over the chunks
int launch_wgrad(float *wpart, const float *x, int cin, const float *dz, int cout, int B, float *dw, hipStream_t st) {
    const int cinp = round4(cin), k = 9 * cinp, nk = (k + 15) / 16, ntiles = (round16(cout) / 16) * nk;
    const int groups = std::max(1, (ntiles + 4 * kWgMaxTiles - 1) / (4 * kWgMaxTiles));
    const int chunks = (B + kWgSamples - 1) / kWgSamples;
    const size_t lds = ((size_t)cinp * kPlane + (size_t)round16(cout) * 44) * sizeof(float);
    const dim3 grid(chunks, groups);
    switch (cinp) {
    case 4: k_wgrad_mfma<4><<<grid, kThreads, lds, st>>>(x, cin, dz, cout, B, groups, wpart); break;
    case 64: k_wgrad_mfma<64><<<grid, kThreads, lds, st>>>(x, cin, dz, cout, B, groups, wpart); break;
    default: set_error("learner wgrad: %d input channels not built", cin); return SPAI_ERR_UNSUPPORTED;
    }
    k_wgrad_reduce<<<blocks_of((size_t)cout * k, kWgReduceThreads), kWgReduceThreads, 0, st>>>(wpart, chunks, cin, cout,
                                                                                              dw);
    return SPAI_OK;
}

}  // namespace

int learner_create(spai_engine *e, int blocks, int hidden, const float *params, size_t n, const spai_adam_config *cfg,
                   spai_learner **out) {
    SPAI_CHECK(e->game == SPAI_GAME_CONNECT4, SPAI_ERR_UNSUPPORTED, "learner: only Connect4 is built");
    SPAI_CHECK(hidden == 64, SPAI_ERR_UNSUPPORTED, "learner: hidden must be 64 (got %d)", hidden);
    SPAI_CHECK(blocks >= 0 && blocks <= 40, SPAI_ERR_UNSUPPORTED, "learner: 0..40 blocks (got %d)", blocks);
    SPAI_CHECK(params && n == net_num_params(e->game, blocks, hidden), SPAI_ERR_INVALID, "expected %zu params, got %zu",
               net_num_params(e->game, blocks, hidden), n);
    SPAI_TRY(validate_adam_config(cfg));
    spai_learner *L = new spai_learner();
    L->eng = e;
    L->blocks = blocks;
    L->hidden = hidden;
    if (cfg) L->cfg = *cfg;
    else spai_adam_config_default(&L->cfg);
    size_t off = 0;
    auto conv = [&](int ci, int co) {
        spai_learner::Conv c{ci, co, 0, 0, 0, 0, 0, 0, 0, 0};
        c.w = off;
        off += (size_t)co * ci * 9;
        c.b = off;
        off += co;
        c.g = off;
        c.be = off + co;
        c.mu = off + 2 * co;
        c.var = off + 3 * co;
        off += 4 * (size_t)co;
        L->convs.push_back(c);
    };
    conv(3, hidden);
    for (int i = 0; i < 2 * blocks; ++i) conv(hidden, hidden);
    conv(hidden, 32);
    L->pol_w = off;
    off += 7 * 32 * kCells;
    L->pol_b = off;
    off += 7;
    conv(hidden, 3);
    L->val_w = off;
    off += 3 * kCells;
    L->val_b = off;
    off += 1;
    L->n_params = off;
    int rc = SPAI_OK;
    auto chk = [&](int r) {
        if (rc == SPAI_OK) rc = r;
    };
    chk(L->p.alloc(n));
    chk(L->g.alloc(n));
    chk(L->bsum.alloc(1));
    chk(L->m.alloc(n));
    chk(L->v.alloc(n));
    {   // packed [k][n] matrices: every conv forward, every conv but the stem data gradient
        std::vector<uint32_t> desc;
        size_t woff = 0;
        auto entry = [&](size_t wparam, int cin, int cout, int dgrad) {
            const int cinp = round4(cin), coutp = round16(cout);
            desc.insert(desc.end(), {(uint32_t)wparam, (uint32_t)cin, (uint32_t)cout, (uint32_t)cinp, (uint32_t)coutp,
                                     (uint32_t)dgrad, (uint32_t)woff, 0u});
            woff += (size_t)9 * cinp * coutp;
            return woff - (size_t)9 * cinp * coutp;
        };
        for (size_t l = 0; l < L->convs.size(); ++l) {
            spai_learner::Conv &c = L->convs[l];
            c.wk = entry(c.w, c.ci, c.co, 0);
            c.wkd = l == 0 ? 0 : entry(c.w, c.co, c.ci, 1);
        }
        L->n_pack = (int)(desc.size() / kPackDesc);
        chk(L->wt.alloc(woff));
        chk(L->pack_desc.alloc(desc.size()));
        if (rc == SPAI_OK &&
            hipMemcpy(L->pack_desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
            set_error("learner: upload failed");
            rc = SPAI_ERR_DEVICE;
        }
    }
    L->z.resize(L->convs.size());
    L->a.resize(L->convs.size());
    L->mean.resize(L->convs.size());
    L->invstd.resize(L->convs.size());
    std::vector<uint32_t> ridx;
    for (size_t l = 0; l < L->convs.size(); ++l) {
        chk(L->mean[l].alloc(L->convs[l].co));
        chk(L->invstd[l].alloc(L->convs[l].co));
        for (int c = 0; c < L->convs[l].co; ++c) ridx.push_back((uint32_t)(L->convs[l].mu + c));
        for (int c = 0; c < L->convs[l].co; ++c) ridx.push_back((uint32_t)(L->convs[l].var + c));
    }
    chk(L->run_idx.alloc(ridx.size()));
    L->ev_dz.assign(L->convs.size(), nullptr);
    for (int k = 0; k < spai_learner::kWgStreams; ++k)
        if (rc == SPAI_OK && (hipStreamCreateWithFlags(&L->wg_stream[k], hipStreamNonBlocking) != hipSuccess ||
                              hipEventCreateWithFlags(&L->ev_wg_done[k], hipEventDisableTiming) != hipSuccess)) {
            set_error("learner: stream/event creation failed");
            rc = SPAI_ERR_DEVICE;
        }
    for (auto &ev : L->stage_ev)
        if (rc == SPAI_OK && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            set_error("learner: event creation failed");
            rc = SPAI_ERR_DEVICE;
        }
    for (auto &ev : L->ev_dz)
        if (rc == SPAI_OK && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            set_error("learner: event creation failed");
            rc = SPAI_ERR_DEVICE;
        }
    chk(L->run_buf.alloc(ridx.size()));
    if (rc == SPAI_OK) {
        hipStream_t st = e->stream;
        if (hipMemcpyAsync(L->p.p, params, n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(L->run_idx.p, ridx.data(), ridx.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemsetAsync(L->m.p, 0, n * 4, st) != hipSuccess || hipMemsetAsync(L->v.p, 0, n * 4, st) != hipSuccess ||
            hipMemsetAsync(L->g.p, 0, n * 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            set_error("learner: upload failed");
            rc = SPAI_ERR_DEVICE;
        }
    }
    if (rc != SPAI_OK) {
        learner_destroy(L);
        return rc;
    }
    *out = L;
    return SPAI_OK;
}

void learner_destroy(spai_learner *L) {
    if (!L) return;
    if (L->eng) (void)hipStreamSynchronize(L->eng->stream);
    for (hipStream_t ws : L->wg_stream)
        if (ws) (void)hipStreamSynchronize(ws);
    if (L->comm) (void)ncclCommDestroy((ncclComm_t)L->comm);
    for (hipEvent_t ev : L->ev_dz)
        if (ev) (void)hipEventDestroy(ev);
    for (int k = 0; k < spai_learner::kWgStreams; ++k) {
        if (L->ev_wg_done[k]) (void)hipEventDestroy(L->ev_wg_done[k]);
        if (L->wg_stream[k]) (void)hipStreamDestroy(L->wg_stream[k]);
        L->wpart_side[k].release();
    }
    L->pack_desc.release();
    if (L->stage) (void)hipHostFree(L->stage);
    if (L->stage_b) (void)hipHostFree(L->stage_b);
    if (L->terms_host) (void)hipHostFree(L->terms_host);
    for (hipEvent_t ev : L->stage_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (L->host_buf) (void)hipHostFree(L->host_buf);
    for (auto *b : {&L->p, &L->g, &L->bsum, &L->m, &L->v, &L->wt, &L->batch_in, &L->d0, &L->d1, &L->dlogits, &L->dpre,
                    &L->loss_terms, &L->run_buf})
        b->release();
    L->run_idx.release();
    for (auto *vec : {&L->z, &L->a, &L->mean, &L->invstd})
        for (auto &b : *vec) b.release();
    delete L;
}

// One cross-rank sum of n device floats, in place, in stream order: RCCL over
// xGMI, or the caller's host collective (spai_learner_set_host_comm) through the
// pinned staging buffer, which blocks the calling thread until every rank arrived.
static int learner_allreduce(spai_learner *L, float *buf, size_t n, hipStream_t st, const char *what) {
    if (L->comm) {
        if (ncclAllReduce(buf, buf, n, ncclFloat32, ncclSum, (ncclComm_t)L->comm, st) != ncclSuccess) {
            set_error("ncclAllReduce of %s failed", what);
            return SPAI_ERR_DEVICE;
        }
        return SPAI_OK;
    }
    SPAI_CHECK(L->host_ar && n <= L->host_buf_n, SPAI_ERR_INVALID, "host all-reduce of %s: no collective", what);
    SPAI_HIP(hipMemcpyAsync(L->host_buf, buf, n * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    const int r = L->host_ar(L->host_ar_user, L->host_buf, n);
    SPAI_CHECK(r == 0, SPAI_ERR_DEVICE, "host all-reduce of %s failed (%d)", what, r);
    SPAI_HIP(hipMemcpyAsync(buf, L->host_buf, n * 4, hipMemcpyHostToDevice, st));
    return SPAI_OK;
}

// Everything of one train step after the batch upload: gradients zeroed, weights
// packed, forward, loss, backward (weight gradients on the side streams), the cross-rank
// reduction when there is a communicator, Adam.  Launch-only (no host sync).
int enqueue_step(spai_learner *L, uint32_t B, hipStream_t st, const float *x_in, const float *pi_in,
                 const float *z_in, const float *bc) {
    float *P = L->p.p, *G = L->g.p;
    // G needs no clearing: every trainable entry is written (not accumulated) by
    // this step's kernels, and the BN running-statistic entries stay at the zero
    // they got at learner_create
    const float eps = L->cfg.bn_eps, mom = L->cfg.bn_momentum;
    const size_t nl = L->convs.size();
    k_pack_all<<<dim3(blocks_of((size_t)9 * 64 * 64), L->n_pack), kThreads, 0, st>>>(P, L->pack_desc.p, L->wt.p);
    const float *W = L->wt.p;
    const int pol = (int)nl - 2, val = (int)nl - 1;

    // ---------------- forward (train mode)
    int crc = SPAI_OK;   // conv launch status (shape dispatch)
    auto conv_bn_act = [&](int l, const float *in, const float *res) {
        const spai_learner::Conv &c = L->convs[l];
        if (crc == SPAI_OK) crc = launch_conv(in, c.ci, W + c.wk, P + c.b, c.co, L->z[l].p, (int)B, false, st);
        k_bn_fwd<<<c.co, kBn, 0, st>>>(L->z[l].p, c.co, (int)B, eps, mom, L->mean[l].p, L->invstd[l].p, P + c.mu,
                                       P + c.var, P + c.g, P + c.be, res, L->a[l].p);
    };
    conv_bn_act(0, x_in, nullptr);
    const float *h = L->a[0].p;
    for (int k = 0; k < L->blocks; ++k) {   // relu(h + BN(conv(relu(BN(conv(h)))))) (model/mod.rs:152-165)
        conv_bn_act(1 + 2 * k, h, nullptr);
        conv_bn_act(2 + 2 * k, L->a[1 + 2 * k].p, h);
        h = L->a[2 + 2 * k].p;
    }
    conv_bn_act(pol, h, nullptr);
    conv_bn_act(val, h, nullptr);
    k_heads_loss<<<B, kThreads, 0, st>>>(L->a[pol].p, L->a[val].p, P + L->pol_w, P + L->pol_b, P + L->val_w,
                                         P + L->val_b, pi_in, z_in, (int)B, L->dlogits.p, L->dpre.p, L->loss_terms.p);

    // ---------------- backward
    // heads: linears -> relu/BN -> conv; dh (d0) = dgrad(policy) + dgrad(value)
    k_linear_bwd_w<<<(7 * 32 * kCells + 63) / 64, kThreads, 0, st>>>(L->a[pol].p, L->dlogits.p, (int)B, 7, 32 * kCells,
                                                                     G + L->pol_w, G + L->pol_b);
    k_linear_bwd_x<<<blocks_of((size_t)B * 32 * kCells), kThreads, 0, st>>>(L->dlogits.p, P + L->pol_w, (int)B, 7,
                                                                             32 * kCells, L->d1.p);
    // conv l's dz (written over z[l] by k_bn_bwd) feeds its data gradient here and
    // its weight gradient on a side stream; nothing rewrites z[l] before the next step
    constexpr int kWgSide = spai_learner::kWgStreams;   // side streams the weight gradients rotate over
    int side = 0;
    auto wgrad_async = [&](int l, const float *in) {
        const spai_learner::Conv &c = L->convs[l];
        if (crc != SPAI_OK) return;
        const int k = side++ % kWgSide;
        if (hipEventRecord(L->ev_dz[l], st) != hipSuccess ||
            hipStreamWaitEvent(L->wg_stream[k], L->ev_dz[l], 0) != hipSuccess) {
            set_error("learner: event record/wait failed");
            crc = SPAI_ERR_DEVICE;
            return;
        }
        crc = launch_wgrad(L->wpart_side[k].p, in, c.ci, L->z[l].p, c.co, (int)B, G + c.w, L->wg_stream[k]);
    };
    auto bn_conv_bwd = [&](int l, const float *da, const float *in, float *dx, bool acc, float *dy_out) {
        const spai_learner::Conv &c = L->convs[l];
        k_bn_bwd<<<c.co, kBn, 0, st>>>(da, L->a[l].p, L->z[l].p, c.co, (int)B, L->mean[l].p, L->invstd[l].p,
                                       P + c.g, G + c.g, G + c.be, G + c.b, L->z[l].p, dy_out);
        wgrad_async(l, in);
        if (dx && crc == SPAI_OK) crc = launch_conv(L->z[l].p, c.co, W + c.wkd, nullptr, c.ci, dx, (int)B, acc, st);
    };
    bn_conv_bwd(pol, L->d1.p, h, L->d0.p, false, nullptr);
    k_linear_bwd_w<<<(3 * kCells + 63) / 64, kThreads, 0, st>>>(L->a[val].p, L->dpre.p, (int)B, 1, 3 * kCells,
                                                                G + L->val_w, G + L->val_b);
    k_linear_bwd_x<<<blocks_of((size_t)B * 3 * kCells), kThreads, 0, st>>>(L->dpre.p, P + L->val_w, (int)B, 1,
                                                                            3 * kCells, L->d1.p);
    bn_conv_bwd(val, L->d1.p, h, L->d0.p, true, nullptr);
    // residual blocks in reverse; d0 holds dL/d(block output)
    for (int k = L->blocks - 1; k >= 0; --k) {
        const int l1 = 1 + 2 * k, l2 = 2 + 2 * k;
        const float *hin = k == 0 ? L->a[0].p : L->a[l2 - 2].p;
        // BN2/conv2 backward: dt = d(out) * (out > 0) is the gradient of the pre-ReLU sum, shared
        // by BN2 and the skip path (k_bn_bwd also writes it to d1); conv2's input is a[l1]; its
        // data gradient overwrites d0 with dL/d(relu1 output)
        bn_conv_bwd(l2, L->d0.p, L->a[l1].p, L->d0.p, false, L->d1.p);
        // BN1/conv1 backward: da = d0 (gradient wrt relu1 output), mask a[l1]; its input is hin;
        // dgrad accumulates into d1 (= dt, the skip gradient) -> d(block input)
        bn_conv_bwd(l1, L->d0.p, hin, L->d1.p, true, nullptr);
        std::swap(L->d0, L->d1);   // d0 = dL/d(block input)
    }
    // stem: no data gradient
    bn_conv_bwd(0, L->d0.p, x_in, nullptr, false, nullptr);
    // join: every weight gradient is in G before the reduction and Adam
    for (int k = 0; k < kWgSide && crc == SPAI_OK; ++k)
        if (hipEventRecord(L->ev_wg_done[k], L->wg_stream[k]) != hipSuccess ||
            hipStreamWaitEvent(st, L->ev_wg_done[k], 0) != hipSuccess) {
            set_error("learner: event record/wait failed");
            crc = SPAI_ERR_DEVICE;
        }
    SPAI_TRY(crc);
    // ---------------- cross-rank reduction + Adam
    // The global step's gradient is the mean over every rank's samples: each rank
    // weights its own mean gradient by B / sum(B) (one 4-byte all-reduce first),
    // then the gradients are summed.  Exact for unequal per-rank batches; a 1-rank
    // communicator multiplies by 1 and reduces to a copy (bit-identical step).
    const float gscale = 1.0f;
    const bool dp = L->comm || L->host_ar;
    if (dp) {
        k_set1<<<1, 1, 0, st>>>(L->bsum.p, (float)B);
        SPAI_TRY(learner_allreduce(L, L->bsum.p, 1, st, "the batch sizes"));
        k_weight_grad<<<blocks_of(L->n_params), kThreads, 0, st>>>(G, L->n_params, (float)B, L->bsum.p);
        SPAI_TRY(learner_allreduce(L, G, L->n_params, st, "the gradients"));
    }
    k_adam<<<blocks_of(L->n_params), kThreads, 0, st>>>(P, G, L->m.p, L->v.p, L->n_params, gscale, L->cfg.lr,
                                                        L->cfg.beta1, L->cfg.beta2, L->cfg.eps, bc);
    if (dp) {   // average the BN running statistics so replicas stay identical
        const uint32_t nr = (uint32_t)L->run_idx.n;
        k_gather<<<blocks_of(nr), kThreads, 0, st>>>(P, L->run_idx.p, nr, L->run_buf.p);
        SPAI_TRY(learner_allreduce(L, L->run_buf.p, nr, st, "the BN running statistics"));
        k_scatter_scaled<<<blocks_of(nr), kThreads, 0, st>>>(L->run_buf.p, L->run_idx.p, nr, 1.0f / (float)L->world, P);
    }
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

// one step's batch and Adam bias corrections into the pinned staging half `stage`,
// one DMA of it, the step; launch-only
static int stage_and_enqueue(spai_learner *L, uint32_t B, const float *states, const float *policies,
                             const float *values, float *stage) {
    hipStream_t st = L->eng->stream;
    const size_t nin = (size_t)B * (3 * kCells + 8);
    L->step += 1;
    const double t = (double)L->step;
    stage[nin] = (float)(1.0 - std::pow((double)L->cfg.beta1, t));
    stage[nin + 1] = (float)std::sqrt(1.0 - std::pow((double)L->cfg.beta2, t));
    std::memcpy(stage, states, (size_t)B * 3 * kCells * 4);
    std::memcpy(stage + (size_t)B * 3 * kCells, policies, (size_t)B * 7 * 4);
    std::memcpy(stage + (size_t)B * (3 * kCells + 7), values, (size_t)B * 4);
    SPAI_HIP(hipMemcpyAsync(L->batch_in.p, stage, (nin + 2) * 4, hipMemcpyHostToDevice, st));
    const float *x_in = L->batch_in.p, *pi_in = x_in + (size_t)B * 3 * kCells, *z_in = pi_in + (size_t)B * 7;
    const float *bc = L->batch_in.p + nin;
    // (Replaying the step as a captured hipGraph was measured slower twice: the replay
    // runs every kernel on one queue, so the weight gradients lose their overlap with the
    // data-gradient chain; profiles/r05/learner/graph, profiles/r02/learner/graph_ab.txt)
    SPAI_TRY(enqueue_step(L, B, st, x_in, pi_in, z_in, bc));
    L->last_batch = B;
    return SPAI_OK;
}

int learner_train_batch(spai_learner *L, uint32_t B, const float *states, const float *policies, const float *values,
                        float *loss3) {
    SPAI_CHECK(B >= 1, SPAI_ERR_INVALID, "train_batch: empty batch");
    SPAI_TRY(learner_alloc_batch(L, B));
    hipStream_t st = L->eng->stream;
    SPAI_TRY(stage_and_enqueue(L, B, states, policies, values, L->stage));
    const size_t nin = (size_t)B * (3 * kCells + 8);
    float *terms = L->stage + nin + 2;   // the staged inputs were consumed by the DMA above (stream order)
    SPAI_HIP(hipMemcpyAsync(terms, L->loss_terms.p, (size_t)B * 2 * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    (void)lc::sum_loss(terms, B, loss3);
    return SPAI_OK;
}

// k consecutive train steps of B samples each (batch j = rows [j B, (j + 1) B) of
// the arrays), exactly k learner_train_batch calls, with one host synchronisation
// at the end instead of one per step: step j + 1's batch is staged into the other
// pinned half while step j runs (the half is refilled once its previous upload is
// done), and every step's loss terms come back by a stream-ordered copy.
// losses[3 j ..] = step j's {total, policy, value}.
int learner_train_batches(spai_learner *L, uint32_t k, uint32_t B, const float *states, const float *policies,
                          const float *values, float *losses) {
    SPAI_CHECK(B >= 1 && k >= 1, SPAI_ERR_INVALID, "train_batches: need k >= 1 batches of B >= 1 samples");
    SPAI_TRY(learner_alloc_batch(L, B));
    hipStream_t st = L->eng->stream;
    const size_t need = (size_t)k * B * 2;
    if (L->terms_host_n < need) {
        if (L->terms_host) (void)hipHostFree(L->terms_host);
        L->terms_host = nullptr;
        L->terms_host_n = 0;
        SPAI_HIP(hipHostMalloc((void **)&L->terms_host, need * sizeof(float), hipHostMallocDefault));
        L->terms_host_n = need;
    }
    for (uint32_t j = 0; j < k; ++j) {
        float *half = (j & 1) ? L->stage_b : L->stage;
        if (j >= 2) SPAI_HIP(hipEventSynchronize(L->stage_ev[j & 1]));   // its previous upload is done
        SPAI_TRY(stage_and_enqueue(L, B, states + (size_t)j * B * 3 * kCells, policies + (size_t)j * B * 7,
                                   values + (size_t)j * B, half));
        SPAI_HIP(hipEventRecord(L->stage_ev[j & 1], st));   // after the upload (and the step) in stream order
        SPAI_HIP(hipMemcpyAsync(L->terms_host + (size_t)j * B * 2, L->loss_terms.p, (size_t)B * 2 * 4,
                                hipMemcpyDeviceToHost, st));
    }
    SPAI_HIP(hipStreamSynchronize(st));
    if (losses)
        for (uint32_t j = 0; j < k; ++j) (void)lc::sum_loss(L->terms_host + (size_t)j * B * 2, B, losses + 3 * j);
    return SPAI_OK;
}

// Model::train: lc::train_epochs (learner_common.h) over learner_train_batch
int learner_train_epochs(spai_learner *L, uint32_t n, const float *states, const float *policies,
                         const float *values, uint32_t epochs, uint32_t batch, uint64_t seed, float *loss3) {
    return lc::train_epochs(*L, L->eng->stream, 3 * kCells, 7, n, states, policies, values, epochs, batch, seed,
                            [&](uint32_t m, const float *s, const float *p, const float *v) {
                                return learner_train_batch(L, m, s, p, v, loss3);
                            });
}

int learner_params(spai_learner *L, float *params, size_t n, bool grads) {
    SPAI_CHECK(n == L->n_params, SPAI_ERR_INVALID, "expected %zu params, got %zu", L->n_params, n);
    hipStream_t st = L->eng->stream;
    SPAI_HIP(hipMemcpyAsync(params, grads ? L->g.p : L->p.p, n * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    return SPAI_OK;
}

// the latest step's post-ReLU activations of conv layer `layer` (construction
// order: stem, 2*blocks residual convs, policy head, value head), [B][co][6][7]
int learner_activation(spai_learner *L, int layer, float *out, size_t n) {
    SPAI_CHECK(layer >= 0 && (size_t)layer < L->convs.size(), SPAI_ERR_INVALID, "layer %d of %zu", layer,
               L->convs.size());
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    const size_t want = (size_t)L->last_batch * L->convs[layer].co * kCells;
    SPAI_CHECK(n == want, SPAI_ERR_INVALID, "expected %zu activations, got %zu", want, n);
    hipStream_t st = L->eng->stream;
    SPAI_HIP(hipMemcpyAsync(out, L->a[layer].p, n * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    return SPAI_OK;
}

int learner_set_comm(spai_learner *L, int rank, int world, const uint8_t *id) {
    SPAI_CHECK(world >= 1 && rank >= 0 && rank < world, SPAI_ERR_INVALID, "bad rank %d / world %d", rank, world);
    if (L->comm) {
        (void)ncclCommDestroy((ncclComm_t)L->comm);
        L->comm = nullptr;
    }
    L->host_ar = nullptr;   // an RCCL communicator (or none) replaces a host collective
    L->host_ar_user = nullptr;
    L->rank = rank;
    L->world = world;
    if (!id) return SPAI_OK;   // world == 1 without an id: no communicator
    ncclUniqueId uid;
    static_assert(sizeof(uid.internal) == SPAI_COMM_ID_BYTES, "RCCL unique id size");
    memcpy(uid.internal, id, SPAI_COMM_ID_BYTES);
    SPAI_HIP(hipSetDevice(L->eng->device));
    ncclComm_t c = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c, world, uid, rank);
    SPAI_CHECK(r == ncclSuccess, SPAI_ERR_DEVICE, "ncclCommInitRank failed: %s", ncclGetErrorString(r));
    L->comm = c;
    return SPAI_OK;
}

// weight refresh of data-parallel replicas: every rank's parameters (BN running
// statistics included) become rank `root`'s, by one RCCL broadcast over xGMI
int learner_broadcast(spai_learner *L, int root) {
    SPAI_CHECK(root >= 0 && root < L->world, SPAI_ERR_INVALID, "broadcast root %d outside world %d", root, L->world);
    hipStream_t st = L->eng->stream;
    if (L->host_ar) {   // rank root's values plus -0.0 from every other rank: x + -0.0 == x exactly
        SPAI_HIP(hipStreamSynchronize(st));
        if (L->rank == root) {
            SPAI_HIP(hipMemcpy(L->host_buf, L->p.p, L->n_params * 4, hipMemcpyDeviceToHost));
        } else {
            for (size_t i = 0; i < L->n_params; ++i) L->host_buf[i] = -0.0f;
        }
        const int r = L->host_ar(L->host_ar_user, L->host_buf, L->n_params);
        SPAI_CHECK(r == 0, SPAI_ERR_DEVICE, "host all-reduce of the parameters failed (%d)", r);
        SPAI_HIP(hipMemcpy(L->p.p, L->host_buf, L->n_params * 4, hipMemcpyHostToDevice));
        return SPAI_OK;
    }
    if (!L->comm) return SPAI_OK;   // no communicator: a single replica
    if (ncclBroadcast(L->p.p, L->p.p, L->n_params, ncclFloat32, root, (ncclComm_t)L->comm, st) != ncclSuccess) {
        set_error("ncclBroadcast of the parameters failed");
        return SPAI_ERR_DEVICE;
    }
    SPAI_HIP(hipStreamSynchronize(st));
    return SPAI_OK;
}

// host collective in place of RCCL (the same step, each all-reduce staged through pinned memory)
int learner_set_host_comm(spai_learner *L, int rank, int world, spai_host_allreduce fn, void *user) {
    SPAI_CHECK(world >= 1 && rank >= 0 && rank < world, SPAI_ERR_INVALID, "bad rank %d / world %d", rank, world);
    if (L->comm) {
        (void)ncclCommDestroy((ncclComm_t)L->comm);
        L->comm = nullptr;
    }
    // NULL or world 1 drops the collective (spai.h): a 1-rank reduction is the
    // identity, and staging it through host memory would cost the step its
    // launch-only property (three syncs and callbacks per step)
    const bool on = fn && world > 1;
    L->rank = on ? rank : 0;
    L->world = on ? world : 1;
    L->host_ar = on ? fn : nullptr;
    L->host_ar_user = on ? user : nullptr;
    if (!on) return SPAI_OK;
    const size_t need = std::max(L->n_params, L->run_idx.n);
    if (L->host_buf_n < need) {
        if (L->host_buf) (void)hipHostFree(L->host_buf);
        L->host_buf = nullptr;
        L->host_buf_n = 0;
        if (hipHostMalloc((void **)&L->host_buf, need * sizeof(float), hipHostMallocDefault) != hipSuccess) {
            L->host_buf = nullptr;
            L->host_ar = nullptr;
            L->world = 1;
            set_error("learner: pinned host-collective buffer allocation failed");
            return SPAI_ERR_DEVICE;
        }
        L->host_buf_n = need;
    }
    return SPAI_OK;
}

int comm_unique_id(uint8_t *id) {
    ncclUniqueId uid;
    const ncclResult_t r = ncclGetUniqueId(&uid);
    SPAI_CHECK(r == ncclSuccess, SPAI_ERR_DEVICE, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    memcpy(id, uid.internal, SPAI_COMM_ID_BYTES);
    return SPAI_OK;
}

}  // namespace spai
