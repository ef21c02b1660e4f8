// chess_learner.hip — the train step of the chess net on the device
// (model/chess.rs:48-70 under model/mod.rs:128-141), in fp32 or with the conv
// GEMMs' operands in bf16 (spai_chess_learner_set_compute), behind
// spai_chess_learner_* in include/spai.h; and the entry points of the in-place
// weight refresh of a self-play net that Learner::learn needs,
// spai_chess_net_set_params and spai_chess_net_set_params_from_learner (the
// learner's state is private to this file; the kernels are chess_net_pack.hip's).
//
// Train-mode forward (BatchNorm batch statistics in the trunk; the heads have no
// BN), loss = -(log_softmax(p) . pi).sum()/B + mean((v - z)^2), backward, one
// Adam step.  Activations and gradients are NCHW, [B][C][64].
//
// Unlike the Connect4 and TicTacToe steps this one is GEMM-bound: a 3x3 conv at
// 256 channels is 9.66 GFLOP per GEMM at B = 128.  All three GEMMs of a conv run
// on v_mfma_f32_32x32x2_f32 (a k-ordered f32 fmaf chain: one accumulator per
// wave reaches the issue rate) with both operands staged in LDS:
//
//  * k_cl_conv<MODE, TAPS, KC>, forward and data gradient.  A workgroup (4 waves)
//    owns one sample (64 cells = two 32-row tiles, so no tile straddles samples)
//    times 64 output channels; wave = (row half, 32 channels).  Per chunk of KC
//    input channels it stages the sample's KC planes once, with a zero halo
//    (10 x 10), so the nine taps reuse them, and the [tap][channel][64] weight
//    tile, which both row tiles reuse.  The next chunk's global loads are issued
//    into registers before the current chunk's MFMAs.  D = W (A operand, rows =
//    output channels) x plane (B operand, columns = cells), so a store is 32
//    consecutive cells.  The data gradient is the same kernel with the taps
//    flipped and the weights read transposed.  TAPS = 1 serves the 1x1 policy
//    convs; the 19-channel stem is the 3x3 kernel with a masked second chunk.
//  * k_cl_wgrad<TAPS>, weight gradient.  The 64 B rows are cut into chunks of
//    kWgSamples samples; a workgroup owns (chunk, 64 output x 64 input channels)
//    and all taps: 12 waves = 3 tap rows x 2 x 2 tiles of 32 x 32, three
//    accumulators (the row's taps) per wave.  Per sample it stages dz [64][64] and
//    the input planes with halo.  Each chunk's partial dW goes to scratch and
//    k_cl_wreduce sums the chunks in order.
//
// Padding, channels past the layer's count (19, 73) and taps off the board are
// exact zeros in LDS; stores are masked; a workgroup never sees a partial sample.
//
// Summation: a K = 2304 sum as one fmaf chain is ~5x noisier than PyTorch's blocked
// CPU sums, and Adam turns a near-zero gradient's sign into a step of lr.  So an
// MFMA chain runs over one channel chunk (144 products) or one sample (64 rows)
// in an accumulator of its own and the partial sums are added in order.
//
// Determinism: no floating-point atomics.  Every MFMA chain has a fixed order
// (chunk, tap, channel pair / sample, cell pair); weight-gradient chunks are summed
// in chunk order; BN statistics, gamma/beta/bias gradients: one workgroup per
// channel, per-thread partials in a fixed element order and a fixed LDS tree;
// linear gradients: one thread per entry, samples in order; loss: per-sample
// terms, summed on the host in order.
//
// bf16 compute (opt-in; DESIGN.md section 2.2 is the contract, 9.1.1 the design):
// every operand of every conv GEMM is rounded to bf16 (nearest even), the products are summed in
// fp32 on v_mfma_f32_32x32x16_bf16 and stored as fp32; everything else, and every
// tensor in HBM, stays fp32.  A lane's fragment is 8 consecutive K, so the LDS
// images are not the f32 kernels':
//
//  * k_cl_pack writes, at the start of each step, a bf16 shadow of every conv's
//    weights laid out as the A fragments themselves ([32-channel tile][tap][16-K
//    step][lane][8]), once as the forward reads them and once transposed with the
//    taps flipped for the data gradient, zero past the layer's channels.  A wave
//    loads its fragment straight from that shadow (16 B a lane, 1 KiB a wave,
//    consecutive), one tap ahead of the MFMAs; the weights never enter LDS.
//  * k_cl_conv_bf16<TAPS>, forward and data gradient (they differ only in the shadow
//    they are given).  A workgroup (2 waves) owns one sample times 64 output
//    channels; a wave owns 32 channels times all 64 cells (two accumulators), so a
//    weight fragment serves two MFMAs.  Per chunk of 64 source channels the sample's
//    fp32 planes are read, rounded and stored channel-innermost, [10 x 10 position]
//    [64 channels + 8], so a B fragment (8 channels at one tap-shifted cell) is one
//    aligned 16-byte read.
//  * k_cl_wgrad_bf16<TAPS>, weight gradient: (chunk of kWgSamples samples, 64 x 64
//    channels), 4 waves of 32 x 32, one accumulator per tap.  K runs over cells, a
//    fragment is one board row.  dz is stored [channel][64 cells]; the input is
//    stored three times, shifted by dx = -1, 0, +1 with the zero the shift brings in
//    (the thread that loaded the row has all three in registers), under zero halo
//    rows, so every tap's fragment is again one aligned 16-byte read.  The partials
//    go through the same k_cl_wreduce.
//
// In bf16 an MFMA chain runs over the whole K in one fp32 accumulator (the operand
// rounding, 2^-9 relative, is far above the chain's own noise); the order is fixed.
//
// A step may also take its batch as compact self-play samples (spai_chess_sample):
// the records are uploaded instead of the dense arrays and chess_samples.hip's
// k_samples_expand writes batch_in from them, bit for bit the dense upload.
//
// This file holds what is chess's: the conv, weight-gradient and head kernels, the
// step's launch chain and the entry points.  The BatchNorm and Adam kernels
// (k_lc_bn_fwd<64>, k_lc_bn_bwd<64>, k_lc_adam), the workgroup reductions, the
// learner's state, the staged train step and Model::train's epoch loop are
// learner_common.h's, shared with ttt_learner.hip.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "chess_engine.h"
#include "learner_common.h"

namespace spai {
namespace chess {
namespace {

using lc::block_max;
using lc::block_sum;
using lc::Conv;
using lc::kBnThreads;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kCells = 64, kHid = 256, kPolC = 73, kMaxBlocks = 40;
constexpr int kEnc = kPlanes * kCells;   // 1216
constexpr int kWgSamples = 8;            // samples per weight-gradient chunk
constexpr int kConvKC3 = 16, kConvKC1 = 64;   // input channels per chunk: 3x3, 1x1

// conv (TAPS = 9: 3x3 pad 1; 1: 1x1) as an implicit GEMM for sample blockIdx.x and output
// channels 64 blockIdx.y ..+63: out[s][n][cell] = sum_{c,t} src[s][c][cell + d(t)] Wm[c][t][n]
// MODE 0, forward:       Wm[c][t][n] = w[n][c][t]           out = z + bias (relu: max(., 0))
// MODE 1, data gradient: Wm[c][t][n] = w[c][n][TAPS-1-t]    out = da (+ addend)
// out may alias addend (each element is read and written by the same lane).
template <int MODE, int TAPS, int KC>
__global__ __launch_bounds__(256, 2) void k_cl_conv(const float *__restrict__ src, int csrc,
                                                    const float *__restrict__ w, const float *__restrict__ bias,
                                                    int relu, const float *addend, float *out, int N) {
    // the weight tile is copied as it lies in memory: MODE 0 rows = the 64 output channels,
    // KC * TAPS contiguous floats each; MODE 1 rows = the KC source channels, 64 * TAPS each.
    // TPR threads share a row, so a thread's global and LDS addresses are one base plus
    // constants; the odd row pitch keeps the 32 lanes of an operand read on 32 banks.
    constexpr int PL = TAPS == 9 ? 100 : 64;
    constexpr int ROWS = MODE == 0 ? 64 : KC, RL = (MODE == 0 ? KC : 64) * TAPS, RP = RL + 1;
    constexpr int TPR = 256 / ROWS, NWR = RL / TPR, NPR = KC * 64 / 256;
    __shared__ float planes[KC * PL];
    __shared__ float wl[ROWS * RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, n0 = blockIdx.y * 64;
    const int li = lane & 31, hk = lane >> 5, rh = wave & 1, ch = wave >> 1;
    const int wrow = tid / TPR, wq = tid - wrow * TPR;
    float wr[NWR], pr[NPR];
    auto load = [&](int k0) {
        // MODE 0: row = channel n0 + wrow, element e = (c - k0) * TAPS + t; MODE 1: row = channel k0 + wrow, e = (n - n0) * TAPS + t
        const float *g = MODE == 0 ? w + ((size_t)(n0 + wrow) * csrc + k0) * TAPS
                                   : w + ((size_t)(k0 + wrow) * N + n0) * TAPS;
        const bool rowok = MODE == 0 ? n0 + wrow < N : k0 + wrow < csrc;
        const int lim = rowok ? (MODE == 0 ? min(KC, csrc - k0) : min(64, N - n0)) * TAPS : 0;
#pragma unroll
        for (int j = 0; j < NWR; ++j) wr[j] = wq + TPR * j < lim ? g[wq + TPR * j] : 0.0f;
#pragma unroll
        for (int j = 0; j < NPR; ++j) {
            const int kc = (tid >> 6) + 4 * j;
            pr[j] = k0 + kc < csrc ? src[((size_t)s * csrc + k0 + kc) * kCells + (tid & 63)] : 0.0f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NWR; ++j) wl[wrow * RP + wq + TPR * j] = wr[j];
        const int pc = tid & 63;
#pragma unroll
        for (int j = 0; j < NPR; ++j)
            planes[((tid >> 6) + 4 * j) * PL + (TAPS == 9 ? ((pc >> 3) + 1) * 10 + (pc & 7) + 1 : pc)] = pr[j];
    };
    if (TAPS == 9) {   // the halo: zero once, only the interior is ever stored
        for (int i = tid; i < KC * PL; i += 256) planes[i] = 0.0f;
        __syncthreads();
    }
    const int cell = rh * 32 + li, y = cell >> 3, x = cell & 7;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    load(0);
    for (int k0 = 0; k0 < csrc; k0 += KC) {
        store();
        __syncthreads();
        if (k0 + KC < csrc) load(k0 + KC);   // in flight under this chunk's MFMAs
        // a chunk sums in an accumulator of its own (a chain of KC * TAPS products) and the
        // chunks are added in order: the rounding error of one 2304-long chain is ~5x larger
        f32x16 part;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[r] = 0.0f;
#pragma unroll 1   // a tap row per trip: unrolled further, the hoisted LDS reads spill
        for (int ty = 0; ty < (TAPS == 9 ? 3 : 1); ++ty) {
#pragma unroll
            for (int tx = 0; tx < (TAPS == 9 ? 3 : 1); ++tx) {
                const int t = 3 * ty + tx;
                const int po = TAPS == 9 ? (y + ty) * 10 + x + tx : cell;   // (y + dy + 1, x + dx + 1)
#pragma unroll
                for (int k2 = 0; k2 < KC / 2; ++k2) {
                    const int kc = 2 * k2 + hk;
                    const float a = MODE == 0 ? wl[(ch * 32 + li) * RP + kc * TAPS + t]   // A[m = channel][k]
                                              : wl[kc * RP + (ch * 32 + li) * TAPS + TAPS - 1 - t];
                    const float b = planes[kc * PL + po];                    // B[k][n = cell]
                    part = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, part, 0, 0, 0);
                }
            }
        }
        acc += part;
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {   // D: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int n = n0 + ch * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
        if (n < N) {
            const size_t idx = ((size_t)s * N + n) * kCells + cell;
            float v = acc[r];
            if (bias) v += bias[n];
            if (addend) v += addend[idx];
            if (relu) v = fmaxf(v, 0.0f);
            out[idx] = v;
        }
    }
}

// partial weight gradient of the samples of chunk blockIdx.y for output channels
// 64 cot ..+63 and input channels 64 cit ..+63, (cot, cit) = blockIdx.x:
// part[chunk][t][co][ci] = sum_{s, cell} dz[s][co][cell] in[s][ci][cell + d(t)]
template <int TAPS>
__global__ __launch_bounds__(TAPS == 9 ? 768 : 256) void k_cl_wgrad(const float *__restrict__ dz, int CO,
                                                                    const float *__restrict__ in, int CI,
                                                                    float *__restrict__ part, int B) {
    constexpr int NT = TAPS == 9 ? 768 : 256, PLW = TAPS == 9 ? 101 : 65, TW = TAPS == 9 ? 3 : 1;
    constexpr int NR = (64 * kCells + NT - 1) / NT;
    __shared__ float dzs[64 * 65];
    __shared__ float ins[64 * PLW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nci = (CI + 63) / 64;
    const int cot = blockIdx.x / nci, cit = blockIdx.x - cot * nci, chunk = blockIdx.y;
    const int co0 = cot * 64, ci0 = cit * 64;
    const int s0 = chunk * kWgSamples, s1 = min(B, s0 + kWgSamples);
    const int li = lane & 31, hk = lane >> 5;
    const int g = wave >> 2, cm = wave & 1, cn = (wave >> 1) & 1;   // tap row; 32 x 32 tile of the 64 x 64
    float ra[NR], rb[NR];
    auto load = [&](int s) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int i = tid + NT * j, c = i >> 6, cell = i & 63;
            ra[j] = (i < 64 * kCells && co0 + c < CO) ? dz[((size_t)s * CO + co0 + c) * kCells + cell] : 0.0f;
            rb[j] = (i < 64 * kCells && ci0 + c < CI) ? in[((size_t)s * CI + ci0 + c) * kCells + cell] : 0.0f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int i = tid + NT * j, c = i >> 6, cell = i & 63;
            if (i < 64 * kCells) {
                dzs[c * 65 + cell] = ra[j];
                ins[c * PLW + (TAPS == 9 ? ((cell >> 3) + 1) * 10 + (cell & 7) + 1 : cell)] = rb[j];
            }
        }
    };
    if (TAPS == 9) {
        for (int i = tid; i < 64 * PLW; i += NT) ins[i] = 0.0f;
        __syncthreads();
    }
    f32x16 acc[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    load(s0);
    for (int s = s0; s < s1; ++s) {
        store();
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        f32x16 part[TW];   // a sample's 64 rows sum on their own, the samples are added in order
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[j][r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < kCells / 2; ++ks) {
            const int cell = 2 * ks + hk;
            const float a = dzs[(cm * 32 + li) * 65 + cell];   // A[m = co][k = cell]
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                const int po = TAPS == 9 ? ((cell >> 3) + g) * 10 + (cell & 7) + j : cell;
                const float b = ins[(cn * 32 + li) * PLW + po];   // B[k = cell][n = ci]
                part[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, part[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[j] += part[j];
        __syncthreads();
    }
    const int ci = ci0 + cn * 32 + li;
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int t = g * 3 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (co < CO && ci < CI) part[(((size_t)chunk * TAPS + t) * CO + co) * CI + ci] = acc[j][r];
        }
    }
}

// dw[co][ci][t] = the chunks' partials summed in chunk order
__global__ void k_cl_wreduce(const float *__restrict__ part, int chunks, int CO, int CI, int TAPS,
                             float *__restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= CO * CI * TAPS) return;
    const int co = i / (CI * TAPS), r = i - co * CI * TAPS, ci = r / TAPS, t = r - ci * TAPS;
    float acc = 0.0f;
    for (int c = 0; c < chunks; ++c) acc += part[(((size_t)c * TAPS + t) * CO + co) * CI + ci];
    dw[i] = acc;
}

// ------------------------------------------------------------------ bf16 compute
// two floats rounded to nearest even, packed (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ __forceinline__ uint4 pack_bf16x8(const float *v) {
    return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                      pack_bf16x2(v[6], v[7]));
}
__device__ __forceinline__ f32x16 mfma_bf16(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                   0, 0);
}

constexpr int kBfKC = 64;   // source channels per chunk of k_cl_conv_bf16 = 4 K steps of 16

// the bf16 shadow of layer blockIdx.y's weights w [CO][CI][TAPS] as k_cl_conv_bf16's A
// fragments: out[((mt TAPS + t) KS + ks) 64 + lane], lane = 32 h + r, holds
// Wm[m = 32 mt + r][k = 16 ks + 8 h + j] at tap t in element j;
// mode 0 (forward):       Wm[m][k] = w[m][k][t]
// mode 1 (data gradient): Wm[m][k] = w[k][m][TAPS-1-t]
// and zero past the layer's channels (MT 32-row tiles, KS 16-K steps are padded counts)
__global__ void k_cl_pack(const float *__restrict__ w, size_t wstride, int CO, int CI, int TAPS, int mode,
                          uint4 *__restrict__ out, size_t ostride, int MT, int KS) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MT * TAPS * KS * 64) return;
    w += blockIdx.y * wstride;
    out += blockIdx.y * ostride;
    const int lane = i & 63;
    int q = i >> 6;
    const int ks = q % KS;
    q /= KS;
    const int t = q % TAPS, mt = q / TAPS;
    const int m = 32 * mt + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
    const int M = mode == 0 ? CO : CI, K = mode == 0 ? CI : CO;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        v[j] = (m < M && k < K) ? (mode == 0 ? w[((size_t)m * CI + k) * TAPS + t]
                                             : w[((size_t)k * CI + m) * TAPS + TAPS - 1 - t])
                                : 0.0f;
    }
    out[i] = pack_bf16x8(v);
}

// k_cl_conv's product for sample blockIdx.x and output channels 64 blockIdx.y ..+63 with
// both operands rounded to bf16: out[s][n][cell] = sum_{c,t} bf(src[s][c][cell + d(t)]) Wm[n][c] at t,
// Wm the k_cl_pack shadow of the layer (forward or data gradient), KS its K steps.
// wave = 32 output channels x 64 cells.  out may alias addend.
template <int TAPS>
__global__ __launch_bounds__(128) void k_cl_conv_bf16(const float *__restrict__ src, int csrc,
                                                      const uint4 *__restrict__ wpk, int KS,
                                                      const float *__restrict__ bias, int relu, const float *addend,
                                                      float *out, int N) {
    constexpr int NPOS = TAPS == 9 ? 100 : 64, PQ = kBfKC / 8 + 1;   // a position's row: 8 + 1 (pad) 16-byte groups
    __shared__ uint4 planes[NPOS * PQ];                               // [position][channel of the chunk] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, mt = blockIdx.y * 2 + wave;
    const int li = lane & 31, hk = lane >> 5;
    // staging: cell = lane, channel groups (8 channels) wave + 2 j
    float pr[4][8];
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = k0 + 8 * (wave + 2 * j) + e;
                pr[j][e] = c < csrc ? src[((size_t)s * csrc + c) * kCells + lane] : 0.0f;
            }
    };
    const int spos = TAPS == 9 ? ((lane >> 3) + 1) * 10 + (lane & 7) + 1 : lane;
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) planes[spos * PQ + wave + 2 * j] = pack_bf16x8(pr[j]);
    };
    if (TAPS == 9) {   // the halo: zero once, only the interior is ever stored
        for (int i = tid; i < NPOS * PQ; i += 128) planes[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    const uint4 *wa = wpk + (size_t)mt * TAPS * KS * 64 + lane;
    uint4 an[4];
    auto load_a = [&](int chunk, int t) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) an[kk] = wa[((size_t)t * KS + chunk * 4 + kk) * 64];
    };
    f32x16 acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.0f;
    const int nchunks = KS / 4;
    load(0);
    load_a(0, 0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        store();
        __syncthreads();
        if (chunk + 1 < nchunks) load((chunk + 1) * kBfKC);   // in flight under this chunk's MFMAs
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            uint4 a[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) a[kk] = an[kk];
            if (t + 1 < TAPS) load_a(chunk, t + 1);   // the next tap's weights, one tap ahead
            else if (chunk + 1 < nchunks) load_a(chunk + 1, 0);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const int cell = rt * 32 + li;
                const int po = TAPS == 9 ? ((cell >> 3) + t / 3) * 10 + (cell & 7) + t % 3 : cell;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[rt] = mfma_bf16(a[kk], planes[po * PQ + 2 * kk + hk], acc[rt]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {   // D: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            const int n = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (n < N) {
                const size_t idx = ((size_t)s * N + n) * kCells + rt * 32 + li;
                float v = acc[rt][r];
                if (bias) v += bias[n];
                if (addend) v += addend[idx];
                if (relu) v = fmaxf(v, 0.0f);
                out[idx] = v;
            }
        }
}

// k_cl_wgrad's partial with both operands rounded to bf16 (same grid, same partials):
// part[chunk][t][co][ci] = sum_{s, cell} bf(dz[s][co][cell]) bf(in[s][ci][cell + d(t)])
// 4 waves = 2 x 2 tiles of 32 x 32, an accumulator per tap; K = cells, a fragment = a board row
template <int TAPS>
__global__ __launch_bounds__(256) void k_cl_wgrad_bf16(const float *__restrict__ dz, int CO,
                                                       const float *__restrict__ in, int CI,
                                                       float *__restrict__ part, int B) {
    constexpr int TW = TAPS == 9 ? 3 : 1;        // images of the input, one per x shift
    constexpr int DQ = 9;                        // dz row: 8 board rows + 1 (pad) 16-byte groups
    constexpr int IQ = TAPS == 9 ? 11 : 9;       // input row: (halo +) 8 board rows (+ halo) + 1 (pad)
    __shared__ uint4 dzs[64 * DQ];
    __shared__ uint4 ins[TW * 64 * IQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nci = (CI + 63) / 64;
    const int cot = blockIdx.x / nci, cit = blockIdx.x - cot * nci, chunk = blockIdx.y;
    const int co0 = cot * 64, ci0 = cit * 64;
    const int s0 = chunk * kWgSamples, s1 = min(B, s0 + kWgSamples);
    const int li = lane & 31, hk = lane >> 5, cm = wave & 1, cn = wave >> 1;
    // staging: board row y = tid & 7 of channels (tid >> 3) + 32 j
    const int sy = tid & 7, sc = tid >> 3;
    float4 ra[2][2], rb[2][2];
    auto load = [&](int s) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = sc + 32 * j;
            const float4 *pa = (const float4 *)(dz + ((size_t)s * CO + co0 + c) * kCells + 8 * sy);
            const float4 *pb = (const float4 *)(in + ((size_t)s * CI + ci0 + c) * kCells + 8 * sy);
            const bool oka = co0 + c < CO, okb = ci0 + c < CI;
            ra[j][0] = oka ? pa[0] : zero;
            ra[j][1] = oka ? pa[1] : zero;
            rb[j][0] = okb ? pb[0] : zero;
            rb[j][1] = okb ? pb[1] : zero;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = sc + 32 * j;
            const float a[8] = {ra[j][0].x, ra[j][0].y, ra[j][0].z, ra[j][0].w,
                                ra[j][1].x, ra[j][1].y, ra[j][1].z, ra[j][1].w};
            dzs[c * DQ + sy] = pack_bf16x8(a);
            const float b[10] = {0.0f,       rb[j][0].x, rb[j][0].y, rb[j][0].z, rb[j][0].w,
                                 rb[j][1].x, rb[j][1].y, rb[j][1].z, rb[j][1].w, 0.0f};
            if (TAPS == 9) {   // image tx holds in[y][x + tx - 1] at x, under halo row 0
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) ins[(tx * 64 + c) * IQ + sy + 1] = pack_bf16x8(b + tx);
            } else {
                ins[c * IQ + sy] = pack_bf16x8(b + 1);
            }
        }
    };
    if (TAPS == 9) {   // the halo rows: zero once, only the board rows are ever stored
        for (int i = tid; i < TW * 64 * IQ; i += 256) ins[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    load(s0);
    for (int s = s0; s < s1; ++s) {
        store();
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int y = 2 * ks + hk;                            // cells 8 y .. 8 y + 7
            const uint4 a = dzs[(cm * 32 + li) * DQ + y];         // A[m = co][k = cell]
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int row = TAPS == 9 ? y + t / 3 : y;        // halo row index of board row y + dy
                const uint4 b = ins[((TAPS == 9 ? t % 3 : 0) * 64 + cn * 32 + li) * IQ + row];   // B[k = cell][n = ci]
                acc[t] = mfma_bf16(a, b, acc[t]);
            }
        }
        __syncthreads();
    }
    const int ci = ci0 + cn * 32 + li;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hk;
            if (co < CO && ci < CI) part[(((size_t)chunk * TAPS + t) * CO + co) * CI + ci] = acc[t][r];
        }
}

// a conv with bias and no BN, channel blockIdx.x: d becomes d [a > 0] (a: its ReLU
// output, or NULL for none), g_bias[c] = its sum
__global__ __launch_bounds__(kBnThreads) void k_cl_bias_grad(float *__restrict__ d, const float *__restrict__ a, int C,
                                                             int B, float *__restrict__ g_bias) {
    __shared__ float sh[kBnThreads];
    const int c = blockIdx.x, t = threadIdx.x, nn = kCells * B;
    float acc = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) {
        const size_t idx = ((size_t)(i >> 6) * C + c) * kCells + (i & 63);
        float v = d[idx];
        if (a) {
            v = a[idx] > 0.0f ? v : 0.0f;
            d[idx] = v;
        }
        acc += v;
    }
    acc = block_sum(acc, sh);
    if (t == 0) g_bias[c] = acc;
}

// sample blockIdx.x: the policy loss term -(log_softmax(logits) . pi) and
// dlogits = (softmax sum(pi) - pi) / B over the 4672 logits
__global__ __launch_bounds__(kBnThreads) void k_cl_policy_loss(const float *__restrict__ logits,
                                                               const float *__restrict__ pi, int B,
                                                               float *__restrict__ dlogits,
                                                               float *__restrict__ terms) {
    __shared__ float sh[kBnThreads];
    const int s = blockIdx.x, t = threadIdx.x;
    const float *lg = logits + (size_t)s * kPolicy, *p = pi + (size_t)s * kPolicy;
    float mx = -INFINITY;
    for (int j = t; j < kPolicy; j += kBnThreads) mx = fmaxf(mx, lg[j]);
    mx = block_max(mx, sh);
    float se = 0.0f, spi = 0.0f;
    for (int j = t; j < kPolicy; j += kBnThreads) {
        se += expf(lg[j] - mx);
        spi += p[j];
    }
    se = block_sum(se, sh);
    spi = block_sum(spi, sh);
    const float lse = logf(se) + mx;
    float lp = 0.0f;
    for (int j = t; j < kPolicy; j += kBnThreads) {
        const float ls = lg[j] - lse, pj = p[j];
        lp -= ls * pj;
        dlogits[(size_t)s * kPolicy + j] = (expf(ls) * spi - pj) / (float)B;
    }
    lp = block_sum(lp, sh);
    if (t == 0) terms[2 * s] = lp;
}

// sample blockIdx.x: the value head (conv1x1 256->1 + ReLU, linear 64->256 + ReLU,
// linear 256->1, tanh), its loss term (v - z)^2, dpre = 2 (v - z) / B (1 - v^2), the
// gradients of both hidden activations, and the value head's share of the trunk
// output's gradient (dtower is overwritten)
__global__ __launch_bounds__(kBnThreads) void k_cl_value(const float *__restrict__ tower, const float *__restrict__ vw,
                                                         const float *__restrict__ vb, const float *__restrict__ l1w,
                                                         const float *__restrict__ l1b, const float *__restrict__ l2w,
                                                         const float *__restrict__ l2b, const float *__restrict__ zt,
                                                         int B, float *__restrict__ vc_out, float *__restrict__ h1_out,
                                                         float *__restrict__ dh1_out, float *__restrict__ dvc_out,
                                                         float *__restrict__ dpre, float *__restrict__ terms,
                                                         float *__restrict__ dtower) {
    __shared__ float sh[kBnThreads], vcs[kCells], dvs[kCells], dh1s[kHid];
    const int s = blockIdx.x, t = threadIdx.x;
    const float *h = tower + (size_t)s * kHid * kCells;
    {
        const int cell = t & 63, part = t >> 6;
        float acc = 0.0f;
        for (int c = part * 64; c < part * 64 + 64; ++c) acc = fmaf(vw[c], h[c * kCells + cell], acc);
        sh[t] = acc;
    }
    __syncthreads();
    if (t < kCells) {
        const float v = fmaxf(((sh[t] + sh[64 + t]) + (sh[128 + t] + sh[192 + t])) + vb[0], 0.0f);
        vcs[t] = v;
        vc_out[(size_t)s * kCells + t] = v;
    }
    __syncthreads();
    float h1 = l1b[t];
    for (int c = 0; c < kCells; ++c) h1 = fmaf(l1w[t * kCells + c], vcs[c], h1);
    h1 = fmaxf(h1, 0.0f);
    h1_out[(size_t)s * kHid + t] = h1;
    const float v = tanhf(block_sum(l2w[t] * h1, sh) + l2b[0]);
    const float e = v - zt[s];
    const float dpv = 2.0f * e / (float)B * (1.0f - v * v);
    if (t == 0) {
        terms[2 * s + 1] = e * e;
        dpre[s] = dpv;
    }
    const float dh1 = h1 > 0.0f ? dpv * l2w[t] : 0.0f;
    dh1_out[(size_t)s * kHid + t] = dh1;
    dh1s[t] = dh1;
    __syncthreads();
    if (t < kCells) {
        float acc = 0.0f;
        for (int j = 0; j < kHid; ++j) acc = fmaf(dh1s[j], l1w[j * kCells + t], acc);
        const float dv = vcs[t] > 0.0f ? acc : 0.0f;
        dvs[t] = dv;
        dvc_out[(size_t)s * kCells + t] = dv;
    }
    __syncthreads();
    for (int i = t; i < kHid * kCells; i += kBnThreads)
        dtower[(size_t)s * kHid * kCells + i] = dvs[i & 63] * vw[i >> 6];
}

// value conv gradients: blockIdx.x = c < 256: g_vw[c] = sum dvc[s][cell] tower[s][c][cell];
// blockIdx.x = 256: g_vb = sum dvc
__global__ __launch_bounds__(kBnThreads) void k_cl_vconv_grad(const float *__restrict__ dvc,
                                                              const float *__restrict__ tower, int B,
                                                              float *__restrict__ g_vw, float *__restrict__ g_vb) {
    __shared__ float sh[kBnThreads];
    const int c = blockIdx.x, t = threadIdx.x, nn = kCells * B;
    float acc = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) {
        const float d = dvc[i];
        acc += c < kHid ? d * tower[((size_t)(i >> 6) * kHid + c) * kCells + (i & 63)] : d;
    }
    acc = block_sum(acc, sh);
    if (t == 0) (c < kHid ? g_vw[c] : g_vb[0]) = acc;
}

// gradients of the two value linears, one thread per entry, samples in order
constexpr int kLinGrads = kHid * kCells + kHid + kHid + 1;   // 16897
__global__ void k_cl_lin_grad(const float *__restrict__ dh1, const float *__restrict__ dpre,
                              const float *__restrict__ vc, const float *__restrict__ h1, int B,
                              float *__restrict__ g_l1w, float *__restrict__ g_l1b, float *__restrict__ g_l2w,
                              float *__restrict__ g_l2b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kLinGrads) return;
    float acc = 0.0f;
    if (i < kHid * kCells) {
        const int j = i >> 6, c = i & 63;
        for (int s = 0; s < B; ++s) acc = fmaf(dh1[(size_t)s * kHid + j], vc[(size_t)s * kCells + c], acc);
        g_l1w[i] = acc;
    } else if (i < kHid * kCells + kHid) {
        const int j = i - kHid * kCells;
        for (int s = 0; s < B; ++s) acc += dh1[(size_t)s * kHid + j];
        g_l1b[j] = acc;
    } else if (i < kHid * kCells + 2 * kHid) {
        const int j = i - kHid * kCells - kHid;
        for (int s = 0; s < B; ++s) acc = fmaf(dpre[s], h1[(size_t)s * kHid + j], acc);
        g_l2w[j] = acc;
    } else {
        for (int s = 0; s < B; ++s) acc += dpre[s];
        g_l2b[0] = acc;
    }
}

}  // namespace

struct Learner : lc::Core {   // batch_in: [x: B*1216 | pi: B*4672 | z: B]
    int blocks = 0;
    std::vector<Conv> convs;   // stem, 2*blocks residual
    size_t p1_w = 0, p1_b = 0, p2_w = 0, p2_b = 0, v_w = 0, v_b = 0, l1_w = 0, l1_b = 0, l2_w = 0, l2_b = 0;
    std::vector<DevBuf<float>> z, a;       // per trunk conv: pre-BN output, post-ReLU activation [B][256][64]
    DevBuf<float> stat;                    // per trunk conv: batch mean [256] | inverse std [256]
    DevBuf<float> ap1, logits, dlogits;    // policy head: relu(conv1x1) [B][256][64], logits and their gradient [B][4672]
    DevBuf<float> vc, h1, dh1, dvc;        // value head: [B][64], [B][256] and their gradients
    DevBuf<float> g0, g1, dz;              // backward: two activation-gradient buffers and dz, [B][256][64]
    DevBuf<float> wpart;                   // weight-gradient partials [chunks][9][256][256]
    // bf16 compute: the k_cl_pack shadows of a conv's weights, forward and data gradient
    struct Shadow {
        size_t fwd = 0, bwd = 0;           // offsets into wsh (16-byte groups)
        int mt_f = 0, ks_f = 0, mt_b = 0, ks_b = 0;   // padded 32-row tiles and 16-K steps of each
    };
    int compute = SPAI_DTYPE_F32;
    DevBuf<uint4> wsh;                     // allocated by the first bf16 step
    size_t wsh_groups = 0;
    std::vector<Shadow> sconvs;            // per trunk conv (the stem has no data gradient)
    Shadow sp1, sp2;
    // the checker's window: copies of the gradients a step overwrites
    int capture = 0;
    uint32_t captured_batch = 0;           // the last step's batch if it was captured
    std::vector<DevBuf<float>> cap;        // per trunk conv: dz; then the masked gradient of the first policy conv
    // compact samples (chess_samples.hip): a batch's records and their children [visits | moves]
    uint32_t compact_batch = 0;            // the batch size the two buffers hold
    DevBuf<spai_chess_sample> csamples;
    DevBuf<uint32_t> cchildren;
};

}  // namespace chess
}  // namespace spai

struct spai_chess_learner : spai::chess::Learner {};

using namespace spai;
using namespace spai::chess;

namespace {

int alloc_batch(spai_chess_learner *L, uint32_t B) {
    if (B <= L->max_batch) return SPAI_OK;
    SPAI_TRY(lc::core_grow_batch(*L, B));
    const size_t act = (size_t)B * kHid * kCells;
    for (size_t l = 0; l < L->convs.size(); ++l) {
        SPAI_TRY(L->z[l].alloc(act));
        SPAI_TRY(L->a[l].alloc(act));
    }
    for (auto *d : {&L->ap1, &L->g0, &L->g1, &L->dz}) SPAI_TRY(d->alloc(act));
    SPAI_TRY(L->logits.alloc((size_t)B * kPolicy));
    SPAI_TRY(L->dlogits.alloc((size_t)B * kPolicy));
    SPAI_TRY(L->vc.alloc((size_t)B * kCells));
    SPAI_TRY(L->dvc.alloc((size_t)B * kCells));
    SPAI_TRY(L->h1.alloc((size_t)B * kHid));
    SPAI_TRY(L->dh1.alloc((size_t)B * kHid));
    SPAI_TRY(L->wpart.alloc((size_t)((B + kWgSamples - 1) / kWgSamples) * 9 * kHid * kHid));
    for (auto &d : L->cap) d.release();   // regrown by the next captured step
    L->captured_batch = 0;
    L->max_batch = B;
    return SPAI_OK;
}

// the capture buffers, for batches up to max_batch
int alloc_capture(spai_chess_learner *L) {
    for (auto &d : L->cap)
        if (!d.p) SPAI_TRY(d.alloc((size_t)L->max_batch * kHid * kCells));
    return SPAI_OK;
}

// the device buffers of a compact batch of B samples: every sample may bring kMaxMoves children
constexpr size_t kChildWords = (size_t)kMaxMoves * (4 + 2) / 4;   // uint32 visits + uint16 moves, in 4-byte words
int alloc_compact(spai_chess_learner *L, uint32_t B) {
    if (B <= L->compact_batch) return SPAI_OK;
    SPAI_HIP(hipStreamSynchronize(L->stream));   // nothing in flight reads the old buffers
    L->compact_batch = 0;
    SPAI_TRY(L->csamples.alloc(B));
    SPAI_TRY(L->cchildren.alloc((size_t)B * kChildWords));
    L->compact_batch = B;
    return SPAI_OK;
}

// the bf16 weight shadows
int alloc_shadow(spai_chess_learner *L) {
    if (L->wsh.p) return SPAI_OK;
    return L->wsh.alloc(L->wsh_groups);
}

void pack_launch(const float *w, size_t wstride, int co, int ci, int taps, int mode, uint4 *out, size_t ostride, int mt,
                 int ks, int layers, hipStream_t st) {
    const int n = mt * taps * ks * 64;
    k_cl_pack<<<dim3((n + 255) / 256, layers), 256, 0, st>>>(w, wstride, co, ci, taps, mode, out, ostride, mt, ks);
}

// refresh every shadow from the parameters (the start of a bf16 step)
void pack_weights(spai_chess_learner *L, hipStream_t st) {
    const float *P = L->p.p;
    uint4 *S = L->wsh.p;
    const Learner::Shadow &s0 = L->sconvs[0];
    pack_launch(P + L->convs[0].w, 0, kHid, kPlanes, 9, 0, S + s0.fwd, 0, s0.mt_f, s0.ks_f, 1, st);
    const int nres = (int)L->convs.size() - 1;
    if (nres > 0) {   // the residual convs lie a fixed stride apart, in the parameters and in the shadow
        const Learner::Shadow &s1 = L->sconvs[1];
        const size_t wstride = nres > 1 ? L->convs[2].w - L->convs[1].w : 0;
        const size_t ostride = nres > 1 ? L->sconvs[2].fwd - s1.fwd : 0;
        pack_launch(P + L->convs[1].w, wstride, kHid, kHid, 9, 0, S + s1.fwd, ostride, s1.mt_f, s1.ks_f, nres, st);
        pack_launch(P + L->convs[1].w, wstride, kHid, kHid, 9, 1, S + s1.bwd, ostride, s1.mt_b, s1.ks_b, nres, st);
    }
    pack_launch(P + L->p1_w, 0, kHid, kHid, 1, 0, S + L->sp1.fwd, 0, L->sp1.mt_f, L->sp1.ks_f, 1, st);
    pack_launch(P + L->p1_w, 0, kHid, kHid, 1, 1, S + L->sp1.bwd, 0, L->sp1.mt_b, L->sp1.ks_b, 1, st);
    pack_launch(P + L->p2_w, 0, kPolC, kHid, 1, 0, S + L->sp2.fwd, 0, L->sp2.mt_f, L->sp2.ks_f, 1, st);
    pack_launch(P + L->p2_w, 0, kPolC, kHid, 1, 1, S + L->sp2.bwd, 0, L->sp2.mt_b, L->sp2.ks_b, 1, st);
}

// out = conv(src) of a layer with weights w [co][ci][taps]: forward (mode 0: src has ci
// channels, out co) or data gradient (mode 1: src has co channels, out ci)
// sh: the layer's bf16 shadow when the learner computes in bf16, else NULL
void conv_launch(spai_chess_learner *L, const Learner::Shadow *sh, int mode, int taps, const float *src, int csrc,
                 const float *w, const float *bias, int relu, const float *addend, float *out, int N, int B,
                 hipStream_t st) {
    const dim3 grid(B, (N + 63) / 64);
    if (sh) {
        const uint4 *wpk = L->wsh.p + (mode == 0 ? sh->fwd : sh->bwd);
        const int ks = mode == 0 ? sh->ks_f : sh->ks_b;
        if (taps == 9) k_cl_conv_bf16<9><<<grid, 128, 0, st>>>(src, csrc, wpk, ks, bias, relu, addend, out, N);
        else k_cl_conv_bf16<1><<<grid, 128, 0, st>>>(src, csrc, wpk, ks, bias, relu, addend, out, N);
        return;
    }
    if (taps == 9) {
        if (mode == 0) k_cl_conv<0, 9, kConvKC3><<<grid, 256, 0, st>>>(src, csrc, w, bias, relu, addend, out, N);
        else k_cl_conv<1, 9, kConvKC3><<<grid, 256, 0, st>>>(src, csrc, w, bias, relu, addend, out, N);
    } else {
        if (mode == 0) k_cl_conv<0, 1, kConvKC1><<<grid, 256, 0, st>>>(src, csrc, w, bias, relu, addend, out, N);
        else k_cl_conv<1, 1, kConvKC1><<<grid, 256, 0, st>>>(src, csrc, w, bias, relu, addend, out, N);
    }
}

// dw [co][ci][taps] from dz [B][co][64] and the layer's input [B][ci][64]
void wgrad_launch(spai_chess_learner *L, int taps, const float *dz, int co, const float *in, int ci, float *dw, int B,
                  hipStream_t st) {
    const int chunks = (B + kWgSamples - 1) / kWgSamples;
    const dim3 grid(((co + 63) / 64) * ((ci + 63) / 64), chunks);
    if (L->compute == SPAI_DTYPE_BF16) {
        if (taps == 9) k_cl_wgrad_bf16<9><<<grid, 256, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
        else k_cl_wgrad_bf16<1><<<grid, 256, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
    } else if (taps == 9) k_cl_wgrad<9><<<grid, 768, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
    else k_cl_wgrad<1><<<grid, 256, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
    const int n = co * ci * taps;
    k_cl_wreduce<<<(n + 255) / 256, 256, 0, st>>>(L->wpart.p, chunks, co, ci, taps, dw);
}

const Learner::Shadow *shadow(spai_chess_learner *L, const Learner::Shadow *sh) {
    return L->compute == SPAI_DTYPE_BF16 ? sh : nullptr;
}

void conv_fwd(spai_chess_learner *L, int l, const float *in, const float *res, int B, hipStream_t st) {
    const Conv &c = L->convs[l];
    float *P = L->p.p, *stat = L->stat.p + (size_t)l * 2 * kHid;
    conv_launch(L, shadow(L, &L->sconvs[l]), 0, 9, in, c.ci, P + c.w, P + c.b, 0, nullptr, L->z[l].p, c.co, B,
                st);
    lc::k_lc_bn_fwd<kCells><<<c.co, kBnThreads, 0, st>>>(L->z[l].p, c.co, B, P + c.g, P + c.be, P + c.mu, P + c.var,
                                                         res, L->a[l].p, stat, stat + kHid, L->cfg.bn_momentum,
                                                         L->cfg.bn_eps);
}

// da: gradient of layer l's activation (becomes dy when keep_dy); in: the layer's input
// activation; dx (may be NULL): receives the input's gradient, plus addend
void conv_bwd(spai_chess_learner *L, int l, float *da, int keep_dy, const float *in, float *dx, const float *addend,
              int B, hipStream_t st) {
    const Conv &c = L->convs[l];
    float *P = L->p.p, *G = L->g.p, *stat = L->stat.p + (size_t)l * 2 * kHid;
    lc::k_lc_bn_bwd<kCells><<<c.co, kBnThreads, 0, st>>>(da, L->a[l].p, L->z[l].p, c.co, B, stat, stat + kHid, P + c.g,
                                                         L->dz.p, G + c.g, G + c.be, G + c.b, keep_dy);
    if (L->capture)
        (void)hipMemcpyAsync(L->cap[l].p, L->dz.p, (size_t)B * kHid * kCells * 4, hipMemcpyDeviceToDevice, st);
    wgrad_launch(L, 9, L->dz.p, c.co, in, c.ci, G + c.w, B, st);
    if (dx)
        conv_launch(L, shadow(L, &L->sconvs[l]), 1, 9, L->dz.p, c.co, P + c.w, nullptr, 0, addend, dx, c.ci, B,
                    st);
}

// one train step on the batch already in batch_in
int enqueue_step(spai_chess_learner *L, int B) {
    hipStream_t st = L->stream;
    float *P = L->p.p, *G = L->g.p;
    const float *x = L->batch_in.p, *pi = x + (size_t)B * kEnc, *zt = pi + (size_t)B * kPolicy;
    const int nb = L->blocks;
    const Learner::Shadow *sp1 = shadow(L, &L->sp1), *sp2 = shadow(L, &L->sp2);
    if (L->compute == SPAI_DTYPE_BF16) pack_weights(L, st);
    conv_fwd(L, 0, x, nullptr, B, st);
    for (int k = 0; k < nb; ++k) {
        conv_fwd(L, 1 + 2 * k, L->a[2 * k].p, nullptr, B, st);
        conv_fwd(L, 2 + 2 * k, L->a[1 + 2 * k].p, L->a[2 * k].p, B, st);
    }
    const float *tower = L->a[2 * nb].p;
    // policy head: relu(conv1x1 + bias), conv1x1 + bias = the logits [B][73 * 64]
    conv_launch(L, sp1, 0, 1, tower, kHid, P + L->p1_w, P + L->p1_b, 1, nullptr, L->ap1.p, kHid, B, st);
    conv_launch(L, sp2, 0, 1, L->ap1.p, kHid, P + L->p2_w, P + L->p2_b, 0, nullptr, L->logits.p, kPolC, B, st);
    k_cl_policy_loss<<<B, kBnThreads, 0, st>>>(L->logits.p, pi, B, L->dlogits.p, L->terms.p);
    // value head, forward and backward; cur starts as its share of the trunk output's gradient
    float *cur = L->g0.p, *oth = L->g1.p;
    k_cl_value<<<B, kBnThreads, 0, st>>>(tower, P + L->v_w, P + L->v_b, P + L->l1_w, P + L->l1_b, P + L->l2_w,
                                         P + L->l2_b, zt, B, L->vc.p, L->h1.p, L->dh1.p, L->dvc.p, L->dpre.p,
                                         L->terms.p, cur);
    k_cl_vconv_grad<<<kHid + 1, kBnThreads, 0, st>>>(L->dvc.p, tower, B, G + L->v_w, G + L->v_b);
    k_cl_lin_grad<<<(kLinGrads + 255) / 256, 256, 0, st>>>(L->dh1.p, L->dpre.p, L->vc.p, L->h1.p, B, G + L->l1_w,
                                                           G + L->l1_b, G + L->l2_w, G + L->l2_b);
    // policy head backward; the trunk output's gradient becomes complete in cur
    k_cl_bias_grad<<<kPolC, kBnThreads, 0, st>>>(L->dlogits.p, nullptr, kPolC, B, G + L->p2_b);
    wgrad_launch(L, 1, L->dlogits.p, kPolC, L->ap1.p, kHid, G + L->p2_w, B, st);
    conv_launch(L, sp2, 1, 1, L->dlogits.p, kPolC, P + L->p2_w, nullptr, 0, nullptr, oth, kHid, B, st);
    k_cl_bias_grad<<<kHid, kBnThreads, 0, st>>>(oth, L->ap1.p, kHid, B, G + L->p1_b);
    if (L->capture)
        (void)hipMemcpyAsync(L->cap.back().p, oth, (size_t)B * kHid * kCells * 4, hipMemcpyDeviceToDevice, st);
    wgrad_launch(L, 1, oth, kHid, tower, kHid, G + L->p1_w, B, st);
    conv_launch(L, sp1, 1, 1, oth, kHid, P + L->p1_w, nullptr, 0, cur, cur, kHid, B, st);
    for (int k = nb - 1; k >= 0; --k) {
        conv_bwd(L, 2 + 2 * k, cur, 1, L->a[1 + 2 * k].p, oth, nullptr, B, st);   // cur becomes dy, the skip's share
        conv_bwd(L, 1 + 2 * k, oth, 0, L->a[2 * k].p, cur, cur, B, st);
    }
    conv_bwd(L, 0, cur, 0, x, nullptr, nullptr, B, st);
    lc::adam_step(*L);
    SPAI_HIP(hipGetLastError());
    L->last_batch = (uint32_t)B;
    L->captured_batch = L->capture ? (uint32_t)B : 0;
    return SPAI_OK;
}

int train_batch(spai_chess_learner *L, uint32_t B, const float *states, const float *policies, const float *values,
                float *loss3) {
    SPAI_CHECK(B >= 1 && B <= (1u << 16), SPAI_ERR_INVALID, "train_batch: batch of %u samples", B);
    SPAI_TRY(alloc_batch(L, B));
    if (L->capture) SPAI_TRY(alloc_capture(L));
    if (L->compute == SPAI_DTYPE_BF16) SPAI_TRY(alloc_shadow(L));
    bool finite = true;
    SPAI_TRY(lc::train_batch(*L, B, states, policies, values, loss3, &finite,
                             [&](int b) { return enqueue_step(L, b); }));
    // intended: chess alone makes a non-finite loss an error (spai.h); TicTacToe and Connect4 return it as the loss
    SPAI_CHECK(finite, SPAI_ERR_NAN, "chess learner: non-finite loss at step %llu", (unsigned long long)L->step);
    return SPAI_OK;
}

// one train step on B validated compact samples, sample i of the batch being
// samples[index ? index[i] : i]: the records and the children they own go through the
// pinned staging (which holds a dense batch, so it holds them) in one copy each, with
// `first` rebuilt for the packed children; k_samples_expand writes batch_in; the step
// itself is the dense one's
int train_batch_compact(spai_chess_learner *L, uint32_t B, const spai_chess_sample *samples, const uint32_t *index,
                        const uint16_t *child_moves, const uint32_t *child_visits, float *loss3) {
    SPAI_CHECK(B >= 1 && B <= (1u << 16), SPAI_ERR_INVALID, "train_batch: batch of %u samples", B);
    SPAI_TRY(alloc_batch(L, B));
    SPAI_TRY(alloc_compact(L, B));
    if (L->capture) SPAI_TRY(alloc_capture(L));
    if (L->compute == SPAI_DTYPE_BF16) SPAI_TRY(alloc_shadow(L));
    spai_chess_sample *hs = reinterpret_cast<spai_chess_sample *>(L->stage);
    uint32_t total = 0;
    for (uint32_t i = 0; i < B; ++i) {
        hs[i] = samples[index ? index[i] : i];
        total += hs[i].n_children;
    }
    uint32_t *hv = reinterpret_cast<uint32_t *>(hs + B);
    uint16_t *hm = reinterpret_cast<uint16_t *>(hv + total);
    uint32_t at = 0;
    for (uint32_t i = 0; i < B; ++i) {
        const uint32_t f = hs[i].first, k = hs[i].n_children;
        memcpy(hv + at, child_visits + f, (size_t)k * 4);
        memcpy(hm + at, child_moves + f, (size_t)k * 2);
        hs[i].first = at;
        at += k;
    }
    hipStream_t st = L->stream;
    const uint32_t *dv = L->cchildren.p;
    const uint16_t *dm = reinterpret_cast<const uint16_t *>(dv + total);
    SPAI_HIP(hipMemcpyAsync(L->csamples.p, hs, (size_t)B * sizeof(spai_chess_sample), hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(L->cchildren.p, hv, (size_t)total * 6, hipMemcpyHostToDevice, st));
    SPAI_TRY(samples_expand_device(L->csamples.p, dv, dm, total, B, L->batch_in.p, st));
    bool finite = true;
    SPAI_TRY(lc::run_step(*L, B, loss3, &finite, [&](int b) { return enqueue_step(L, b); }));
    SPAI_CHECK(finite, SPAI_ERR_NAN, "chess learner: non-finite loss at step %llu", (unsigned long long)L->step);
    return SPAI_OK;
}

void learner_free(spai_chess_learner *L) {
    L->csamples.release();
    L->cchildren.release();
    for (auto &d : L->z) d.release();
    for (auto &d : L->a) d.release();
    for (auto &d : L->cap) d.release();
    L->wsh.release();
    for (auto *d : {&L->stat, &L->ap1, &L->logits, &L->dlogits, &L->vc, &L->h1, &L->dh1, &L->dvc, &L->g0, &L->g1,
                    &L->dz, &L->wpart})
        d->release();
    lc::core_free(*L);
    delete L;
}

int learner_init(spai_chess_learner *L, const float *params) {
    lc::Layout lay;
    L->convs.push_back(lay.conv3x3_bn(kPlanes, kHid));
    for (int i = 0; i < 2 * L->blocks; ++i) L->convs.push_back(lay.conv3x3_bn(kHid, kHid));
    L->p1_w = lay.take((size_t)kHid * kHid);
    L->p1_b = lay.take(kHid);
    L->p2_w = lay.take((size_t)kPolC * kHid);
    L->p2_b = lay.take(kPolC);
    L->v_w = lay.take(kHid);
    L->v_b = lay.take(1);
    L->l1_w = lay.take((size_t)kHid * kCells);
    L->l1_b = lay.take(kHid);
    L->l2_w = lay.take(kHid);
    L->l2_b = lay.take(1);
    SPAI_CHECK(lay.off == L->n_params, SPAI_ERR_INVALID, "chess learner layout: %zu != %zu", lay.off, L->n_params);
    const size_t nl = L->convs.size();
    L->z.resize(nl);
    L->a.resize(nl);
    L->cap.resize(nl + 1);
    // the shadows: rows padded to the 64 a workgroup owns, K to whole chunks, zeros beyond the layer
    auto shadow_of = [&](int co, int ci, int taps, bool bwd) {
        auto up = [](int v, int m) { return (v + m - 1) / m * m; };
        Learner::Shadow s;
        s.mt_f = up(co, 64) / 32;
        s.ks_f = up(ci, kBfKC) / 16;
        s.fwd = L->wsh_groups;
        L->wsh_groups += (size_t)s.mt_f * taps * s.ks_f * 64;
        if (bwd) {
            s.mt_b = up(ci, 64) / 32;
            s.ks_b = up(co, kBfKC) / 16;
            s.bwd = L->wsh_groups;
            L->wsh_groups += (size_t)s.mt_b * taps * s.ks_b * 64;
        }
        return s;
    };
    for (size_t l = 0; l < nl; ++l) L->sconvs.push_back(shadow_of(kHid, L->convs[l].ci, 9, l > 0));
    L->sp1 = shadow_of(kHid, kHid, 1, true);
    L->sp2 = shadow_of(kPolC, kHid, 1, true);
    SPAI_TRY(L->stat.alloc(nl * 2 * kHid));
    return lc::core_init(*L, params);
}

}  // namespace

extern "C" {

int spai_chess_learner_create(spai_chess *e, int blocks, const float *params, size_t n_params,
                              const spai_adam_config *cfg, spai_chess_learner **out) {
    SPAI_PTR(e);
    SPAI_PTR(params);
    SPAI_PTR(out);
    *out = nullptr;
    SPAI_CHECK(blocks >= 0 && blocks <= kMaxBlocks, SPAI_ERR_UNSUPPORTED, "chess learner: 0..%d blocks", kMaxBlocks);
    SPAI_CHECK(n_params == net_num_params(blocks), SPAI_ERR_INVALID, "expected %zu params, got %zu",
               net_num_params(blocks), n_params);
    SPAI_SET_DEVICE(e);
    spai_chess_learner *L = new (std::nothrow) spai_chess_learner();
    SPAI_CHECK(L, SPAI_ERR_INVALID, "out of host memory");
    int rc = lc::core_setup(*L, e->device, e->stream, n_params, cfg, kEnc, kPolicy);
    L->blocks = blocks;
    if (rc == SPAI_OK) rc = learner_init(L, params);
    if (rc != SPAI_OK) {
        learner_free(L);
        return rc;
    }
    *out = L;
    return SPAI_OK;
}

int spai_chess_learner_destroy(spai_chess_learner *L) {
    if (!L) return SPAI_OK;
    (void)hipSetDevice(L->device);
    (void)hipStreamSynchronize(L->stream);
    learner_free(L);
    return SPAI_OK;
}

int spai_chess_learner_train_batch(spai_chess_learner *L, uint32_t n, const float *states, const float *policies,
                                   const float *values, float *loss) {
    SPAI_PTR(L);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    SPAI_SET_DEVICE(L);
    return train_batch(L, n, states, policies, values, loss);
}

// Model::train: lc::train_epochs over this learner's train step
int spai_chess_learner_train(spai_chess_learner *L, uint32_t n, const float *states, const float *policies,
                             const float *values, uint32_t epochs, uint32_t batch, uint64_t seed, float *loss) {
    SPAI_PTR(L);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    SPAI_SET_DEVICE(L);
    return lc::train_epochs(*L, L->stream, L->xw, L->pw, n, states, policies, values, epochs, batch, seed,
                            [&](uint32_t m, const float *s, const float *p, const float *v) {
                                return train_batch(L, m, s, p, v, loss);
                            });
}

int spai_chess_learner_train_batch_compact(spai_chess_learner *L, uint32_t n, const spai_chess_sample *samples,
                                           const uint16_t *child_moves, const uint32_t *child_visits,
                                           uint32_t n_children_total, float *loss) {
    SPAI_PTR(L);
    SPAI_PTR(samples);
    SPAI_PTR(child_moves);
    SPAI_PTR(child_visits);
    SPAI_CHECK(n >= 1 && n <= (1u << 16), SPAI_ERR_INVALID, "train_batch: batch of %u samples", n);
    SPAI_TRY(samples_validate(n, samples, child_moves, child_visits, n_children_total));
    SPAI_SET_DEVICE(L);
    return train_batch_compact(L, n, samples, nullptr, child_moves, child_visits, loss);
}

// Model::train over the n * repeat virtual samples: lc::train_epochs' loop with the
// gather replaced by a list of sample indices
int spai_chess_learner_train_compact(spai_chess_learner *L, uint32_t n, const spai_chess_sample *samples,
                                     const uint16_t *child_moves, const uint32_t *child_visits,
                                     uint32_t n_children_total, uint32_t repeat, uint32_t epochs, uint32_t batch,
                                     uint64_t seed, float *loss) {
    SPAI_PTR(L);
    SPAI_PTR(samples);
    SPAI_PTR(child_moves);
    SPAI_PTR(child_visits);
    SPAI_CHECK(n >= 1 && batch >= 1, SPAI_ERR_INVALID, "train: need samples and a batch size");
    SPAI_CHECK(repeat >= 1 && (uint64_t)n * repeat <= 0xFFFFFFFFull, SPAI_ERR_INVALID,
               "train: repeat %u of %u samples (need repeat >= 1 and n * repeat < 2^32)", repeat, n);
    SPAI_TRY(samples_validate(n, samples, child_moves, child_visits, n_children_total));
    SPAI_SET_DEVICE(L);
    const uint32_t nv = n * repeat;
    SPAI_TRY(lc::adam_reset(*L, L->stream));
    std::vector<uint32_t> perm;
    choose_multiple(nv, nv, seed, 0x7EA1Bull, perm);
    batch = std::min(batch, nv);
    std::vector<uint32_t> index(batch);
    const uint32_t nb = (nv + batch - 1) / batch;
    for (uint32_t ep = 0; ep < epochs; ++ep)
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t lo = b * batch, m = std::min(batch, nv - lo);
            for (uint32_t i = 0; i < m; ++i) index[i] = perm[lo + i] % n;
            SPAI_TRY(train_batch_compact(L, m, samples, index.data(), child_moves, child_visits, loss));
        }
    return SPAI_OK;
}

int spai_chess_learner_batch(spai_chess_learner *L, float *states, float *policies, float *values, uint32_t n) {
    SPAI_PTR(L);
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    SPAI_CHECK(n == L->last_batch, SPAI_ERR_INVALID, "the last step's batch has %u samples, not %u", L->last_batch, n);
    SPAI_SET_DEVICE(L);
    const float *x = L->batch_in.p, *pi = x + (size_t)n * kEnc, *z = pi + (size_t)n * kPolicy;
    hipStream_t st = L->stream;
    if (states) SPAI_HIP(hipMemcpyAsync(states, x, (size_t)n * kEnc * 4, hipMemcpyDeviceToHost, st));
    if (policies) SPAI_HIP(hipMemcpyAsync(policies, pi, (size_t)n * kPolicy * 4, hipMemcpyDeviceToHost, st));
    if (values) SPAI_HIP(hipMemcpyAsync(values, z, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    return SPAI_OK;
}

int spai_chess_learner_params(spai_chess_learner *L, float *params, size_t n_params) {
    SPAI_PTR(L);
    SPAI_PTR(params);
    SPAI_SET_DEVICE(L);
    return lc::read_flat(*L, L->p.p, params, n_params);
}

int spai_chess_learner_grads(spai_chess_learner *L, float *grads, size_t n_params) {
    SPAI_PTR(L);
    SPAI_PTR(grads);
    SPAI_SET_DEVICE(L);
    return lc::read_flat(*L, L->g.p, grads, n_params);
}

int spai_chess_learner_activation(spai_chess_learner *L, int layer, float *out, size_t n) {
    SPAI_PTR(L);
    SPAI_PTR(out);
    SPAI_SET_DEVICE(L);
    const int nt = (int)L->convs.size();   // trunk layers 0 .. 2 blocks
    SPAI_CHECK(layer >= 0 && layer < nt + 3, SPAI_ERR_INVALID, "layer %d of %d", layer, nt + 3);
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    const float *src = layer < nt ? L->a[layer].p : layer == nt ? L->ap1.p : layer == nt + 1 ? L->vc.p : L->h1.p;
    const size_t per = layer <= nt ? (size_t)kHid * kCells : layer == nt + 1 ? (size_t)kCells : (size_t)kHid;
    const size_t want = (size_t)L->last_batch * per;
    SPAI_CHECK(n == want, SPAI_ERR_INVALID, "expected %zu activations, got %zu", want, n);
    SPAI_HIP(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, L->stream));
    SPAI_HIP(hipStreamSynchronize(L->stream));
    return SPAI_OK;
}

int spai_chess_learner_set_compute(spai_chess_learner *L, int dtype) {
    SPAI_PTR(L);
    SPAI_CHECK(dtype == SPAI_DTYPE_F32 || dtype == SPAI_DTYPE_BF16, SPAI_ERR_INVALID, "compute type %d", dtype);
    SPAI_SET_DEVICE(L);
    SPAI_HIP(hipStreamSynchronize(L->stream));
    if (dtype == SPAI_DTYPE_BF16) SPAI_TRY(alloc_shadow(L));
    L->compute = dtype;
    return SPAI_OK;
}

int spai_chess_learner_get_compute(spai_chess_learner *L, int *dtype) {
    SPAI_PTR(L);
    SPAI_PTR(dtype);
    *dtype = L->compute;
    return SPAI_OK;
}

int spai_chess_learner_set_capture(spai_chess_learner *L, int on) {
    SPAI_PTR(L);
    SPAI_SET_DEVICE(L);
    SPAI_HIP(hipStreamSynchronize(L->stream));
    L->capture = on != 0;
    if (!L->capture) {
        for (auto &d : L->cap) d.release();
        L->captured_batch = 0;
    }
    return SPAI_OK;
}

int spai_chess_learner_gradient(spai_chess_learner *L, int layer, float *out, size_t n) {
    SPAI_PTR(L);
    SPAI_PTR(out);
    SPAI_SET_DEVICE(L);
    const int nt = (int)L->convs.size();   // trunk layers 0 .. 2 blocks
    SPAI_CHECK(layer >= 0 && layer < nt + 2, SPAI_ERR_INVALID, "layer %d of %d", layer, nt + 2);
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    SPAI_CHECK(L->capture && L->captured_batch == L->last_batch, SPAI_ERR_INVALID,
               "the last train step was not captured");
    const float *src = layer <= nt ? L->cap[layer].p : L->dlogits.p;
    const size_t want = (size_t)L->last_batch * (layer <= nt ? (size_t)kHid * kCells : (size_t)kPolicy);
    SPAI_CHECK(n == want, SPAI_ERR_INVALID, "expected %zu gradients, got %zu", want, n);
    SPAI_HIP(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, L->stream));
    SPAI_HIP(hipStreamSynchronize(L->stream));
    return SPAI_OK;
}

int spai_chess_learner_logits(spai_chess_learner *L, float *out, size_t n) {
    SPAI_PTR(L);
    SPAI_PTR(out);
    SPAI_SET_DEVICE(L);
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    const size_t want = (size_t)L->last_batch * kPolicy;
    SPAI_CHECK(n == want, SPAI_ERR_INVALID, "expected %zu logits, got %zu", want, n);
    SPAI_HIP(hipMemcpyAsync(out, L->logits.p, n * 4, hipMemcpyDeviceToHost, L->stream));
    SPAI_HIP(hipStreamSynchronize(L->stream));
    return SPAI_OK;
}

int spai_chess_learner_last_batch(spai_chess_learner *L, uint32_t *n) {
    SPAI_PTR(L);
    SPAI_PTR(n);
    *n = L->last_batch;
    return SPAI_OK;
}

int spai_chess_net_set_params(spai_chess_net *net, const float *params, size_t n_params) {
    SPAI_PTR(net);
    SPAI_PTR(params);
    SPAI_SET_DEVICE(net->eng);
    return net_set_params(net, params, n_params);
}

int spai_chess_net_set_params_from_learner(spai_chess_net *net, spai_chess_learner *l) {
    SPAI_PTR(net);
    SPAI_PTR(l);
    // a learner steps on its engine's stream, and every engine has a stream of its own
    SPAI_CHECK(l->device == net->eng->device && l->stream == net->eng->stream, SPAI_ERR_INVALID,
               "learner belongs to another engine than the net");
    SPAI_CHECK(l->blocks == net->blocks, SPAI_ERR_INVALID, "learner has %d blocks, the net %d", l->blocks, net->blocks);
    const size_t want = net_num_params(net->blocks);
    SPAI_CHECK(l->n_params == want && l->p.n >= want, SPAI_ERR_INVALID, "learner holds %zu params, the net needs %zu",
               l->n_params, want);
    SPAI_SET_DEVICE(net->eng);
    // the pack reads the learner's latest parameters: both are on the engine's stream
    return net_set_params_device(net, l->p.p, want);
}

}  // extern "C"
