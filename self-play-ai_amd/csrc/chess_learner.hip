// chess_learner.hip — the train step of the chess net on the device
// (model/chess.rs:48-70 under model/mod.rs:128-141), in fp32, behind
// spai_chess_learner_* in include/spai.h; and spai_chess_net_set_params, the
// in-place weight refresh of a self-play net that Learner::learn needs.
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
    L->max_batch = B;
    return SPAI_OK;
}

// out = conv(src) of a layer with weights w [co][ci][taps]: forward (mode 0: src has ci
// channels, out co) or data gradient (mode 1: src has co channels, out ci)
void conv_launch(int mode, int taps, const float *src, int csrc, const float *w, const float *bias, int relu,
                 const float *addend, float *out, int N, int B, hipStream_t st) {
    const dim3 grid(B, (N + 63) / 64);
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
    if (taps == 9) k_cl_wgrad<9><<<grid, 768, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
    else k_cl_wgrad<1><<<grid, 256, 0, st>>>(dz, co, in, ci, L->wpart.p, B);
    const int n = co * ci * taps;
    k_cl_wreduce<<<(n + 255) / 256, 256, 0, st>>>(L->wpart.p, chunks, co, ci, taps, dw);
}

void conv_fwd(spai_chess_learner *L, int l, const float *in, const float *res, int B, hipStream_t st) {
    const Conv &c = L->convs[l];
    float *P = L->p.p, *stat = L->stat.p + (size_t)l * 2 * kHid;
    conv_launch(0, 9, in, c.ci, P + c.w, P + c.b, 0, nullptr, L->z[l].p, c.co, B, st);
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
    wgrad_launch(L, 9, L->dz.p, c.co, in, c.ci, G + c.w, B, st);
    if (dx) conv_launch(1, 9, L->dz.p, c.co, P + c.w, nullptr, 0, addend, dx, c.ci, B, st);
}

// one train step on the batch already in batch_in
int enqueue_step(spai_chess_learner *L, int B) {
    hipStream_t st = L->stream;
    float *P = L->p.p, *G = L->g.p;
    const float *x = L->batch_in.p, *pi = x + (size_t)B * kEnc, *zt = pi + (size_t)B * kPolicy;
    const int nb = L->blocks;
    conv_fwd(L, 0, x, nullptr, B, st);
    for (int k = 0; k < nb; ++k) {
        conv_fwd(L, 1 + 2 * k, L->a[2 * k].p, nullptr, B, st);
        conv_fwd(L, 2 + 2 * k, L->a[1 + 2 * k].p, L->a[2 * k].p, B, st);
    }
    const float *tower = L->a[2 * nb].p;
    // policy head: relu(conv1x1 + bias), conv1x1 + bias = the logits [B][73 * 64]
    conv_launch(0, 1, tower, kHid, P + L->p1_w, P + L->p1_b, 1, nullptr, L->ap1.p, kHid, B, st);
    conv_launch(0, 1, L->ap1.p, kHid, P + L->p2_w, P + L->p2_b, 0, nullptr, L->logits.p, kPolC, B, st);
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
    conv_launch(1, 1, L->dlogits.p, kPolC, P + L->p2_w, nullptr, 0, nullptr, oth, kHid, B, st);
    k_cl_bias_grad<<<kHid, kBnThreads, 0, st>>>(oth, L->ap1.p, kHid, B, G + L->p1_b);
    wgrad_launch(L, 1, oth, kHid, tower, kHid, G + L->p1_w, B, st);
    conv_launch(1, 1, oth, kHid, P + L->p1_w, nullptr, 0, cur, cur, kHid, B, st);
    for (int k = nb - 1; k >= 0; --k) {
        conv_bwd(L, 2 + 2 * k, cur, 1, L->a[1 + 2 * k].p, oth, nullptr, B, st);   // cur becomes dy, the skip's share
        conv_bwd(L, 1 + 2 * k, oth, 0, L->a[2 * k].p, cur, cur, B, st);
    }
    conv_bwd(L, 0, cur, 0, x, nullptr, nullptr, B, st);
    lc::adam_step(*L);
    SPAI_HIP(hipGetLastError());
    L->last_batch = (uint32_t)B;
    return SPAI_OK;
}

int train_batch(spai_chess_learner *L, uint32_t B, const float *states, const float *policies, const float *values,
                float *loss3) {
    SPAI_CHECK(B >= 1 && B <= (1u << 16), SPAI_ERR_INVALID, "train_batch: batch of %u samples", B);
    SPAI_TRY(alloc_batch(L, B));
    bool finite = true;
    SPAI_TRY(lc::train_batch(*L, B, states, policies, values, loss3, &finite,
                             [&](int b) { return enqueue_step(L, b); }));
    // intended: chess alone makes a non-finite loss an error (spai.h); TicTacToe and Connect4 return it as the loss
    SPAI_CHECK(finite, SPAI_ERR_NAN, "chess learner: non-finite loss at step %llu", (unsigned long long)L->step);
    return SPAI_OK;
}

void learner_free(spai_chess_learner *L) {
    for (auto &d : L->z) d.release();
    for (auto &d : L->a) d.release();
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
    SPAI_CHECK(blocks >= 0 && blocks <= kMaxBlocks, SPAI_ERR_UNSUPPORTED, "chess learner: 0..%d blocks", kMaxBlocks);
    SPAI_CHECK(n_params == net_num_params(blocks), SPAI_ERR_INVALID, "expected %zu params, got %zu",
               net_num_params(blocks), n_params);
    SPAI_SET_DEVICE(e);
    spai_chess_learner *L = new (std::nothrow) spai_chess_learner();
    SPAI_CHECK(L, SPAI_ERR_INVALID, "out of host memory");
    lc::core_setup(*L, e->device, e->stream, n_params, cfg, kEnc, kPolicy);
    L->blocks = blocks;
    const int rc = learner_init(L, params);
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

}  // extern "C"
