// ttt_learner.hip — the train step of the TicTacToe net on the device
// (model/tictactoe.rs:50-81 under model/mod.rs:128-141), in fp32, behind
// spai_ttt_learner_* in include/spai.h; and spai_ttt_net_set_params, the
// in-place weight refresh of a self-play net that Learner::learn needs.
//
// The step is the one oracle/learner_ref.py documents for Connect4, on a 3x3
// board with a 9-way policy head: train-mode forward (BatchNorm batch
// statistics), loss = -(log_softmax(p) . pi).sum()/B + mean((v - z)^2),
// backward, one Adam step.
//
// Activations and gradients are NCHW, [B][C][9].  The three convolution GEMMs
// (forward, data gradient, weight gradient) run on v_mfma_f32_16x16x4_f32,
// which is a k-ordered f32 fmaf chain, one wave per 16x16 output tile, the
// operands gathered straight from global memory (everything of a step fits
// L2).  A GEMM row is a (sample, cell) pair, row = 9*sample + cell, so an
// M-tile straddles samples and the last one is partial unless 16 | B; the
// zero padding of the 3x3 conv, rows >= 9B, k >= K and columns >= N are all
// masked to exact zeros at the operand load.
//
// The step is launch-bound, so it stays a chain of small launches on the
// engine's stream: per conv layer forward {conv, BN statistics + apply + ReLU
// (+ residual)} and backward {BN backward + bias gradient, weight gradient,
// data gradient (+ the skip connection's gradient)}; the heads, the loss and
// their backward are one kernel, the linear weight gradients one, Adam one.
//
// Determinism: no floating-point atomics.  BN statistics, gamma/beta/bias
// gradients: one workgroup per channel, per-thread partials in a fixed
// element order and a fixed LDS tree.  Weight gradient: one wave owns a
// 16x16 tile of dW for one tap and sums all 9B rows in order inside its MFMA
// accumulator.  Linear gradients: one thread per entry, samples in order.
// Loss: per-sample terms, summed on the host in order.
//
// This file holds what is TicTacToe's: the conv, weight-gradient and head
// kernels, the step's launch chain and the entry points.  The BatchNorm and Adam
// kernels (k_lc_bn_fwd<9>, k_lc_bn_bwd<9>, k_lc_adam), the learner's state, the
// staged train step and Model::train's epoch loop are learner_common.h's, shared
// with chess_learner.hip.
#include <cmath>
#include <new>
#include <vector>

#include "learner_common.h"
#include "ttt_engine.h"

namespace spai {
namespace ttt {
namespace {

using lc::Conv;
using lc::kBnThreads;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPolC = 32, kValC = 3;
constexpr int kPolK = kPolC * kCells;   // 288
constexpr int kValK = kValC * kCells;   // 27

// 3x3 conv (pad 1) as an implicit GEMM, out[row][n] = sum_kk A[row][kk] Bm[kk][n],
// kk = channel*9 + tap, one wave per (M-tile = blockIdx.x, N-tile = wave).
// MODE 0, forward:       A = src[s][ci][cell + d(tap)],  Bm = w[n][ci][tap],  out = z + bias
// MODE 1, data gradient: A = src[s][co][cell - d(tap)],  Bm = w[co][n][tap],  out = da (+ addend)
// out may alias addend (each element is read and written by the same lane).
template <int MODE>
__global__ __launch_bounds__(256) void k_tl_conv(const float *__restrict__ src, int csrc, const float *__restrict__ w,
                                                 const float *__restrict__ bias, const float *addend, float *out,
                                                 int N, int M) {
    const int lane = threadIdx.x & 63, nt = threadIdx.x >> 6, mt = blockIdx.x;
    const int li = lane & 15, lk = lane >> 4;
    const int row = mt * 16 + li;
    const bool rv = row < M;
    const int s = row / kCells, cell = row - kCells * s, y = cell / 3, x = cell - 3 * y;
    const int n = nt * 16 + li;
    const bool nv = n < N;
    const int K = csrc * 9;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int kk = k0 + lk;
        const bool kv = kk < K;
        const int ch = kk / 9, tap = kk - 9 * ch, ty = tap / 3;
        int dy = ty - 1, dx = tap - 3 * ty - 1;
        if (MODE == 1) {
            dy = -dy;
            dx = -dx;
        }
        const int ny = y + dy, nx = x + dx;
        float a = 0.0f, b = 0.0f;
        if (rv && kv && (unsigned)ny < 3u && (unsigned)nx < 3u) a = src[((size_t)s * csrc + ch) * kCells + ny * 3 + nx];
        if (nv && kv) b = MODE == 0 ? w[(size_t)n * K + kk] : w[((size_t)ch * N + n) * 9 + tap];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // D: column lane & 15, rows 4 (lane >> 4) + r
        const int orow = mt * 16 + 4 * lk + r;
        if (orow < M && nv) {
            const int os = orow / kCells, oc = orow - kCells * os;
            const size_t idx = ((size_t)os * N + n) * kCells + oc;
            float v = acc[r];
            if (MODE == 0) v += bias[n];
            else if (addend) v += addend[idx];
            out[idx] = v;
        }
    }
}

// dW[co][ci][tap] = sum_row dz[row][co] in[row + d(tap)][ci]: one wave per
// (co-tile, ci-tile) = blockIdx.x and tap = blockIdx.y, all 9B rows in order
__global__ __launch_bounds__(64) void k_tl_wgrad(const float *__restrict__ dz, int cout, const float *__restrict__ in,
                                                 int cin, float *__restrict__ dw, int M) {
    const int nit = (cin + 15) / 16;
    const int ct = blockIdx.x / nit, it = blockIdx.x - ct * nit, tap = blockIdx.y;
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int co = ct * 16 + li, ci = it * 16 + li;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r0 = 0; r0 < M; r0 += 4) {
        const int row = r0 + lk;
        const bool rv = row < M;
        const int s = row / kCells, cell = row - kCells * s, y = cell / 3, x = cell - 3 * y;
        const int ny = y + dy, nx = x + dx;
        float a = 0.0f, b = 0.0f;
        if (rv && co < cout) a = dz[((size_t)s * cout + co) * kCells + cell];
        if (rv && ci < cin && (unsigned)ny < 3u && (unsigned)nx < 3u) b = in[((size_t)s * cin + ci) * kCells + ny * 3 + nx];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int oco = ct * 16 + 4 * lk + r;
        if (oco < cout && ci < cin) dw[((size_t)oco * cin + ci) * 9 + tap] = acc[r];
    }
}

// sample blockIdx.x: both linears, tanh, the loss terms {-(log_softmax . pi), (v - z)^2},
// dlogits = (softmax sum(pi) - pi) / B, dpre = 2 (v - z) / B (1 - v^2), and the
// gradients of the two head activations
__global__ __launch_bounds__(64) void k_tl_heads(const float *__restrict__ ap, const float *__restrict__ av,
                                                 const float *__restrict__ pw, const float *__restrict__ pb,
                                                 const float *__restrict__ vw, const float *__restrict__ vb,
                                                 const float *__restrict__ pi, const float *__restrict__ zt, int B,
                                                 float *__restrict__ dlogits, float *__restrict__ dpre,
                                                 float *__restrict__ terms, float *__restrict__ dap,
                                                 float *__restrict__ dav) {
    __shared__ float lg[kCells], dl[kCells], vv, dpv;
    const int s = blockIdx.x, t = threadIdx.x;
    if (t < kCells) {
        float acc = pb[t];
        for (int k = 0; k < kPolK; ++k) acc = fmaf(pw[t * kPolK + k], ap[(size_t)s * kPolK + k], acc);
        lg[t] = acc;
    } else if (t == kCells) {
        float acc = vb[0];
        for (int k = 0; k < kValK; ++k) acc = fmaf(vw[k], av[(size_t)s * kValK + k], acc);
        vv = tanhf(acc);
    }
    __syncthreads();
    if (t == 0) {
        float mx = lg[0];
        for (int j = 1; j < kCells; ++j) mx = fmaxf(mx, lg[j]);
        float se = 0.0f, spi = 0.0f;
        for (int j = 0; j < kCells; ++j) {
            se += expf(lg[j] - mx);
            spi += pi[(size_t)s * kCells + j];
        }
        const float lse = logf(se) + mx;
        float lp = 0.0f;
        for (int j = 0; j < kCells; ++j) {
            const float ls = lg[j] - lse, p = pi[(size_t)s * kCells + j];
            lp -= ls * p;
            const float d = (expf(ls) * spi - p) / (float)B;
            dl[j] = d;
            dlogits[(size_t)s * kCells + j] = d;
        }
        const float v = vv, e = v - zt[s];
        terms[2 * s] = lp;
        terms[2 * s + 1] = e * e;
        dpv = 2.0f * e / (float)B * (1.0f - v * v);
        dpre[s] = dpv;
    }
    __syncthreads();
    for (int k = t; k < kPolK; k += 64) {
        float acc = 0.0f;
        for (int j = 0; j < kCells; ++j) acc = fmaf(dl[j], pw[j * kPolK + k], acc);
        dap[(size_t)s * kPolK + k] = acc;
    }
    if (t < kValK) dav[(size_t)s * kValK + t] = dpv * vw[t];
}

// gradients of the two linears, one thread per entry, samples in order
constexpr int kLinGrads = kCells * kPolK + kCells + kValK + 1;   // 2629
__global__ void k_tl_lin_grad(const float *__restrict__ dlogits, const float *__restrict__ dpre,
                              const float *__restrict__ ap, const float *__restrict__ av, int B,
                              float *__restrict__ g_pw, float *__restrict__ g_pb, float *__restrict__ g_vw,
                              float *__restrict__ g_vb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kLinGrads) return;
    float acc = 0.0f;
    if (i < kCells * kPolK) {
        const int j = i / kPolK, k = i - j * kPolK;
        for (int s = 0; s < B; ++s) acc = fmaf(dlogits[(size_t)s * kCells + j], ap[(size_t)s * kPolK + k], acc);
        g_pw[i] = acc;
    } else if (i < kCells * kPolK + kCells) {
        const int j = i - kCells * kPolK;
        for (int s = 0; s < B; ++s) acc += dlogits[(size_t)s * kCells + j];
        g_pb[j] = acc;
    } else if (i < kCells * kPolK + kCells + kValK) {
        const int k = i - kCells * kPolK - kCells;
        for (int s = 0; s < B; ++s) acc = fmaf(dpre[s], av[(size_t)s * kValK + k], acc);
        g_vw[k] = acc;
    } else {
        for (int s = 0; s < B; ++s) acc += dpre[s];
        g_vb[0] = acc;
    }
}

}  // namespace

struct Learner : lc::Core {   // batch_in: [x: B*27 | pi: B*9 | z: B]
    int blocks = 0;
    std::vector<Conv> convs;   // stem, 2*blocks residual, policy conv, value conv
    size_t pol_w = 0, pol_b = 0, val_w = 0, val_b = 0;
    std::vector<DevBuf<float>> z, a;       // per conv layer: pre-BN output, post-ReLU activation
    DevBuf<float> stat;                    // per conv layer: batch mean [64] | inverse std [64]
    DevBuf<float> g0, g1, dz;              // backward: two activation-gradient buffers and dz, [B][64][9]
    DevBuf<float> dlogits;
};

}  // namespace ttt
}  // namespace spai

struct spai_ttt_learner : spai::ttt::Learner {};

using namespace spai;
using namespace spai::ttt;

namespace {

int alloc_batch(spai_ttt_learner *L, uint32_t B) {
    if (B <= L->max_batch) return SPAI_OK;
    SPAI_TRY(lc::core_grow_batch(*L, B));
    const size_t nl = L->convs.size();
    for (size_t l = 0; l < nl; ++l) {
        SPAI_TRY(L->z[l].alloc((size_t)B * L->convs[l].co * kCells));
        SPAI_TRY(L->a[l].alloc((size_t)B * L->convs[l].co * kCells));
    }
    SPAI_TRY(L->g0.alloc((size_t)B * kHid * kCells));
    SPAI_TRY(L->g1.alloc((size_t)B * kHid * kCells));
    SPAI_TRY(L->dz.alloc((size_t)B * kHid * kCells));
    SPAI_TRY(L->dlogits.alloc((size_t)B * kCells));
    L->max_batch = B;
    return SPAI_OK;
}

void conv_fwd(spai_ttt_learner *L, int l, const float *in, const float *res, int B, hipStream_t st) {
    const Conv &c = L->convs[l];
    const int M = kCells * B, mt = (M + 15) / 16, nt = (c.co + 15) / 16;
    float *P = L->p.p, *stat = L->stat.p + (size_t)l * 2 * kHid;
    k_tl_conv<0><<<mt, 64 * nt, 0, st>>>(in, c.ci, P + c.w, P + c.b, nullptr, L->z[l].p, c.co, M);
    lc::k_lc_bn_fwd<kCells><<<c.co, kBnThreads, 0, st>>>(L->z[l].p, c.co, B, P + c.g, P + c.be, P + c.mu, P + c.var,
                                                         res, L->a[l].p, stat, stat + kHid, L->cfg.bn_momentum,
                                                         L->cfg.bn_eps);
}

// da: gradient of layer l's activation (becomes dy when keep_dy); in: the layer's input
// activation; dx (may be NULL): receives the input's gradient, plus addend
void conv_bwd(spai_ttt_learner *L, int l, float *da, int keep_dy, const float *in, float *dx, const float *addend,
              int B, hipStream_t st) {
    const Conv &c = L->convs[l];
    const int M = kCells * B;
    float *P = L->p.p, *G = L->g.p, *stat = L->stat.p + (size_t)l * 2 * kHid;
    lc::k_lc_bn_bwd<kCells><<<c.co, kBnThreads, 0, st>>>(da, L->a[l].p, L->z[l].p, c.co, B, stat, stat + kHid, P + c.g,
                                                         L->dz.p, G + c.g, G + c.be, G + c.b, keep_dy);
    k_tl_wgrad<<<dim3(((c.co + 15) / 16) * ((c.ci + 15) / 16), 9), 64, 0, st>>>(L->dz.p, c.co, in, c.ci, G + c.w, M);
    if (dx)
        k_tl_conv<1><<<(M + 15) / 16, 64 * ((c.ci + 15) / 16), 0, st>>>(L->dz.p, c.co, P + c.w, nullptr, addend, dx,
                                                                        c.ci, M);
}

// one train step on the batch already in batch_in
int enqueue_step(spai_ttt_learner *L, int B) {
    hipStream_t st = L->stream;
    float *P = L->p.p, *G = L->g.p;
    const float *x = L->batch_in.p, *pi = x + (size_t)B * 27, *zt = pi + (size_t)B * kCells;
    const int nb = L->blocks, lp = 2 * nb + 1, lv = lp + 1;
    conv_fwd(L, 0, x, nullptr, B, st);
    for (int k = 0; k < nb; ++k) {
        conv_fwd(L, 1 + 2 * k, L->a[2 * k].p, nullptr, B, st);
        conv_fwd(L, 2 + 2 * k, L->a[1 + 2 * k].p, L->a[2 * k].p, B, st);
    }
    const float *tower = L->a[2 * nb].p;
    conv_fwd(L, lp, tower, nullptr, B, st);
    conv_fwd(L, lv, tower, nullptr, B, st);
    // the head activations' gradients go to g1: [B][288] then [B][27]
    float *dap = L->g1.p, *dav = dap + (size_t)B * kPolK;
    k_tl_heads<<<B, 64, 0, st>>>(L->a[lp].p, L->a[lv].p, P + L->pol_w, P + L->pol_b, P + L->val_w, P + L->val_b, pi,
                                 zt, B, L->dlogits.p, L->dpre.p, L->terms.p, dap, dav);
    k_tl_lin_grad<<<(kLinGrads + 255) / 256, 256, 0, st>>>(L->dlogits.p, L->dpre.p, L->a[lp].p, L->a[lv].p, B,
                                                           G + L->pol_w, G + L->pol_b, G + L->val_w, G + L->val_b);
    float *cur = L->g0.p, *oth = L->g1.p;   // cur: the gradient of the trunk activation being walked back
    conv_bwd(L, lv, dav, 0, tower, cur, nullptr, B, st);
    conv_bwd(L, lp, dap, 0, tower, cur, cur, B, st);
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

int train_batch(spai_ttt_learner *L, uint32_t B, const float *states, const float *policies, const float *values,
                float *loss3) {
    SPAI_CHECK(B >= 1 && B <= (1u << 20), SPAI_ERR_INVALID, "train_batch: batch of %u samples", B);
    SPAI_TRY(alloc_batch(L, B));
    return lc::train_batch(*L, B, states, policies, values, loss3, nullptr, [&](int b) { return enqueue_step(L, b); });
}

void learner_free(spai_ttt_learner *L) {
    for (auto &d : L->z) d.release();
    for (auto &d : L->a) d.release();
    for (auto *d : {&L->stat, &L->g0, &L->g1, &L->dz, &L->dlogits}) d->release();
    lc::core_free(*L);
    delete L;
}

int learner_init(spai_ttt_learner *L, const float *params) {
    lc::Layout lay;
    L->convs.push_back(lay.conv3x3_bn(3, kHid));
    for (int i = 0; i < 2 * L->blocks; ++i) L->convs.push_back(lay.conv3x3_bn(kHid, kHid));
    L->convs.push_back(lay.conv3x3_bn(kHid, kPolC));
    L->pol_w = lay.take((size_t)kCells * kPolK);
    L->pol_b = lay.take(kCells);
    L->convs.push_back(lay.conv3x3_bn(kHid, kValC));
    L->val_w = lay.take(kValK);
    L->val_b = lay.take(1);
    SPAI_CHECK(lay.off == L->n_params, SPAI_ERR_INVALID, "ttt learner layout: %zu != %zu", lay.off, L->n_params);
    const size_t nl = L->convs.size();
    L->z.resize(nl);
    L->a.resize(nl);
    SPAI_TRY(L->stat.alloc(nl * 2 * kHid));
    return lc::core_init(*L, params);
}

}  // namespace

extern "C" {

int spai_ttt_learner_create(spai_ttt *e, int blocks, const float *params, size_t n_params,
                            const spai_adam_config *cfg, spai_ttt_learner **out) {
    SPAI_PTR(e);
    SPAI_PTR(params);
    SPAI_PTR(out);
    *out = nullptr;
    SPAI_CHECK(blocks >= 0 && blocks <= kMaxBlocks, SPAI_ERR_UNSUPPORTED, "ttt learner: 0..%d blocks", kMaxBlocks);
    SPAI_CHECK(n_params == num_params(blocks), SPAI_ERR_INVALID, "expected %zu params, got %zu", num_params(blocks),
               n_params);
    SPAI_SET_DEVICE(e);
    spai_ttt_learner *L = new (std::nothrow) spai_ttt_learner();
    SPAI_CHECK(L, SPAI_ERR_INVALID, "out of host memory");
    int rc = lc::core_setup(*L, e->device, e->stream, n_params, cfg, 3 * kCells, kCells);
    L->blocks = blocks;
    if (rc == SPAI_OK) rc = learner_init(L, params);
    if (rc != SPAI_OK) {
        learner_free(L);
        return rc;
    }
    *out = L;
    return SPAI_OK;
}

int spai_ttt_learner_destroy(spai_ttt_learner *L) {
    if (!L) return SPAI_OK;
    (void)hipSetDevice(L->device);
    (void)hipStreamSynchronize(L->stream);
    learner_free(L);
    return SPAI_OK;
}

int spai_ttt_learner_train_batch(spai_ttt_learner *L, uint32_t n, const float *states, const float *policies,
                                 const float *values, float *loss) {
    SPAI_PTR(L);
    SPAI_PTR(states);
    SPAI_PTR(policies);
    SPAI_PTR(values);
    SPAI_SET_DEVICE(L);
    return train_batch(L, n, states, policies, values, loss);
}

// Model::train: lc::train_epochs over this learner's train step
int spai_ttt_learner_train(spai_ttt_learner *L, uint32_t n, const float *states, const float *policies,
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

int spai_ttt_learner_params(spai_ttt_learner *L, float *params, size_t n_params) {
    SPAI_PTR(L);
    SPAI_PTR(params);
    SPAI_SET_DEVICE(L);
    return lc::read_flat(*L, L->p.p, params, n_params);
}

int spai_ttt_learner_grads(spai_ttt_learner *L, float *grads, size_t n_params) {
    SPAI_PTR(L);
    SPAI_PTR(grads);
    SPAI_SET_DEVICE(L);
    return lc::read_flat(*L, L->g.p, grads, n_params);
}

int spai_ttt_learner_activation(spai_ttt_learner *L, int layer, float *out, size_t n) {
    SPAI_PTR(L);
    SPAI_PTR(out);
    SPAI_SET_DEVICE(L);
    SPAI_CHECK(layer >= 0 && (size_t)layer < L->convs.size(), SPAI_ERR_INVALID, "layer %d of %zu", layer,
               L->convs.size());
    SPAI_CHECK(L->last_batch > 0, SPAI_ERR_INVALID, "no train step yet");
    const size_t want = (size_t)L->last_batch * L->convs[layer].co * kCells;
    SPAI_CHECK(n == want, SPAI_ERR_INVALID, "expected %zu activations, got %zu", want, n);
    SPAI_HIP(hipMemcpyAsync(out, L->a[layer].p, n * 4, hipMemcpyDeviceToHost, L->stream));
    SPAI_HIP(hipStreamSynchronize(L->stream));
    return SPAI_OK;
}

int spai_ttt_learner_last_batch(spai_ttt_learner *L, uint32_t *n) {
    SPAI_PTR(L);
    SPAI_PTR(n);
    *n = L->last_batch;
    return SPAI_OK;
}

// weight refresh of a self-play net in place: spai_ttt_net_create's host fold (conv +
// eval-mode BN in double, weights transposed to [ci*9 + tap][co]) into the net's own
// allocations, stream-ordered behind whatever search still reads the old weights
int spai_ttt_net_set_params(spai_ttt_net *net, const float *params, size_t n_params) {
    SPAI_PTR(net);
    SPAI_PTR(params);
    SPAI_SET_DEVICE(net->eng);
    SPAI_CHECK(n_params == num_params(net->blocks), SPAI_ERR_INVALID, "expected %zu params, got %zu",
               num_params(net->blocks), n_params);
    std::vector<float> wt, b;
    const float *p = params;
    auto conv = [&](int ci, int co) {
        const float *w = p, *bias = p + (size_t)co * ci * 9, *bn = bias + co;
        p = bn + 4 * co;
        const size_t base = wt.size();
        wt.resize(base + (size_t)ci * 9 * co);
        for (int o = 0; o < co; ++o) {
            const double sc = (double)bn[o] / std::sqrt((double)bn[3 * co + o] + 1e-5);
            b.push_back((float)(((double)bias[o] - (double)bn[2 * co + o]) * sc + (double)bn[co + o]));
            for (int k = 0; k < ci * 9; ++k) wt[base + (size_t)k * co + o] = (float)((double)w[(size_t)o * ci * 9 + k] * sc);
        }
    };
    conv(3, kHid);
    for (int i = 0; i < 2 * net->blocks; ++i) conv(kHid, kHid);
    conv(kHid, kPolC);
    const float *pl = p;
    p += kCells * kPolK + kCells;
    conv(kHid, kValC);
    const float *vl = p;
    SPAI_CHECK(wt.size() == net->wt.n && b.size() == net->b.n, SPAI_ERR_INVALID, "net allocation does not match");
    hipStream_t st = net->eng->stream;
    SPAI_HIP(hipMemcpyAsync(net->wt.p, wt.data(), 4 * wt.size(), hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(net->b.p, b.data(), 4 * b.size(), hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(net->pl_w.p, pl, 4 * kCells * kPolK, hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(net->pl_b.p, pl + kCells * kPolK, 4 * kCells, hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(net->vl_w.p, vl, 4 * kValK, hipMemcpyHostToDevice, st));
    SPAI_HIP(hipMemcpyAsync(net->vl_b.p, vl + kValK, 4, hipMemcpyHostToDevice, st));
    SPAI_HIP(hipStreamSynchronize(st));   // the host vectors die here
    return SPAI_OK;
}

}  // extern "C"
