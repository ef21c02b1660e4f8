// learner_common.h — what the device learners share.
//
// All three learners (learner.hip, ttt_learner.hip, chess_learner.hip): the
// fixed-order host sum of a step's loss terms (sum_loss) and Model::train's epoch
// loop (train_epochs).
//
// The TicTacToe and chess learners alone (namespace spai::lc): the state both hold
// (Core), its allocation, the staged train step around a game's own kernels
// (train_batch), the parameter-layout record (Conv, Layout), and the kernels that
// are the same in both: the workgroup reductions, train-mode BatchNorm forward and
// ReLU + BatchNorm backward (templated on the cells of a plane: 9, 64) and Adam.
// The Connect4 learner keeps its own kernels and state (spai_learner).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "spai_internal.h"

namespace spai {

// the ranges of spai_adam_config (include/spai.h), checked by every learner's create
// (cfg NULL: the defaults).  Each comparison is false for a NaN, so a NaN is rejected
// by the range it is held to.  eps > 0: the BN running statistics have g = m = v = 0
// and stay put only because 0 / (0 + eps) is 0.
inline int validate_adam_config(const spai_adam_config *cfg) {
    if (!cfg) return SPAI_OK;
    const auto finite_pos = [](float x) { return x > 0.0f && std::isfinite(x); };
    SPAI_CHECK(cfg->lr >= 0.0f && std::isfinite(cfg->lr), SPAI_ERR_INVALID,
               "adam config: lr must be finite and >= 0 (got %g)", (double)cfg->lr);
    SPAI_CHECK(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f, SPAI_ERR_INVALID,
               "adam config: beta1 must be in [0, 1) (got %g)", (double)cfg->beta1);
    SPAI_CHECK(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f, SPAI_ERR_INVALID,
               "adam config: beta2 must be in [0, 1) (got %g)", (double)cfg->beta2);
    SPAI_CHECK(finite_pos(cfg->eps), SPAI_ERR_INVALID, "adam config: eps must be finite and > 0 (got %g)",
               (double)cfg->eps);
    SPAI_CHECK(cfg->bn_momentum >= 0.0f && cfg->bn_momentum <= 1.0f, SPAI_ERR_INVALID,
               "adam config: bn_momentum must be in [0, 1] (got %g)", (double)cfg->bn_momentum);
    SPAI_CHECK(finite_pos(cfg->bn_eps), SPAI_ERR_INVALID, "adam config: bn_eps must be finite and > 0 (got %g)",
               (double)cfg->bn_eps);
    return SPAI_OK;
}

namespace lc {

// the fixed-order host sums of one step's loss terms [B][2] into loss3 = {total,
// policy, value} (may be NULL); false if a sum is not finite
inline bool sum_loss(const float *terms, uint32_t B, float *loss3) {
    double lp = 0, lv = 0;
    for (uint32_t b = 0; b < B; ++b) {
        lp += terms[2 * b];
        lv += terms[2 * b + 1];
    }
    if (loss3) {
        loss3[1] = (float)(lp / B);
        loss3[2] = (float)(lv / B);
        loss3[0] = loss3[1] + loss3[2];
    }
    return std::isfinite(lp) && std::isfinite(lv);
}

// a fresh Adam: zero moments, step 0 (L: any learner with m, v, n_params, step)
template <class L>
int adam_reset(L &l, hipStream_t st) {
    SPAI_HIP(hipMemsetAsync(l.m.p, 0, l.n_params * 4, st));
    SPAI_HIP(hipMemsetAsync(l.v.p, 0, l.n_params * 4, st));
    l.step = 0;
    return SPAI_OK;
}

// Model::train (model/mod.rs:100-149): a fresh Adam (the reference builds the
// optimizer inside train), one permutation of the n samples (Tensor::randperm,
// here a Philox-keyed Fisher-Yates), then `epochs` passes of ceil(n / batch)
// train steps over the permuted samples (the last batch may be short).  xw, pw:
// floats per state and per policy row; step(m, states, policies, values) trains
// one gathered minibatch.
template <class L, class Step>
int train_epochs(L &l, hipStream_t st, size_t xw, size_t pw, uint32_t n, const float *states, const float *policies,
                 const float *values, uint32_t epochs, uint32_t batch, uint64_t seed, Step &&step) {
    SPAI_CHECK(n >= 1 && batch >= 1, SPAI_ERR_INVALID, "train: need samples and a batch size");
    SPAI_TRY(adam_reset(l, st));
    std::vector<uint32_t> perm;
    choose_multiple(n, n, seed, 0x7EA1Bull, perm);
    batch = std::min(batch, n);   // the same steps from smaller host buffers
    std::vector<float> s((size_t)batch * xw), p((size_t)batch * pw), v(batch);
    const uint32_t nb = (n + batch - 1) / batch;
    for (uint32_t ep = 0; ep < epochs; ++ep)
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t lo = b * batch, m = std::min(batch, n - lo);
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t j = perm[lo + i];
                memcpy(&s[(size_t)i * xw], states + (size_t)j * xw, xw * 4);
                memcpy(&p[(size_t)i * pw], policies + (size_t)j * pw, pw * 4);
                v[i] = values[j];
            }
            SPAI_TRY(step(m, s.data(), p.data(), v.data()));
        }
    return SPAI_OK;
}

// ------------------------------------------------------------------ host state
struct Conv {
    int ci, co;
    size_t w, b, g, be, mu, var;   // offsets into the flat parameter vector
};

// the flat parameter vector in construction order
struct Layout {
    size_t off = 0;
    size_t take(size_t n) {
        const size_t o = off;
        off += n;
        return o;
    }
    Conv conv3x3_bn(int ci, int co) {   // conv w, b, then BN gamma, beta, running mean, running variance
        Conv c{};
        c.ci = ci;
        c.co = co;
        c.w = take((size_t)co * ci * 9);
        c.b = take(co);
        c.g = take(co);
        c.be = take(co);
        c.mu = take(co);
        c.var = take(co);
        return c;
    }
};

struct Core {
    int device = 0;
    hipStream_t stream = nullptr;          // the engine's
    spai_adam_config cfg{};
    uint64_t step = 0;
    uint32_t max_batch = 0, last_batch = 0;
    size_t n_params = 0;
    size_t xw = 0, pw = 0;                 // floats per sample: input planes, policy
    DevBuf<float> p, g, m, v;              // parameters, gradients, Adam moments (flat)
    DevBuf<float> batch_in;                // [x: B*xw | pi: B*pw | z: B]
    float *stage = nullptr;                // its pinned host copy, then the loss terms [B*2]
    DevBuf<float> dpre, terms;             // value pre-tanh gradient [B]; loss terms [B][2]
    size_t row() const { return xw + pw + 1; }
};

// a new learner's fields: the engine's device and stream, the Adam config (NULL:
// defaults; out of range: SPAI_ERR_INVALID), the row widths
inline int core_setup(Core &c, int device, hipStream_t stream, size_t n_params, const spai_adam_config *cfg,
                      size_t xw, size_t pw) {
    SPAI_TRY(validate_adam_config(cfg));
    c.device = device;
    c.stream = stream;
    c.n_params = n_params;
    if (cfg) c.cfg = *cfg;
    else (void)spai_adam_config_default(&c.cfg);
    c.xw = xw;
    c.pw = pw;
    return SPAI_OK;
}

// allocate and upload the parameters, zero the gradients and the moments
inline int core_init(Core &c, const float *params) {
    const size_t n = c.n_params;
    for (auto *d : {&c.p, &c.g, &c.m, &c.v}) SPAI_TRY(d->alloc(n));
    SPAI_HIP(hipMemcpyAsync(c.p.p, params, n * 4, hipMemcpyHostToDevice, c.stream));
    for (auto *d : {&c.g, &c.m, &c.v}) SPAI_HIP(hipMemsetAsync(d->p, 0, n * 4, c.stream));
    SPAI_HIP(hipStreamSynchronize(c.stream));   // params is the caller's
    return SPAI_OK;
}

inline void core_free(Core &c) {
    for (auto *d : {&c.p, &c.g, &c.m, &c.v, &c.batch_in, &c.dpre, &c.terms}) d->release();
    if (c.stage) (void)hipHostFree(c.stage);
    c.stage = nullptr;
}

// the core's half of growing to batches of B > max_batch: drains the stream, leaves
// max_batch 0 (the caller sets it once its own buffers are grown too)
inline int core_grow_batch(Core &c, uint32_t B) {
    SPAI_HIP(hipStreamSynchronize(c.stream));   // nothing in flight reads the old buffers
    c.max_batch = 0;
    c.last_batch = 0;
    SPAI_TRY(c.dpre.alloc(B));
    SPAI_TRY(c.terms.alloc((size_t)B * 2));
    SPAI_TRY(c.batch_in.alloc((size_t)B * c.row()));
    if (c.stage) (void)hipHostFree(c.stage);
    c.stage = nullptr;
    SPAI_HIP(hipHostMalloc((void **)&c.stage, (size_t)B * (c.row() + 2) * sizeof(float), hipHostMallocDefault));
    return SPAI_OK;
}

// what follows a batch's way into batch_in, whatever brought it there (the upload
// below, or work already enqueued on the stream: the chess learner's compact
// samples): the game's enqueue_step(B), the loss terms back, one synchronisation,
// the loss sums.  finite (may be NULL): whether the loss sums are finite.
template <class Enqueue>
int run_step(Core &c, uint32_t B, float *loss3, bool *finite, Enqueue &&enqueue_step) {
    hipStream_t st = c.stream;
    SPAI_TRY(enqueue_step((int)B));
    float *terms = c.stage + (size_t)B * c.row();
    SPAI_HIP(hipMemcpyAsync(terms, c.terms.p, (size_t)B * 2 * 4, hipMemcpyDeviceToHost, st));
    SPAI_HIP(hipStreamSynchronize(st));
    const bool ok = sum_loss(terms, B, loss3);
    if (finite) *finite = ok;
    return SPAI_OK;
}

// one train step on B <= max_batch samples: stage and upload the batch, then run_step
template <class Enqueue>
int train_batch(Core &c, uint32_t B, const float *states, const float *policies, const float *values, float *loss3,
                bool *finite, Enqueue &&enqueue_step) {
    memcpy(c.stage, states, (size_t)B * c.xw * 4);
    memcpy(c.stage + (size_t)B * c.xw, policies, (size_t)B * c.pw * 4);
    memcpy(c.stage + (size_t)B * (c.xw + c.pw), values, (size_t)B * 4);
    SPAI_HIP(hipMemcpyAsync(c.batch_in.p, c.stage, (size_t)B * c.row() * 4, hipMemcpyHostToDevice, c.stream));
    return run_step(c, B, loss3, finite, enqueue_step);
}

// the parameters or the gradients to the host
inline int read_flat(Core &c, const float *src, float *dst, size_t n) {
    SPAI_CHECK(n == c.n_params, SPAI_ERR_INVALID, "expected %zu params, got %zu", c.n_params, n);
    SPAI_HIP(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, c.stream));
    SPAI_HIP(hipStreamSynchronize(c.stream));
    return SPAI_OK;
}

// ------------------------------------------------------------------ device
constexpr int kBnThreads = 256;

// the workgroup's sum in a fixed order (every thread gets it)
__device__ __forceinline__ float block_sum(float v, float *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = kBnThreads / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = sh[t] + sh[t + o];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_max(float v, float *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = kBnThreads / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] = fmaxf(sh[t], sh[t + o]);
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// element i = CELLS * sample + cell of channel c in [B][C][CELLS].  A power of two
// divides unsigned, so the split is a shift and a mask; 9 divides as it always has
// (both compile to the code the two learners had when each carried these kernels)
template <int CELLS>
__device__ __forceinline__ size_t plane_index(int i, int C, int c) {
    const int s = (CELLS & (CELLS - 1)) == 0 ? (int)((unsigned)i / (unsigned)CELLS) : i / CELLS;
    return ((size_t)s * C + c) * CELLS + (i - CELLS * s);
}

// train-mode BatchNorm of channel blockIdx.x over the CELLS B values z[:, c, :]: batch
// mean and biased variance, a = relu(gamma xhat + beta (+ res)), and the running
// statistics (momentum, unbiased variance)
template <int CELLS>
__global__ __launch_bounds__(kBnThreads) void k_lc_bn_fwd(const float *__restrict__ z, int C, int B,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float *__restrict__ run_mu,
                                                          float *__restrict__ run_var, const float *__restrict__ res,
                                                          float *__restrict__ a, float *__restrict__ mean_out,
                                                          float *__restrict__ invstd_out, float momentum, float eps) {
    __shared__ float sh[kBnThreads];
    const int c = blockIdx.x, t = threadIdx.x, nn = CELLS * B;
    float acc = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) acc += z[plane_index<CELLS>(i, C, c)];
    const float mean = block_sum(acc, sh) / (float)nn;
    acc = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) {
        const float d = z[plane_index<CELLS>(i, C, c)] - mean;
        acc += d * d;
    }
    const float var = block_sum(acc, sh) / (float)nn;
    const float invstd = 1.0f / sqrtf(var + eps);
    const float g = gamma[c], be = beta[c];
    for (int i = t; i < nn; i += kBnThreads) {
        const size_t idx = plane_index<CELLS>(i, C, c);
        float yv = g * ((z[idx] - mean) * invstd) + be;
        if (res) yv += res[idx];
        a[idx] = fmaxf(yv, 0.0f);
    }
    if (t == 0) {
        mean_out[c] = mean;
        invstd_out[c] = invstd;
        run_mu[c] = (1.0f - momentum) * run_mu[c] + momentum * mean;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (var * ((float)nn / (float)(nn - 1)));
    }
}

// backward of ReLU + BatchNorm for channel blockIdx.x: dy = da [a > 0];
// dbeta = sum dy, dgamma = sum dy xhat, dz = gamma invstd / nn (nn dy - dbeta - xhat dgamma),
// dbias = sum dz.  keep_dy: da becomes dy (the skip connection's gradient).
template <int CELLS>
__global__ __launch_bounds__(kBnThreads) void k_lc_bn_bwd(float *__restrict__ da, const float *__restrict__ a,
                                                          const float *__restrict__ z, int C, int B,
                                                          const float *__restrict__ mean,
                                                          const float *__restrict__ invstd,
                                                          const float *__restrict__ gamma, float *__restrict__ dz,
                                                          float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                          float *__restrict__ g_bias, int keep_dy) {
    __shared__ float sh[kBnThreads];
    const int c = blockIdx.x, t = threadIdx.x, nn = CELLS * B;
    const float mu = mean[c], is = invstd[c];
    float sb = 0.0f, sg = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) {
        const size_t idx = plane_index<CELLS>(i, C, c);
        const float dy = a[idx] > 0.0f ? da[idx] : 0.0f;
        sb += dy;
        sg += dy * ((z[idx] - mu) * is);
    }
    sb = block_sum(sb, sh);
    sg = block_sum(sg, sh);
    const float k = gamma[c] * is / (float)nn;
    float sz = 0.0f;
    for (int i = t; i < nn; i += kBnThreads) {
        const size_t idx = plane_index<CELLS>(i, C, c);
        const float dy = a[idx] > 0.0f ? da[idx] : 0.0f;
        const float v = k * ((float)nn * dy - sb - ((z[idx] - mu) * is) * sg);
        dz[idx] = v;
        if (keep_dy) da[idx] = dy;
        sz += v;
    }
    sz = block_sum(sz, sh);
    if (t == 0) {
        g_gamma[c] = sg;
        g_beta[c] = sb;
        g_bias[c] = sz;
    }
}

// Adam, torch semantics (as learner.hip): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  The BN running
// statistics have gradient 0, so their moments stay 0 and they do not move.
// (static: a copy per translation unit that launches it, as a kernel cannot be inline)
static __global__ void k_lc_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                 float *__restrict__ v, size_t n, float lr, float b1, float b2, float eps, float bc1,
                                 float bc2_sqrt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
}

// the step's Adam update: advances step, the bias corrections in double on the host
static inline void adam_step(Core &c) {
    c.step += 1;
    const double t = (double)c.step;
    const float bc1 = (float)(1.0 - std::pow((double)c.cfg.beta1, t));
    const float bc2 = (float)std::sqrt(1.0 - std::pow((double)c.cfg.beta2, t));
    k_lc_adam<<<(unsigned)((c.n_params + 255) / 256), 256, 0, c.stream>>>(c.p.p, c.g.p, c.m.p, c.v.p, c.n_params,
                                                                         c.cfg.lr, c.cfg.beta1, c.cfg.beta2, c.cfg.eps,
                                                                         bc1, bc2);
}

}  // namespace lc
}  // namespace spai
