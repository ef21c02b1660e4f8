// dirichlet.h — one Dirichlet(alpha, ..., alpha) draw per tree by one wavefront:
// the root exploration noise of AlphaZero self-play, which the reference leaves
// open (mcts.rs:204-207, "TODO: Add Dirichlet noise").  Device only.
//
// wave_dirichlet(seed, game_id, move_no, n, alpha, lane, eta) is called by all 64
// lanes of a wave.  Lane l owns children l, l + 64, l + 128, l + 192 (n <= 218,
// kDirichletMaxN = 256), and eta[k] receives the component of child l + 64 k (0
// for a child >= n).  The draw is a function of (seed, game_id, move_no, n,
// alpha) alone: every reduction below runs over the wave in a fixed xor-butterfly
// order, and nothing reads the tree index, the batch position, the number of
// trees or the launch shape.
//
// Uniforms.  Philox4x32-10 (philox.h) under
//     key     = seed ^ kDirichletDomain               (low word, high word)
//     counter = { game_id low, game_id high, move_no, child | attempt << 8 }
// with child in [0, 256) and attempt in [0, 64).  The move draw of self-play
// (sample_u01_f32) runs under the plain seed with the counter (move, game), so
// the two streams never share a (key, counter) pair.  The four words of one
// block serve one Marsaglia-Tsang attempt of one child:
//     word 0, 1   the Box-Muller pair of the attempt's normal
//     word 2      the attempt's acceptance uniform
//     word 3      (attempt 0 only) the boost uniform of alpha < 1
// A word w becomes the uniform ((w >> 9) + 0.5) * 2^-23, which lies in (0, 1)
// and is exact in float32, so no logarithm below sees 0.
//
// Gamma(alpha, 1) per child, Marsaglia-Tsang on the shape a = alpha (alpha >= 1)
// or alpha + 1 (alpha < 1):  d = a - 1/3, c = 1 / sqrt(9 d); x normal, v = (1 + c
// x)^3, accepted when v > 0 and log u < x^2 / 2 + d - d v + d log v; the draw is d
// v.  At most 64 attempts: after the 64th the last candidate with v > 0 stands (v
// = 1 if there was none), so no lane can spin.  For alpha < 1 the draw is boosted
// by U^(1 / alpha).
//
// All of it in the log domain: log g = log d + log v (+ log U / alpha).  The wave's
// largest log g is subtracted before exponentiating, so the largest component is
// exactly exp(0) = 1 before the division, the sum is >= 1 and the result is never
// 0 / 0 or NaN for any alpha in [0.01, 100]; a tiny component may underflow to 0.
//
// The search mixes the draw into the root children's priors once per search call
// (k_croot_noise, chess_search.hip): P <- (1 - eps) * P + eps * eta.  A root that is
// searched twice without a move in between is therefore mixed twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace spai {

constexpr uint64_t kDirichletDomain = 0xD1A1C4E7B0075EEDull;
constexpr int kDirichletMaxN = 256;
constexpr int kDirichletAttempts = 64;

__device__ __forceinline__ float dirichlet_u01(uint32_t w) {
    return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-7f;   // 2^-23; exact
}

// log of one Gamma(alpha, 1) draw of child `child`
__device__ inline float dirichlet_log_gamma(const uint32_t key[2], uint64_t game_id, uint32_t move_no, uint32_t child,
                                            float alpha) {
    const float a = alpha >= 1.0f ? alpha : alpha + 1.0f;
    const float d = a - 1.0f / 3.0f;
    const float c = 1.0f / sqrtf(9.0f * d);
    float logv = 0.0f;    // the candidate that stands when every attempt is rejected
    float boost = 0.0f;
    for (int attempt = 0; attempt < kDirichletAttempts; ++attempt) {
        uint32_t ctr[4] = {(uint32_t)game_id, (uint32_t)(game_id >> 32), move_no, child | ((uint32_t)attempt << 8)};
        uint32_t w[4];
        philox4x32(ctr, key, w);
        if (attempt == 0 && alpha < 1.0f) boost = logf(dirichlet_u01(w[3])) / alpha;
        const float r = sqrtf(-2.0f * logf(dirichlet_u01(w[0])));
        const float x = r * cosf(6.283185307179586f * dirichlet_u01(w[1]));
        const float t = 1.0f + c * x;
        if (!(t > 0.0f)) continue;
        const float v = t * t * t;
        logv = 3.0f * logf(t);
        if (logf(dirichlet_u01(w[2])) < 0.5f * x * x + d - d * v + d * logv) break;
    }
    return logf(d) + logv + boost;
}

__device__ inline void wave_dirichlet(uint64_t seed, uint64_t game_id, uint32_t move_no, uint32_t n, float alpha,
                                      int lane, float eta[4]) {
    const uint64_t k64 = seed ^ kDirichletDomain;
    const uint32_t key[2] = {(uint32_t)k64, (uint32_t)(k64 >> 32)};
    float lg[4];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t j = (uint32_t)lane + 64u * k;
        lg[k] = j < n ? dirichlet_log_gamma(key, game_id, move_no, j, alpha) : -INFINITY;
        mx = fmaxf(mx, lg[k]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t j = (uint32_t)lane + 64u * k;
        eta[k] = j < n ? expf(lg[k] - mx) : 0.0f;
        sum = sum + eta[k];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum = sum + __shfl_xor(sum, o, 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) eta[k] = eta[k] / sum;
}

// the mix of one prior with its noise component, each operation rounded on its own;
// one_minus_eps = 1.0f - eps, rounded once by the caller
__device__ __forceinline__ float dirichlet_mix(float prior, float eta, float one_minus_eps, float eps) {
    const float a = __fmul_rn(one_minus_eps, prior);
    const float b = __fmul_rn(eps, eta);
    return __fadd_rn(a, b);
}

}  // namespace spai
