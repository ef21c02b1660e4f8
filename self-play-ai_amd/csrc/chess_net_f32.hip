// chess_net_f32.hip — the chess ResNet forward in fp32 (spai_chess_net_create_dtype
// with SPAI_DTYPE_F32): the reference's own arithmetic, for parity work.  The chess
// counterpart of net_c4_f32.hip.
//
// Reference: model/mod.rs:152-184 (stem conv3x3 + BN + ReLU, residual blocks
// relu(x + BN(conv(relu(BN(conv(x)))))) ), model/chess.rs:48-77 (policy head
// conv1x1 256->256 + ReLU + conv1x1 256->73, flattened NCHW; value head conv1x1
// 256->1 + ReLU + linear 64->256 + ReLU + linear 256->1 + tanh).  The reference
// computes all of this in fp32 through libtorch (model/mod.rs:36-98).
//
// Every output element is summed in ONE fixed order, with separate multiply and
// add (-ffp-contract=off):
//  * conv: the conv bias first, then the products input channel ascending, kernel
//    row, kernel column; an off-board tap is skipped;
//  * BatchNorm unfolded: ((x - mean) * inv) * gamma + beta with inv =
//    1 / sqrt(var + 1e-5) computed on the host in float32;
//  * residual: relu(h + bn(conv(...))), the block input as the left operand;
//  * heads (conv1x1 and linears): the bias first, then the input index ascending.
// A numpy float32 restatement of that order (tests/chess_f32_ref.py) reproduces
// every logit and the value's pre-activation bit for bit; only tanhf (device libm
// vs the host's) may differ in the last ulp.
//
// Layout: one workgroup of 256 threads per position.  Thread t owns output
// channel t and keeps its 64 cells' sums in registers.  Activations live in LDS
// as two unpadded fp32 [64 cells][256 channels] buffers (2 x 64 KiB) beside the
// 19 input planes: 132.75 KiB of the CU's 160 KiB (two zero-bordered 10 x 10
// buffers would not fit, so the taps are resolved at compile time instead: the
// cell and tap loops are fully unrolled and an off-board tap emits nothing).
// Conv2 of a block reads buffer B and updates buffer A in place: a thread touches
// only its own channel of A.  Weights are stored [ci][tap][co], so a wave reads
// 64 consecutive floats, and an activation read is a wave-uniform LDS broadcast.
// A position's result depends on nothing but its own input: not on its batch
// slot, nor on what else is in the launch.  Throughput is not the point of this
// kernel; the bf16 MFMA kernel (chess_net.hip) is the production path.
#include <cmath>
#include <vector>

#include "chess_engine.h"

namespace spai {
namespace chess {
namespace {

constexpr int kHid = 256;
constexpr int kThreads = 256;
constexpr int kPolCo = 73;

// LDS carve (floats)
constexpr int kA = 0;                        // [64][256]
constexpr int kB = kA + 64 * kHid;           // [64][256]
constexpr int kX = kB + 64 * kHid;           // input planes [19][64]; after the stem: value-head scratch
constexpr int kLdsFloats = kX + kPlanes * 64;
constexpr int kVCell = kX, kVHid = kX + 64;   // value conv [64], linear 1 [256]

// device views of the flat fp32 buffer: conv weights [ci][tap][co]; BN rows [5][co] =
// conv bias, mean, inv, gamma, beta
struct F32W {
    const float *stem_w, *stem_bn;
    const float *res_w, *res_bn;   // layer l at + l * (256*9*256) / + l * (5*256)
    const float *p1_w, *p1_b;      // [256][256], [256]
    const float *p2_w, *p2_b;      // [256][73], [73]
    const float *v_w, *v_b;        // [256], [1]
    const float *l1_w, *l1_b;      // [256][64] (as given), [256]
    const float *l2_w, *l2_b;      // [256], [1]
    int blocks;
};

// inlined on purpose: out of line, the 64 sums and 64 activations a call keeps live
// cost scratch memory around it.
// in: element (cell, ci) at in[cell * CS + ci * IS].
// MODE 0: relu(BN(conv)) -> out[cell][co]
// MODE 1: relu(out + BN(conv)) -> out (residual; `out` holds the block input)
// MODE 2: relu(conv) -> out[cell][co]           (bn = the bias alone)
// MODE 3: conv -> global out[co * 64 + cell]    (bn = the bias alone)
template <int CI, int TAPS, int CS, int IS, int CO, int MODE>
__device__ __forceinline__ void conv_f32(const float *in, float *out, const float *__restrict__ W,
                                         const float *__restrict__ bn, int tid) {
    const int co = tid;
    if (co >= CO) return;
    float acc[64];
    const float bias = bn[co];
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = bias;
    for (int i = 0; i < CI; ++i) {
        float a[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) a[c] = in[c * CS + i * IS];
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const float wv = W[((size_t)i * TAPS + tap) * CO + co];
            const int dy = TAPS == 9 ? tap / 3 - 1 : 0, dx = TAPS == 9 ? tap % 3 - 1 : 0;
#pragma unroll
            for (int c = 0; c < 64; ++c) {
                const int y = (c >> 3) + dy, x = (c & 7) + dx;
                if (y < 0 || y > 7 || x < 0 || x > 7) continue;   // off-board: compile-time
                acc[c] = acc[c] + wv * a[y * 8 + x];
            }
        }
    }
    float mu = 0.0f, inv = 1.0f, gm = 1.0f, be = 0.0f;
    if (MODE <= 1) {
        mu = bn[CO + co];
        inv = bn[2 * CO + co];
        gm = bn[3 * CO + co];
        be = bn[4 * CO + co];
    }
#pragma unroll
    for (int c = 0; c < 64; ++c) {
        float v = acc[c];
        if (MODE <= 1) v = ((v - mu) * inv) * gm + be;
        if (MODE == 1) v = out[c * kHid + co] + v;
        if (MODE != 3 && v < 0.0f) v = 0.0f;
        if (MODE == 3) out[co * 64 + c] = v;
        else out[c * kHid + co] = v;
    }
}

// One position per workgroup: x [n][19][64] -> logits [n][4672], value [n]
__global__ __launch_bounds__(kThreads) void k_chess_f32_forward(const uint32_t *__restrict__ d_count, uint32_t max_n,
                                                                const float *__restrict__ x, F32W P,
                                                                float *__restrict__ logits,
                                                                float *__restrict__ value) {
    __shared__ float s[kLdsFloats];
    const uint32_t count = d_count ? min(*d_count, max_n) : max_n;
    const uint32_t slot = blockIdx.x;
    if (slot >= count) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < kPlanes * 64; i += kThreads) s[kX + i] = x[(size_t)slot * kPlanes * 64 + i];
    __syncthreads();
    conv_f32<kPlanes, 9, 1, 64, kHid, 0>(s + kX, s + kA, P.stem_w, P.stem_bn, tid);
    __syncthreads();
    constexpr size_t kLw = (size_t)kHid * 9 * kHid, kLb = 5 * kHid;
    for (int b = 0; b < P.blocks; ++b) {
        conv_f32<kHid, 9, kHid, 1, kHid, 0>(s + kA, s + kB, P.res_w + (2 * b) * kLw, P.res_bn + (2 * b) * kLb, tid);
        __syncthreads();
        conv_f32<kHid, 9, kHid, 1, kHid, 1>(s + kB, s + kA, P.res_w + (2 * b + 1) * kLw, P.res_bn + (2 * b + 1) * kLb,
                                            tid);
        __syncthreads();
    }
    // policy head: conv1x1 256->256 + ReLU (A -> B), then conv1x1 256->73 (B -> logits)
    conv_f32<kHid, 1, kHid, 1, kHid, 2>(s + kA, s + kB, P.p1_w, P.p1_b, tid);
    // value head: conv1x1 256->1 + ReLU over the torso output in A, thread = cell
    if (tid < 64) {
        float acc = P.v_b[0];
        for (int i = 0; i < kHid; ++i) acc = acc + P.v_w[i] * s[kA + tid * kHid + i];
        s[kVCell + tid] = acc < 0.0f ? 0.0f : acc;
    }
    __syncthreads();
    conv_f32<kHid, 1, kHid, 1, kPolCo, 3>(s + kB, logits + (size_t)slot * kPolicy, P.p2_w, P.p2_b, tid);
    {   // linear 64 -> 256 + ReLU, thread = output
        float h = P.l1_b[tid];
        const float *w = P.l1_w + (size_t)tid * 64;
        for (int c = 0; c < 64; ++c) h = h + w[c] * s[kVCell + c];
        s[kVHid + tid] = h < 0.0f ? 0.0f : h;
    }
    __syncthreads();
    if (tid == 0) {   // linear 256 -> 1, tanh
        float acc = P.l2_b[0];
        for (int j = 0; j < kHid; ++j) acc = acc + P.l2_w[j] * s[kVHid + j];
        value[slot] = tanhf(acc);
    }
}

F32W weights_f32(const spai_chess_net *n) {
    const float *b = n->wf.p;
    const size_t nres = (size_t)2 * n->blocks;
    F32W P;
    size_t o = 0;
    P.stem_w = b + o; o += (size_t)kPlanes * 9 * kHid;
    P.stem_bn = b + o; o += 5 * kHid;
    P.res_w = b + o; o += nres * kHid * 9 * kHid;
    P.res_bn = b + o; o += nres * 5 * kHid;
    P.p1_w = b + o; o += (size_t)kHid * kHid;
    P.p1_b = b + o; o += kHid;
    P.p2_w = b + o; o += (size_t)kHid * kPolCo;
    P.p2_b = b + o; o += kPolCo;
    P.v_w = b + o; o += kHid;
    P.v_b = b + o; o += 1;
    P.l1_w = b + o; o += (size_t)256 * 64;
    P.l1_b = b + o; o += 256;
    P.l2_w = b + o; o += 256;
    P.l2_b = b + o;
    P.blocks = n->blocks;
    return P;
}

}  // namespace

// params in construction order (net_num_params) -> the flat fp32 image weights_f32 reads
void net_f32_pack(int blocks, const float *params, std::vector<float> &buf) {
    buf.clear();
    buf.reserve(net_num_params(blocks));
    const float *p = params;
    // conv w [co][ci][k][k] -> W^T [ci][tap][co]
    auto conv_w = [&](int ci, int co, int taps) {
        const size_t base = buf.size();
        buf.resize(base + (size_t)ci * taps * co);
        for (int o = 0; o < co; ++o)
            for (int i = 0; i < ci; ++i)
                for (int tap = 0; tap < taps; ++tap)
                    buf[base + ((size_t)i * taps + tap) * co + o] = p[((size_t)o * ci + i) * taps + tap];
        p += (size_t)co * ci * taps;
    };
    auto copy = [&](size_t n) {
        buf.insert(buf.end(), p, p + n);
        p += n;
    };
    // conv bias [co] + BN (gamma, beta, mean, var) -> rows bias, mean, inv, gamma, beta
    auto bn_rows = [&](int co, std::vector<float> &rows) {
        const float *cb = p, *g = cb + co, *be = g + co, *mu = be + co, *var = mu + co;
        const size_t base = rows.size();
        rows.resize(base + (size_t)5 * co);
        for (int o = 0; o < co; ++o) {
            rows[base + 0 * co + o] = cb[o];
            rows[base + 1 * co + o] = mu[o];
            rows[base + 2 * co + o] = 1.0f / sqrtf(var[o] + 1e-5f);
            rows[base + 3 * co + o] = g[o];
            rows[base + 4 * co + o] = be[o];
        }
        p += (size_t)5 * co;
    };
    conv_w(kPlanes, kHid, 9);
    bn_rows(kHid, buf);
    std::vector<float> rbn;
    for (int l = 0; l < 2 * blocks; ++l) {
        conv_w(kHid, kHid, 9);
        bn_rows(kHid, rbn);
    }
    buf.insert(buf.end(), rbn.begin(), rbn.end());
    conv_w(kHid, 256, 1);
    copy(256);
    conv_w(256, kPolCo, 1);
    copy(kPolCo);
    copy(kHid + 1);            // value conv w [1][256], b
    copy(64 * 256 + 256);      // linear 1 w [256][64], b
    copy(256 + 1);             // linear 2 w [1][256], b
}

// `count` (device scalar, or max_n when null) positions of xf [max_n][19][64]; the grid covers max_n
int net_f32_launch(spai_chess_net *n, hipStream_t st, const uint32_t *d_count, uint32_t max_n, const float *xf,
                   float *logits, float *value) {
    if (!max_n) return SPAI_OK;
    SPAI_CHECK(xf, SPAI_ERR_INVALID, "internal: an fp32 chess net needs the fp32 input planes");
    k_chess_f32_forward<<<max_n, kThreads, 0, st>>>(d_count, max_n, xf, weights_f32(n), logits, value);
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

}  // namespace chess
}  // namespace spai
