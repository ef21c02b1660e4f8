// net_c4_pack.hip — weight refresh of a Connect4 net in place
// (spai_net_set_params, spai_net_set_params_from_learner): the BatchNorm fold
// and the bf16 fragment pack of net_create (net_c4.hip, "host packing"), and
// net_create_f32's layout (net_c4_f32.hip), restated as device kernels that
// gather every packed element from the flat fp32 parameters.
//
// The parameters are either a learner's (spai_learner::p, already on the
// device and on the engine's stream) or a host array uploaded to a staging
// buffer the net keeps.  Everything runs on the engine's stream, so the new
// weights land behind the learner's latest step and behind every search that
// still reads the old ones, and before whatever the engine runs next.
//
// The bar is bit equality with the host pack, which stays the yardstick: the
// same operation order as `fold` (scale = g / sqrt(var + 1e-5f), w * scale,
// (b - mu) * scale + be), no contraction (-ffp-contract=off on both sides),
// correctly rounded fp32 divide and sqrt (hipcc's default), f2bf's integer
// rounding.  One output element per thread; speed is not the point (the whole
// 6 x 64 net is 0.5 M elements).
#include "net_c4_layout.h"
#include "spai_internal.h"

namespace spai {
namespace {

using namespace c4net;

constexpr int kThreads = 256;
constexpr int kFragU16 = 4 * 64 * 8;                    // one k-step of a 64-channel layer: [ct 4][lane 64][8]
constexpr int kLayerU16 = kKStepsRes * kFragU16;        // a trunk or head conv's fragments

// flat parameters in construction order (net_num_params): conv = w [co][ci][3][3], b [co],
// BN gamma, beta, running mean, running var [co] each
__host__ __device__ constexpr size_t conv_floats(int ci, int co) { return (size_t)co * ci * 9 + 5 * (size_t)co; }

struct Src {
    const float *p;
    int blocks;
    __device__ const float *stem() const { return p; }
    __device__ const float *res(int layer) const { return p + conv_floats(3, kHid) + layer * conv_floats(kHid, kHid); }
    __device__ const float *pol() const { return res(2 * blocks); }
    __device__ const float *pol_w() const { return pol() + conv_floats(kHid, 32); }
    __device__ const float *pol_b() const { return pol_w() + 7 * kPolIn; }
    __device__ const float *val() const { return pol_b() + 7; }
    __device__ const float *val_w() const { return val() + conv_floats(kHid, 3); }
    __device__ const float *val_b() const { return val_w() + kValIn; }
};

// a conv's parameters inside the flat array
struct ConvView {
    const float *w, *b, *g, *be, *mu, *var;
    int ci;
};
__device__ __forceinline__ ConvView conv_view(const float *p, int ci, int co) {
    const float *b = p + (size_t)co * ci * 9;
    return ConvView{p, b, b + co, b + 2 * co, b + 3 * co, b + 4 * co, ci};
}

__device__ __forceinline__ uint16_t f2bf_dev(float f) {   // net_c4.hip f2bf: round to nearest even, its NaN rule
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFF) ? 0x40 : 0));
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// net_c4.hip fold, one element: w'[o][ci][tap] and b'[o]
__device__ __forceinline__ float bn_scale(const ConvView &c, int o) { return c.g[o] / sqrtf(c.var[o] + 1e-5f); }
__device__ __forceinline__ float fold_w(const ConvView &c, int o, int i, int tap) {
    return c.w[((size_t)o * c.ci + i) * 9 + tap] * bn_scale(c, o);
}
__device__ __forceinline__ float fold_b(const ConvView &c, int o) {
    return (c.b[o] - c.mu[o]) * bn_scale(c, o) + c.be[o];
}

struct Bf16Dst {
    uint16_t *w_stem, *w_res, *w_head, *w_lin;
    float *b_conv, *b_pol, *b_val;
};

// element counts of the bf16 net's buffers, in the order k_pack_bf16 walks them
struct Bf16Sizes {
    size_t stem, res, head, lin, bias, total;
};
__host__ __device__ inline Bf16Sizes bf16_sizes(int blocks) {
    Bf16Sizes s;
    s.stem = kFragU16;
    s.res = (size_t)2 * blocks * kLayerU16;
    s.head = kLayerU16;
    s.lin = (size_t)kLinBSteps * 64 * 8;
    s.bias = (size_t)(2 * blocks + 2) * kHid;
    s.total = s.stem + s.res + s.head + s.lin + s.bias + 7 + 1;
    return s;
}

// the (co, k) of element e of a [ks][ct 4][lane 64][8] fragment block
__device__ __forceinline__ void frag_cok(size_t e, int &co, int &k) {
    const int j = (int)(e & 7), l = (int)(e >> 3) & 63, ct = (int)(e >> 9) & 3, ks = (int)(e >> 11);
    co = ct * 16 + (l & 15);
    k = ks * 32 + 8 * (l >> 4) + j;
}

__global__ __launch_bounds__(kThreads) void k_pack_bf16(Src S, Bf16Dst D) {
    const Bf16Sizes Z = bf16_sizes(S.blocks);
    size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= Z.total) return;
    if (e < Z.stem) {   // stem fragments [ct 4][lane 64][8]; k = tap*3 + ci for k < 27
        int co, k;
        frag_cok(e, co, k);
        float v = 0.f;
        if (k < 27) v = fold_w(conv_view(S.stem(), 3, kHid), co, k % 3, k / 3);
        D.w_stem[e] = f2bf_dev(v);
        return;
    }
    e -= Z.stem;
    if (e < Z.res) {   // residual convs [layer][ks 18][ct 4][lane 64][8]; k = tap*64 + ci
        const int layer = (int)(e / kLayerU16);
        int co, k;
        frag_cok(e - (size_t)layer * kLayerU16, co, k);
        D.w_res[e] = f2bf_dev(fold_w(conv_view(S.res(layer), kHid, kHid), co, k % kHid, k / kHid));
        return;
    }
    e -= Z.res;
    if (e < Z.head) {   // head conv: co 0..31 policy, 32..34 value, rest zero
        int co, k;
        frag_cok(e, co, k);
        const int tap = k / kHid, ci = k % kHid;
        float v = 0.f;
        if (co < 32) v = fold_w(conv_view(S.pol(), kHid, 32), co, ci, tap);
        else if (co < kHeadC) v = fold_w(conv_view(S.val(), kHid, 3), co - 32, ci, tap);
        D.w_head[e] = f2bf_dev(v);
        return;
    }
    e -= Z.head;
    if (e < Z.lin) {   // fused linear, K halves packed: [ks 24][lane 64][8] over H[s][cell*36 + c]
        const int j = (int)(e & 7), l = (int)(e >> 3) & 63, ks = (int)(e >> 9);
        const int o = l & 7;
        const int k = ((l >> 3) & 1) * (kLinK / 2) + ks * 32 + 8 * (l >> 4) + j;
        const int cell = k / kHC, c = k % kHC;
        float v = 0.f;
        if (k < kLinFeat && o < 7 && c < 32) v = S.pol_w()[(size_t)o * kPolIn + c * c4::kCells + cell];
        else if (k < kLinFeat && o == 7 && c >= 32 && c < kHeadC) v = S.val_w()[(c - 32) * c4::kCells + cell];
        D.w_lin[e] = f2bf_dev(v);
        return;
    }
    e -= Z.lin;
    if (e < Z.bias) {   // conv biases, BN folded: [64 stem | 2*blocks x 64 residual convs | 64 head conv]
        const int layer = (int)(e / kHid), o = (int)(e % kHid), nres = 2 * S.blocks;
        float v = 0.f;
        if (layer == 0) v = fold_b(conv_view(S.stem(), 3, kHid), o);
        else if (layer <= nres) v = fold_b(conv_view(S.res(layer - 1), kHid, kHid), o);
        else if (o < 32) v = fold_b(conv_view(S.pol(), kHid, 32), o);
        else if (o < kHeadC) v = fold_b(conv_view(S.val(), kHid, 3), o - 32);
        D.b_conv[e] = v;
        return;
    }
    e -= Z.bias;
    if (e < 7) D.b_pol[e] = S.pol_b()[e];
    else D.b_val[0] = S.val_b()[0];
}

// ---------------------------------------------------------------- fp32 net
// net_create_f32's buffer: stem W^T [ci][9][co] | stem BN [5][co] | residual W^T x nres |
// residual BN x nres | head W^T [64][9][35] | head BN [5][35] | policy linear w, b | value linear w, b;
// BN rows = conv bias, mean, 1 / sqrt(var + eps), gamma, beta
struct F32Sizes {
    size_t stem_w, stem_bn, res_w, res_bn, head_w, head_bn, pol, val, total;
};
__host__ __device__ inline F32Sizes f32_sizes(int blocks) {
    F32Sizes s;
    const size_t nres = (size_t)2 * blocks;
    s.stem_w = (size_t)3 * 9 * kHid;
    s.stem_bn = 5 * kHid;
    s.res_w = nres * kHid * 9 * kHid;
    s.res_bn = nres * 5 * kHid;
    s.head_w = (size_t)kHid * 9 * kHeadC;
    s.head_bn = 5 * kHeadC;
    s.pol = (size_t)7 * kPolIn + 7;
    s.val = kValIn + 1;
    s.total = s.stem_w + s.stem_bn + s.res_w + s.res_bn + s.head_w + s.head_bn + s.pol + s.val;
    return s;
}

// element e of a conv's W^T [ci][9][co_total] whose column c is output channel o of `cv`
__device__ __forceinline__ float wt_elem(const ConvView &cv, size_t e, int co_total, int o) {
    const size_t it = e / co_total;   // ci * 9 + tap
    return cv.w[(size_t)o * cv.ci * 9 + it];
}
__device__ __forceinline__ float bn_row(const ConvView &cv, int row, int o) {
    return row == 0   ? cv.b[o]
           : row == 1 ? cv.mu[o]
           : row == 2 ? 1.0f / sqrtf(cv.var[o] + 1e-5f)   // oracle bn_relu
           : row == 3 ? cv.g[o]
                      : cv.be[o];
}

__global__ __launch_bounds__(kThreads) void k_pack_f32(Src S, float *__restrict__ out) {
    const F32Sizes Z = f32_sizes(S.blocks);
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= Z.total) return;
    size_t e = idx;
    constexpr size_t kLw = (size_t)kHid * 9 * kHid, kLb = 5 * kHid;
    if (e < Z.stem_w) {
        out[idx] = wt_elem(conv_view(S.stem(), 3, kHid), e, kHid, (int)(e % kHid));
        return;
    }
    e -= Z.stem_w;
    if (e < Z.stem_bn) {
        out[idx] = bn_row(conv_view(S.stem(), 3, kHid), (int)(e / kHid), (int)(e % kHid));
        return;
    }
    e -= Z.stem_bn;
    if (e < Z.res_w) {
        const int layer = (int)(e / kLw);
        e -= layer * kLw;
        out[idx] = wt_elem(conv_view(S.res(layer), kHid, kHid), e, kHid, (int)(e % kHid));
        return;
    }
    e -= Z.res_w;
    if (e < Z.res_bn) {
        const int layer = (int)(e / kLb);
        e -= layer * kLb;
        out[idx] = bn_row(conv_view(S.res(layer), kHid, kHid), (int)(e / kHid), (int)(e % kHid));
        return;
    }
    e -= Z.res_bn;
    if (e < Z.head_w + Z.head_bn) {   // the combined head: policy channels, then the value channels
        const bool bn = e >= Z.head_w;
        if (bn) e -= Z.head_w;
        const int c = (int)(e % kHeadC);
        const ConvView cv = c < 32 ? conv_view(S.pol(), kHid, 32) : conv_view(S.val(), kHid, 3);
        const int o = c < 32 ? c : c - 32;
        out[idx] = bn ? bn_row(cv, (int)(e / kHeadC), o) : wt_elem(cv, e, kHeadC, o);
        return;
    }
    e -= Z.head_w + Z.head_bn;
    if (e < Z.pol) {
        out[idx] = S.pol_w()[e];   // weights, then the 7 biases: contiguous in the parameters too
        return;
    }
    e -= Z.pol;
    out[idx] = S.val_w()[e];
}

// fold and pack the flat device parameters `d_params` into net's own buffers, on st
int pack_into(spai_net *n, const float *d_params, hipStream_t st) {
    const Src S{d_params, n->blocks};
    if (n->dtype == SPAI_DTYPE_F32) {
        const F32Sizes Z = f32_sizes(n->blocks);
        SPAI_CHECK(n->f32.n == Z.total, SPAI_ERR_INVALID, "fp32 net buffer holds %zu floats, expected %zu", n->f32.n,
                   Z.total);
        k_pack_f32<<<(unsigned)((Z.total + kThreads - 1) / kThreads), kThreads, 0, st>>>(S, n->f32.p);
    } else {
        const Bf16Sizes Z = bf16_sizes(n->blocks);
        SPAI_CHECK(n->w_stem.n == Z.stem && n->w_res.n == Z.res && n->w_head.n == Z.head && n->w_lin.n == Z.lin &&
                       n->b_conv.n == Z.bias && n->b_pol.n == 7 && n->b_val.n == 1,
                   SPAI_ERR_INVALID, "bf16 net buffers do not have the sizes of a %d-block net", n->blocks);
        const Bf16Dst D{n->w_stem.p, n->w_res.p, n->w_head.p, n->w_lin.p, n->b_conv.p, n->b_pol.p, n->b_val.p};
        k_pack_bf16<<<(unsigned)((Z.total + kThreads - 1) / kThreads), kThreads, 0, st>>>(S, D);
    }
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

// cached evaluations belong to the previous weights (as spai_engine_set_net); a net
// the engine does not search with leaves the cache alone
int after_refresh(spai_net *n) {
    if (n->eng->net == n) return eval_cache_clear(n->eng);
    return SPAI_OK;
}

}  // namespace

int net_set_params(spai_net *n, const float *params, size_t nparams) {
    const size_t want = net_num_params(n->eng->game, n->blocks, n->hidden);
    SPAI_CHECK(nparams == want, SPAI_ERR_INVALID, "expected %zu params, got %zu", want, nparams);
    if (n->stage.n != want) SPAI_TRY(n->stage.alloc(want));   // once per net
    hipStream_t st = n->eng->stream;
    // behind every earlier reader of the staging buffer and of the weights
    SPAI_HIP(hipMemcpyAsync(n->stage.p, params, want * 4, hipMemcpyHostToDevice, st));
    SPAI_TRY(pack_into(n, n->stage.p, st));
    SPAI_HIP(hipStreamSynchronize(st));   // `params` is the caller's again, the weights are in place
    return after_refresh(n);
}

int net_set_params_from_learner(spai_net *n, spai_learner *l) {
    SPAI_CHECK(l->eng == n->eng, SPAI_ERR_INVALID, "learner belongs to another engine than the net");
    SPAI_CHECK(l->blocks == n->blocks, SPAI_ERR_INVALID, "learner has %d blocks, the net %d", l->blocks, n->blocks);
    SPAI_CHECK(l->hidden == n->hidden, SPAI_ERR_INVALID, "learner has hidden %d, the net %d", l->hidden, n->hidden);
    const size_t want = net_num_params(n->eng->game, n->blocks, n->hidden);
    SPAI_CHECK(l->n_params == want && l->p.n >= want, SPAI_ERR_INVALID, "learner holds %zu params, the net needs %zu",
               l->n_params, want);
    // the learner steps on the engine's stream: the pack reads its latest parameters
    SPAI_TRY(pack_into(n, l->p.p, n->eng->stream));
    return after_refresh(n);
}

}  // namespace spai
