// chess_net_pack.hip — weight refresh of a chess net in place
// (spai_chess_net_set_params, spai_chess_net_set_params_from_learner) and the
// checker's window on the packed weights (spai_chess_net_image): net_create's host
// fold and pack (pack_params / pack_conv in chess_net.hip) and the fp32 net's layout
// (net_f32_pack in chess_net_f32.hip), restated as device kernels that read the flat
// fp32 parameters.  The chess counterpart of net_c4_pack.hip.
//
// The parameters are either a learner's (lc::Core::p, already on the device and on
// the engine's stream) or a host array uploaded to a staging buffer the net keeps.
// Everything runs on the engine's stream, so the new weights land behind the
// learner's latest step and behind every search that still reads the old ones, and
// before whatever the engine runs next.  spai_chess_match_run's second chain has a
// stream of its own, but every return of a match drains both streams (Quiesce in
// chess_match.hip), so no match can still be reading the weights when a refresh is
// enqueued: nothing more is needed to order the two.
//
// The bar is bit equality with the host pack, which stays the yardstick (net_create
// keeps using it).  bf16 net: the fold is in double, in the host's operation order:
//   sc = (double)gamma / sqrt((double)var + 1e-5)
//   w' = bf16((float)((double)w * sc))          double -> float -> bf16, both roundings
//   b' = (float)(((double)b - (double)mu) * sc + (double)beta)
// with no contraction (-ffp-contract=off is global in the Makefile, for both sides;
// this file relies on it), the compiler's correctly rounded double divide and square
// root (no fast-math), and f2bf's integer rounding copied.  A padded element
// (o >= co or i >= ci) is bf16 zero and is written on every refresh.  NaN parameters
// are outside the claim: a host NaN's sign and payload need not match the device's.
//
// Shape.  The net is 24 M elements at 20 blocks, so the pack is a memory problem:
// one read of the parameters, one write of the fragments.  A workgroup owns one
// (layer, co tile of 16, ci block of 32): its source is 16 runs of 32 * taps
// consecutive floats, loaded coalesced into LDS; it then writes, per tap, the 64
// lanes x 8 bf16 of that k-step as one 16-byte store per thread, 1 KiB contiguous.
// Every source float is read once and no store is narrower than 16 bytes.  The 16
// scales a workgroup needs are computed by its first 16 threads (a double divide and
// square root each, recomputed by the CB workgroups that share a co tile: nothing
// beside 18 KiB of loads), so the fold needs no prepass and no scratch buffer; the
// ci block 0 workgroups write the folded biases.  The fp32 net's W^T is a tiled
// transpose through LDS, coalesced on both sides.
#include "chess_engine.h"

namespace spai {
namespace chess {
namespace {

// the bf16 net's geometry (chess_net.hip: kHid, kCT, kPolCT) and the policy head's width
constexpr int kHid = 256;
constexpr int kCT = kHid / 16;
constexpr int kPolC = 73;
constexpr int kPolCT = 5;
constexpr int kThreads = 256;

// offsets into the flat parameters in construction order (net_num_params): conv3x3 w
// [256][ci][3][3], b, BN gamma, beta, running mean, running var [256] each; then the
// policy convs, the value conv and the two linears, w then b
struct Offsets {
    size_t res0, res_stride, p1_w, p1_b, p2_w, p2_b, v_w, v_b, l1_w, l1_b, l2_w, l2_b, end;
};
Offsets offsets(int blocks) {
    auto conv = [](size_t ci) { return (size_t)kHid * ci * 9 + 5 * (size_t)kHid; };
    Offsets o;
    o.res0 = conv(kPlanes);
    o.res_stride = conv(kHid);
    o.p1_w = o.res0 + (size_t)2 * blocks * o.res_stride;
    o.p1_b = o.p1_w + (size_t)kHid * kHid;
    o.p2_w = o.p1_b + kHid;
    o.p2_b = o.p2_w + (size_t)kPolC * kHid;
    o.v_w = o.p2_b + kPolC;
    o.v_b = o.v_w + kHid;
    o.l1_w = o.v_b + 1;
    o.l1_b = o.l1_w + (size_t)kHid * 64;
    o.l2_w = o.l1_b + kHid;
    o.l2_b = o.l2_w + kHid;
    o.end = o.l2_b + 1;
    return o;
}

__device__ __forceinline__ uint16_t f2bf_dev(float f) {   // chess_net.hip f2bf: round to nearest even, its NaN rule
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFF) ? 0x40 : 0));
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ---------------------------------------------------------------- bf16 net
// one conv of `layers` equally shaped layers, `src_stride` floats and `dst_stride`
// bf16 apart: w [co][ci][TAPS] (+ b and the BN rows behind it when bn) -> fragments
// [ks = tap*CB + cb][ct][lane 64][8], o = ct*16 + (lane & 15), i = cb*32 + (lane >> 4)*8 + j
struct ConvJob {
    const float *src;
    size_t src_stride;
    uint16_t *dst;
    size_t dst_stride;
    float *bias;   // [layer][co] folded biases (bn only)
    int ci, co, CB, CT, bn;
};

template <int TAPS>
__global__ __launch_bounds__(kThreads) void k_chess_pack_conv(ConvJob J) {
    constexpr int kRun = 32 * TAPS;   // a row's floats: 32 input channels x taps, consecutive in the source
    constexpr int kRow = kRun + 1;    // padded: the 16 rows a wave reads start in 16 different banks
    __shared__ float tile[16 * kRow];
    __shared__ double sc[16];
    const int tid = threadIdx.x;
    const int ct = blockIdx.x / J.CB, cb = blockIdx.x % J.CB, layer = blockIdx.y;
    const float *w = J.src + (size_t)layer * J.src_stride;
    const int i0 = cb * 32;
    const int run = min(32, J.ci - i0) * TAPS;   // valid floats of a row (CB = ceil(ci / 32): never empty)
    for (int idx = tid; idx < 16 * kRun; idx += kThreads) {
        const int r = idx / kRun, c = idx % kRun, o = ct * 16 + r;
        float v = 0.f;
        if (o < J.co && c < run) v = w[((size_t)o * J.ci + i0) * TAPS + c];
        tile[r * kRow + c] = v;
    }
    if (tid < 16) {
        const int o = ct * 16 + tid;
        double s = 1.0;   // the policy head convs: no BatchNorm, scale exactly 1
        if (J.bn && o < J.co) {
            const float *b = w + (size_t)J.co * J.ci * TAPS, *g = b + J.co, *be = g + J.co, *mu = be + J.co,
                        *var = mu + J.co;
            s = (double)g[o] / sqrt((double)var[o] + 1e-5);
            if (cb == 0) J.bias[(size_t)layer * J.co + o] = (float)(((double)b[o] - (double)mu[o]) * s + (double)be[o]);
        }
        sc[tid] = s;
    }
    __syncthreads();
    uint16_t *dst = J.dst + (size_t)layer * J.dst_stride;
    for (int it = tid; it < TAPS * 64; it += kThreads) {
        const int tap = it >> 6, l = it & 63, r = l & 15, q = l >> 4;
        const bool row_ok = ct * 16 + r < J.co;
        const double s = sc[r];
        uint32_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int il = q * 8 + j;
            float v = 0.f;   // padding is +0, never a product
            if (row_ok && i0 + il < J.ci) v = (float)((double)tile[r * kRow + il * TAPS + tap] * s);
            h[j] = f2bf_dev(v);
        }
        const uint4 out = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        *(uint4 *)(dst + ((((size_t)(tap * J.CB + cb) * J.CT + ct) * 64 + l) * 8)) = out;
    }
}

// plain copies with zero padding: dst[i] = i < n_src ? src[i] : 0 for i < n_dst
struct CopyJobs {
    static constexpr int kMax = 8;
    const float *src[kMax];
    float *dst[kMax];
    int n_src[kMax], n_dst[kMax];
    int n = 0, longest = 0;
    void add(const float *s, float *d, int ns, int nd) {
        src[n] = s, dst[n] = d, n_src[n] = ns, n_dst[n] = nd;
        longest = nd > longest ? nd : longest;
        ++n;
    }
};
__global__ __launch_bounds__(kThreads) void k_chess_pack_copy(CopyJobs C) {
    const int k = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i < C.n_dst[k]) C.dst[k][i] = i < C.n_src[k] ? C.src[k][i] : 0.f;
}

// ---------------------------------------------------------------- fp32 net
// w [co][K] -> W^T [K][co] (K = ci * taps) of `layers` layers, through a 32 x 32 LDS tile
__global__ __launch_bounds__(kThreads) void k_chess_pack_wt(const float *__restrict__ src, size_t src_stride, int co,
                                                            int K, float *__restrict__ dst, size_t dst_stride) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    src += (size_t)blockIdx.z * src_stride;
    dst += (size_t)blockIdx.z * dst_stride;
    for (int r = ty; r < 32; r += 8) {
        const int o = o0 + r, k = k0 + tx;
        t[r][tx] = (o < co && k < K) ? src[(size_t)o * K + k] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, o = o0 + tx;
        if (k < K && o < co) dst[(size_t)k * co + o] = t[tx][r];
    }
}

// BN rows [5][256] of `layers` conv3x3 + BN layers: conv bias, mean, 1 / sqrt(var + eps)
// in float32 (net_f32_pack), gamma, beta; `src` points at layer 0's conv bias
__global__ __launch_bounds__(kHid) void k_chess_pack_bn_rows(const float *__restrict__ src, size_t src_stride,
                                                             float *__restrict__ rows) {
    const int o = threadIdx.x;
    const float *b = src + (size_t)blockIdx.x * src_stride, *g = b + kHid, *be = g + kHid, *mu = be + kHid,
                *var = mu + kHid;
    float *out = rows + (size_t)blockIdx.x * 5 * kHid;
    out[0 * kHid + o] = b[o];
    out[1 * kHid + o] = mu[o];
    out[2 * kHid + o] = 1.0f / sqrtf(var[o] + 1e-5f);
    out[3 * kHid + o] = g[o];
    out[4 * kHid + o] = be[o];
}

template <int TAPS>
void conv_launch(const ConvJob &J, int layers, hipStream_t st) {
    if (layers > 0) k_chess_pack_conv<TAPS><<<dim3(J.CT * J.CB, layers), kThreads, 0, st>>>(J);
}

void copy_launch(const CopyJobs &C, hipStream_t st) {
    k_chess_pack_copy<<<dim3((C.longest + kThreads - 1) / kThreads, C.n), kThreads, 0, st>>>(C);
}

void wt_launch(const float *src, size_t src_stride, int co, int K, float *dst, size_t dst_stride, int layers,
               hipStream_t st) {
    if (layers > 0)
        k_chess_pack_wt<<<dim3((K + 31) / 32, (co + 31) / 32, layers), kThreads, 0, st>>>(src, src_stride, co, K, dst,
                                                                                         dst_stride);
}

int pack_bf16(spai_chess_net *n, const float *P, hipStream_t st) {
    const int nres = 2 * n->blocks;
    const Offsets O = offsets(n->blocks);
    constexpr size_t kLayerU16 = (size_t)9 * 8 * kCT * 64 * 8;   // a trunk conv's fragments
    // at blocks == 0 w_res / b_res are net_create's placeholders, and are left alone
    const bool res_ok = nres ? n->w_res.n == nres * kLayerU16 && n->b_res.n == (size_t)nres * kHid
                             : n->w_res.n == 8 && n->b_res.n == 4;
    SPAI_CHECK(n->w_stem.n == (size_t)9 * kCT * 64 * 8 && res_ok && n->w_p1.n == (size_t)8 * kCT * 64 * 8 &&
                   n->w_p2.n == (size_t)8 * kPolCT * 64 * 8 && n->b_stem.n == kHid && n->b_p1.n == kHid &&
                   n->b_p2.n == kPolCT * 16 && n->v_w.n == kHid && n->v_b.n == 1 && n->l1_w.n == (size_t)kHid * 64 &&
                   n->l1_b.n == kHid && n->l2_w.n == kHid && n->l2_b.n == 1,
               SPAI_ERR_INVALID, "bf16 chess net buffers do not have the sizes of a %d-block net", n->blocks);
    conv_launch<9>(ConvJob{P, 0, n->w_stem.p, 0, n->b_stem.p, kPlanes, kHid, 1, kCT, 1}, 1, st);
    conv_launch<9>(ConvJob{P + O.res0, O.res_stride, n->w_res.p, kLayerU16, n->b_res.p, kHid, kHid, 8, kCT, 1}, nres, st);
    conv_launch<1>(ConvJob{P + O.p1_w, 0, n->w_p1.p, 0, nullptr, kHid, kHid, 8, kCT, 0}, 1, st);
    conv_launch<1>(ConvJob{P + O.p2_w, 0, n->w_p2.p, 0, nullptr, kHid, kPolC, 8, kPolCT, 0}, 1, st);
    CopyJobs C;
    C.add(P + O.p1_b, n->b_p1.p, kHid, kHid);
    C.add(P + O.p2_b, n->b_p2.p, kPolC, kPolCT * 16);   // 73 biases and 7 zeros
    C.add(P + O.v_w, n->v_w.p, kHid, kHid);
    C.add(P + O.v_b, n->v_b.p, 1, 1);
    C.add(P + O.l1_w, n->l1_w.p, kHid * 64, kHid * 64);
    C.add(P + O.l1_b, n->l1_b.p, kHid, kHid);
    C.add(P + O.l2_w, n->l2_w.p, kHid, kHid);
    C.add(P + O.l2_b, n->l2_b.p, 1, 1);
    copy_launch(C, st);
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

// net_f32_pack's buffer (weights_f32 in chess_net_f32.hip): stem W^T [19*9][256] | stem BN
// [5][256] | trunk W^T x nres | trunk BN x nres | p1 W^T, b | p2 W^T [256][73], b | value
// conv w, b | linear 1 w, b | linear 2 w, b
int pack_f32(spai_chess_net *n, const float *P, hipStream_t st) {
    const int nres = 2 * n->blocks;
    const Offsets O = offsets(n->blocks);
    constexpr size_t kLw = (size_t)kHid * 9 * kHid, kBn = 5 * kHid;
    SPAI_CHECK(n->wf.n == O.end, SPAI_ERR_INVALID, "fp32 chess net buffer holds %zu floats, expected %zu", n->wf.n,
               O.end);
    float *out = n->wf.p;
    const size_t stem_w = (size_t)kPlanes * 9 * kHid;
    wt_launch(P, 0, kHid, kPlanes * 9, out, 0, 1, st);
    k_chess_pack_bn_rows<<<1, kHid, 0, st>>>(P + stem_w, 0, out + stem_w);
    out += stem_w + kBn;
    wt_launch(P + O.res0, O.res_stride, kHid, kHid * 9, out, kLw, nres, st);
    out += nres * kLw;
    if (nres) k_chess_pack_bn_rows<<<nres, kHid, 0, st>>>(P + O.res0 + kLw, O.res_stride, out);
    out += nres * kBn;
    wt_launch(P + O.p1_w, 0, kHid, kHid, out, 0, 1, st);
    float *p1_b = out + (size_t)kHid * kHid, *p2_w = p1_b + kHid, *p2_b = p2_w + (size_t)kHid * kPolC;
    wt_launch(P + O.p2_w, 0, kPolC, kHid, p2_w, 0, 1, st);
    CopyJobs C;
    C.add(P + O.p1_b, p1_b, kHid, kHid);
    const int tail = (int)(O.end - O.p2_b);   // the policy bias and everything behind it: the same order in both
    C.add(P + O.p2_b, p2_b, tail, tail);
    copy_launch(C, st);
    SPAI_CHECK((size_t)(p2_b + tail - n->wf.p) == n->wf.n, SPAI_ERR_INVALID, "internal: fp32 layout walk mismatch");
    SPAI_HIP(hipGetLastError());
    return SPAI_OK;
}

}  // namespace

// fold and pack the flat device parameters into the net's own buffers on the engine's stream;
// returns once enqueued
int net_set_params_device(spai_chess_net *net, const float *d_params, size_t n) {
    SPAI_CHECK(d_params && n == net_num_params(net->blocks), SPAI_ERR_INVALID, "expected %zu params, got %zu",
               net_num_params(net->blocks), n);
    hipStream_t st = net->eng->stream;
    return net->dtype == SPAI_DTYPE_F32 ? pack_f32(net, d_params, st) : pack_bf16(net, d_params, st);
}

// weight refresh in place from a host array: uploaded to the net's staging buffer, then the
// same kernels; stream-ordered behind whatever search still reads the old weights
int net_set_params(spai_chess_net *net, const float *params, size_t n) {
    const size_t want = net_num_params(net->blocks);
    SPAI_CHECK(params && n == want, SPAI_ERR_INVALID, "expected %zu params, got %zu", want, n);
    if (net->stage.n != want) SPAI_TRY(net->stage.alloc(want));   // once per net
    hipStream_t st = net->eng->stream;
    // behind every earlier reader of the staging buffer and of the weights
    SPAI_HIP(hipMemcpyAsync(net->stage.p, params, want * 4, hipMemcpyHostToDevice, st));
    SPAI_TRY(net_set_params_device(net, net->stage.p, want));
    SPAI_HIP(hipStreamSynchronize(st));   // `params` is the caller's again, the weights are in place
    return SPAI_OK;
}

// the packed weight buffers in a fixed order (include/spai.h), after draining the stream
int net_image(spai_chess_net *net, void *out, size_t cap, size_t *bytes) {
    struct Part {
        const void *p;
        size_t bytes;
    };
    std::vector<Part> parts;
    if (net->dtype == SPAI_DTYPE_F32) {
        parts.push_back({net->wf.p, net->wf.n * 4});
    } else {
        for (auto *d : {&net->w_stem, &net->w_res, &net->w_p1, &net->w_p2}) parts.push_back({d->p, d->n * 2});
        for (auto *d : {&net->b_stem, &net->b_res, &net->b_p1, &net->b_p2, &net->v_w, &net->v_b, &net->l1_w, &net->l1_b,
                        &net->l2_w, &net->l2_b})
            parts.push_back({d->p, d->n * 4});
    }
    size_t total = 0;
    for (const Part &p : parts) total += p.bytes;
    *bytes = total;
    if (!out) return SPAI_OK;
    SPAI_CHECK(cap >= total, SPAI_ERR_INVALID, "image needs %zu bytes, the buffer holds %zu", total, cap);
    hipStream_t st = net->eng->stream;
    size_t off = 0;
    for (const Part &p : parts) {
        SPAI_HIP(hipMemcpyAsync((char *)out + off, p.p, p.bytes, hipMemcpyDeviceToHost, st));
        off += p.bytes;
    }
    SPAI_HIP(hipStreamSynchronize(st));
    return SPAI_OK;
}

}  // namespace chess
}  // namespace spai
