// hn_unet_f64.hip -- the stateful UNet and the solver loop in float64: what the reference computes after solver.double().
//
//   d  = HybridNet(in6)                                            (architectures.py:439-465, 240-252)
//   wf = d / 1e3 + wf;  res = L(wf) + k_sq . wf - src               (single_step, hybridnet.py:558-584; the residual is f64_apply, hn_f64.hip)
//
// A reference, not a race: the reference's layers one by one (no composed out-conv, no fused levels), every launch on the caller's stream, no side
// stream, no flags, no atomics, every sum in a fixed order.  The weights are the fp32 blob of the last hn_load_weights up-cast exactly (what .double()
// does to the parameters), kept in the blob's own PyTorch layout and walked with raw_layout() / for_each_layer().
//
//   k_dc_f64<CIN_A, CIN_B, CM, CO>  one DoubleConv (conv3x3 -> activation -> conv3x3) of cat[a, b] per 16 x 16 output tile: the input tile with halo 2
//                                   and the activated mid tile with halo 1 in LDS; mid positions outside the image are ZERO (conv2 zero-pads the activated
//                                   tensor), not act(conv1(padding) + b1)
//   k_conv8_f64<TRANSPOSED>         Conv2d(8, 8, 8, stride 2, pad 3) per 16 x 16 output tile, one input channel staged at a time; ConvTranspose2d likewise
//                                   per 16 x 16 tile of 2 x 2 output quads (the four parities of a quad use disjoint taps, so the weights stay uniform)
//   k_in6_f64 / k_outc_f64 / k_update_f64   cat[wf, 1e3 res, sigmas], the 1x1 out-conv, wf = d / 1e3 + wf
//
// Weights are read through wave-uniform addresses (scalar loads), activations through LDS.  Nothing here is tuned.
#include <new>

#include "hn_internal.h"

namespace hn {

// the layers' weights as pointers into the up-cast blob (members named as for_each_layer wants them)
struct F64Dc { const double *w1, *b1, *slope, *w2, *b2; int cin, cm, co; };   // w1 [cm][cin][3][3], w2 [co][cm][3][3]
struct F64K8 { const double *w, *b; };                                         // down [out][in][8][8], up [in][out][8][8]
struct F64Unet {
    double* w = nullptr;          // [raw_layout(depth).total]
    F64Dc inc{}, sig[kMaxDepth]{}, st[kMaxDepth]{}, dec[kMaxDepth + 1]{};
    F64K8 down[kMaxDepth]{}, up[kMaxDepth]{};
    const double *outc_w = nullptr, *outc_b = nullptr;
    // workspace for `cap` samples (pieces of `block`): the assembled input and d of hn_step_f64; per level x_d (later the upsampled u_d), y_d and out_d
    // (none at the bottleneck) with 8 channels each; the second flat state buffer, hn_step_f64 ping-pongs between it and the caller's
    int cap = 0;
    DeviceBlock block;
    double *a[kMaxDepth + 1]{}, *o[kMaxDepth]{}, *y[kMaxDepth + 1]{}, *in6 = nullptr, *d = nullptr, *st_tmp = nullptr;
};

namespace {

constexpr int kT = 16;              // output tile
constexpr int kInW = kT + 4;        // input tile with halo 2
constexpr int kMidW = kT + 2;       // mid tile with halo 1
constexpr size_t kD = sizeof(double);   // (the overlap check and the workspace count bytes)

struct View { const double* p; long sb, sc; };   // element (b, c, y, x) at p[b * sb + c * sc + y * W + x]
struct OutView { double* p; long sb, sc; };

// architectures.py:5-44 with the torch modules' default arguments, in double.  The piecewise-linear kinds take the slope the reference's module holds after
// .double(): the up-cast PReLU parameter, 0, or nn.LeakyReLU's Python float 0.01 (NOT the fp32 0.01 of the blob's slope slot).
__device__ __forceinline__ double act_f64(double x, int act, double slope) {
    switch (act) {
        case HN_ACT_PRELU: return x > 0.0 ? x : slope * x;
        case HN_ACT_RELU: return x > 0.0 ? x : 0.0;
        case HN_ACT_LEAKYRELU: return x > 0.0 ? x : 0.01 * x;
        case HN_ACT_CELU: return fmax(x, 0.0) + fmin(expm1(x), 0.0);
        case HN_ACT_TANH: return tanh(x);
        case HN_ACT_GELU: return 0.5 * x * (1.0 + erf(x * 0.7071067811865476));
        case HN_ACT_TANHSHRINK: return x - tanh(x);
        case HN_ACT_SOFTPLUS: return x > 20.0 ? x : log1p(exp(x));
        default: return x;
    }
}

template <int CIN_A, int CIN_B, int CM, int CO>
constexpr size_t dc_lds_bytes() { return sizeof(double) * ((size_t)(CIN_A + CIN_B) * kInW * kInW + (size_t)CM * kMidW * kMidW); }

template <int CIN_A, int CIN_B, int CM, int CO>
__global__ __launch_bounds__(256) void k_dc_f64(View a, View b, OutView out, F64Dc w, int act, int H, int W) {
    constexpr int CIN = CIN_A + CIN_B;
    extern __shared__ double lds[];
    double* s_in = lds;                               // [CIN][kInW][kInW]: image rows y0 - 2 .., columns x0 - 2 ..
    double* s_mid = lds + CIN * kInW * kInW;          // [CM][kMidW][kMidW]: image rows y0 - 1 .., columns x0 - 1 ..
    const int tid = threadIdx.x, bz = blockIdx.z;
    const int y0 = blockIdx.y * kT, x0 = blockIdx.x * kT;
    for (int e = tid; e < CIN * kInW * kInW; e += 256) {
        const int c = e / (kInW * kInW), r = e - c * (kInW * kInW);
        const int y = y0 - 2 + r / kInW, x = x0 - 2 + r % kInW;
        double v = 0.0;
        if (y >= 0 && y < H && x >= 0 && x < W)
            v = c < CIN_A ? a.p[bz * a.sb + c * a.sc + (long)y * W + x] : b.p[bz * b.sb + (c - CIN_A) * b.sc + (long)y * W + x];
        s_in[e] = v;
    }
    __syncthreads();
    const double slope = w.slope[0];
    for (int p = tid; p < kMidW * kMidW; p += 256) {
        const int my = p / kMidW, mx = p - my * kMidW;
        const int y = y0 - 1 + my, x = x0 - 1 + mx;
        double acc[CM];
#pragma unroll
        for (int m = 0; m < CM; ++m) acc[m] = w.b1[m];
        const bool inside = y >= 0 && y < H && x >= 0 && x < W;
        if (inside) {
#pragma unroll 1
            for (int c = 0; c < CIN; ++c) {
                const double* sp = s_in + c * (kInW * kInW) + my * kInW + mx;
                const double* wp = w.w1 + c * 9;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const double v = sp[ky * kInW + kx];
#pragma unroll
                        for (int m = 0; m < CM; ++m) acc[m] = fma(wp[m * (CIN * 9) + ky * 3 + kx], v, acc[m]);
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < CM; ++m) s_mid[m * (kMidW * kMidW) + p] = inside ? act_f64(acc[m], act, slope) : 0.0;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    double acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = w.b2[o];
#pragma unroll 1
    for (int m = 0; m < CM; ++m) {
        const double* sp = s_mid + m * (kMidW * kMidW) + ty * kMidW + tx;
        const double* wp = w.w2 + m * 9;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const double v = sp[ky * kMidW + kx];
#pragma unroll
                for (int o = 0; o < CO; ++o) acc[o] = fma(wp[o * (CM * 9) + ky * 3 + kx], v, acc[o]);
            }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) out.p[bz * out.sb + o * out.sc + (long)y * W + x] = acc[o];
}

// in [B][8][Hin][Win] -> out [B][8][Hout][Wout], both dense.  TRANSPOSED false: Hout = Hin / 2, out[co][oy][ox] = b[co] + sum w[co][ci][ky][kx] in[ci][2 oy - 3 + ky][2 ox - 3 + kx].
// TRANSPOSED true: Hout = 2 Hin, out[co][oy][ox] = b[co] + sum over ky = oy + 3 (mod 2), kx likewise of w[ci][co][ky][kx] in[ci][(oy + 3 - ky) / 2][(ox + 3 - kx) / 2].
constexpr int kDownW = 2 * kT + 6;   // input rows / columns under a 16 x 16 output tile of the stride-2 convolution
constexpr int kUpW = kT + 4;         // input rows / columns under 16 x 16 output quads of the transposed one: quad q reads rows q - 2 .. q + 2
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void k_conv8_f64(const double* __restrict__ in, double* __restrict__ out, F64K8 w, int Hin, int Win) {
    __shared__ double s_in[TRANSPOSED ? kUpW * kUpW : kDownW * kDownW];   // one input channel
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long pin = (long)Hin * Win;
    const double* src = in + (long)blockIdx.z * kFeat * pin;
    if (!TRANSPOSED) {
        const int Hout = Hin >> 1, Wout = Win >> 1;
        const int oy = blockIdx.y * kT + ty, ox = blockIdx.x * kT + tx;
        const int iy0 = 2 * (int)blockIdx.y * kT - 3, ix0 = 2 * (int)blockIdx.x * kT - 3;
        double acc[kFeat];
#pragma unroll
        for (int o = 0; o < kFeat; ++o) acc[o] = w.b[o];
#pragma unroll 1
        for (int c = 0; c < kFeat; ++c) {
            __syncthreads();
            for (int e = tid; e < kDownW * kDownW; e += 256) {
                const int y = iy0 + e / kDownW, x = ix0 + e % kDownW;
                s_in[e] = (y >= 0 && y < Hin && x >= 0 && x < Win) ? src[c * pin + (long)y * Win + x] : 0.0;
            }
            __syncthreads();
#pragma unroll 1
            for (int ky = 0; ky < 8; ++ky) {
                const double* sp = s_in + (2 * ty + ky) * kDownW + 2 * tx;
                const double* wp = w.w + (c * 8 + ky) * 8;
#pragma unroll
                for (int kx = 0; kx < 8; ++kx) {
                    const double v = sp[kx];
#pragma unroll
                    for (int o = 0; o < kFeat; ++o) acc[o] = fma(wp[o * (kFeat * 64) + kx], v, acc[o]);
                }
            }
        }
        if (oy < Hout && ox < Wout) {
            double* dst = out + (long)blockIdx.z * kFeat * Hout * Wout + (long)oy * Wout + ox;
#pragma unroll
            for (int o = 0; o < kFeat; ++o) dst[(long)o * Hout * Wout] = acc[o];
        }
    } else {
        const int Hout = 2 * Hin, Wout = 2 * Win;
        const int qy = blockIdx.y * kT + ty, qx = blockIdx.x * kT + tx;   // the thread's quad: outputs (2 qy + py, 2 qx + px)
        const int iy0 = (int)blockIdx.y * kT - 2, ix0 = (int)blockIdx.x * kT - 2;
        double acc[2][2][kFeat];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px)
#pragma unroll
                for (int o = 0; o < kFeat; ++o) acc[py][px][o] = w.b[o];
#pragma unroll 1
        for (int c = 0; c < kFeat; ++c) {
            __syncthreads();
            for (int e = tid; e < kUpW * kUpW; e += 256) {
                const int y = iy0 + e / kUpW, x = ix0 + e % kUpW;
                s_in[e] = (y >= 0 && y < Hin && x >= 0 && x < Win) ? src[c * pin + (long)y * Win + x] : 0.0;
            }
            __syncthreads();
            // parity py takes ky = 1 - py + 2 j, j = 0 .. 3, from input row qy + 1 + py - j (row ty + 3 + py - j of the tile)
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const int ky = 1 - py + 2 * j;
                    const double* sp = s_in + (ty + 3 + py - j) * kUpW + tx;
                    const double* wp = w.w + (long)c * (kFeat * 64) + ky * 8;
#pragma unroll
                    for (int px = 0; px < 2; ++px)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const double v = sp[3 + px - i];
#pragma unroll
                            for (int o = 0; o < kFeat; ++o) acc[py][px][o] = fma(wp[o * 64 + 1 - px + 2 * i], v, acc[py][px][o]);
                        }
                }
        }
        if (qy < Hin && qx < Win) {
            double* dst = out + (long)blockIdx.z * kFeat * Hout * Wout;
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int o = 0; o < kFeat; ++o) dst[(long)o * Hout * Wout + (long)(2 * qy + py) * Wout + 2 * qx + px] = acc[py][px][o];
        }
    }
}

// in6[b] = cat[wf[b], 1e3 * res[b], sigmas] (hybridnet.py:564-566; the sigma maps are the fp32 table values up-cast)
__global__ __launch_bounds__(256) void k_in6_f64(const double* __restrict__ wf, const double* __restrict__ res, const float* __restrict__ sig,
                                                 double* __restrict__ in6, long plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * plane) return;
    const long b = blockIdx.y;
    double* o = in6 + b * kInCh * plane;
    o[i] = wf[b * 2 * plane + i];
    o[2 * plane + i] = 1e3 * res[b * 2 * plane + i];
    o[4 * plane + i] = (double)sig[i];
}
// the 1x1 out-conv: d[b][c] = bo[c] + sum_k wo[c][k] y[b][k]
__global__ __launch_bounds__(256) void k_outc_f64(const double* __restrict__ y, const double* __restrict__ wo, const double* __restrict__ bo,
                                                  double* __restrict__ d, long plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    const long b = blockIdx.y;
    const double* p = y + b * kFeat * plane + i;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        double acc = bo[c];
#pragma unroll
        for (int k = 0; k < kFeat; ++k) acc = fma(wo[c * kFeat + k], p[k * plane], acc);
        d[(b * 2 + c) * plane + i] = acc;
    }
}
// wf = d / 1e3 + wf: divide, then add, as the reference writes it
__global__ __launch_bounds__(256) void k_update_f64(double* __restrict__ wf, const double* __restrict__ d, long count) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) wf[i] = d[i] / 1e3 + wf[i];
}

template <int CIN_A, int CIN_B, int CM, int CO>
int dc_attr(hn_ctx* ctx) {
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_dc_f64<CIN_A, CIN_B, CM, CO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dc_lds_bytes<CIN_A, CIN_B, CM, CO>()));
    return HN_OK;
}
template <int CIN_A, int CIN_B, int CM, int CO>
void dc_launch(View a, View b, OutView out, const F64Dc& w, int act, int H, int W, int batch, hipStream_t s) {
    const dim3 grid((W + kT - 1) / kT, (H + kT - 1) / kT, batch);
    constexpr size_t lds = dc_lds_bytes<CIN_A, CIN_B, CM, CO>();
    hipLaunchKernelGGL((k_dc_f64<CIN_A, CIN_B, CM, CO>), grid, dim3(256), lds, s, a, b, out, w, act, H, W);
}
// one DoubleConv of cat[a, b] (b.p == nullptr: of a alone), by the channel shapes of for_each_layer
int launch_dc(hn_ctx* ctx, View a, View b, OutView out, const F64Dc& w, int H, int W, int batch, hipStream_t s) {
    const int act = ctx->act_kind;
    if (w.cin == kInCh && w.co == kFeat) dc_launch<kInCh, 0, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat + kState && w.co == kFeat) dc_launch<kFeat, kState, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat + kState && w.co == kState) dc_launch<kFeat, kState, kState, kState>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == 2 * kFeat && w.co == kFeat) dc_launch<kFeat, kFeat, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat && w.co == kFeat) dc_launch<kFeat, 0, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else return fail(ctx, HN_ERR_UNSUPPORTED, "float64 DoubleConv %d -> %d -> %d is not one of the UNet's", w.cin, w.cm, w.co);
    return HN_OK;
}

int build(hn_ctx* ctx, int batch) {
    const int depth = ctx->depth, n = ctx->tab.n;
    if (ctx->f64 == nullptr) {
        const RawLayout L = raw_layout(depth);
        if (ctx->raw_blob.size() != L.total) return fail(ctx, HN_ERR_STATE, "internal: no weight blob of depth %d is held", depth);
        F64Unet* u = new (std::nothrow) F64Unet();
        if (!u) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
        ctx->f64 = u;   // (from here on unet_f64_free releases whatever exists)
        std::vector<double> h(ctx->raw_blob.begin(), ctx->raw_blob.end());
        HN_HIP(ctx, hipMalloc((void**)&u->w, L.total * sizeof(double)));
        HN_HIP(ctx, hipMemcpy(u->w, h.data(), L.total * sizeof(double), hipMemcpyHostToDevice));
        const double* w = u->w;
        for_each_layer(depth,
            [&](int, int, int, const RawDc& r, F64Dc& l) { l = F64Dc{w + r.w1, w + r.b1, w + r.slope, w + r.w2, w + r.b2, r.cin, r.cm, r.co}; },
            [&](bool, const RawK8& r, F64K8& l) { l = F64K8{w + r.w, w + r.b}; }, L, *u);
        u->outc_w = w + L.outc_w;
        u->outc_b = w + L.outc_b;
        int rc = dc_attr<kInCh, 0, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kState, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kState, kState, kState>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kFeat, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, 0, kFeat, kFeat>(ctx);
        if (rc != HN_OK) return rc;
    }
    F64Unet* u = ctx->f64;
    if (batch > u->cap) {
        u->cap = 0;
        const size_t per = kD * batch;   // bytes per double of a sample
        std::vector<size_t> sizes{per * kInCh * n * n, per * 2 * n * n};
        for (int d = 0; d <= depth; ++d) sizes.insert(sizes.end(), d < depth ? 3 : 2, per * kFeat * (n >> d) * (n >> d));
        sizes.push_back(per * kState * ctx->state_len);
        if (const int rc = u->block.alloc(ctx, "float64 UNet", sizes.data(), (int)sizes.size()); rc != HN_OK) return rc;
        auto take = [&]() { return static_cast<double*>(u->block.take()); };
        u->in6 = take();
        u->d = take();
        for (int d = 0; d <= depth; ++d) {
            u->a[d] = take();
            u->y[d] = take();
            if (d < depth) u->o[d] = take();
        }
        u->st_tmp = take();
        u->cap = batch;
    }
    return HN_OK;
}
// weights, workspace and state buffer for `batch` samples: built by the first call, grown by a larger batch -- never under stream capture
int prepare(hn_ctx* ctx, int batch, hipStream_t s) {
    if (ctx->f64 != nullptr && batch <= ctx->f64->cap) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "the float64 weights and workspace (or a larger batch's) are built by the first call, which must not be under stream capture");
    const int rc = build(ctx, batch);
    if (rc != HN_OK) unet_f64_free(ctx);   // nothing half-built stays behind
    return rc;
}

// one HybridNet forward, layer by layer
int forward(hn_ctx* ctx, const double* in6, const double* st_in, double* st_out, double* d_out, int batch, hipStream_t s) {
    const F64Unet& u = *ctx->f64;
    const int n = ctx->tab.n, depth = ctx->depth;
    const long L = ctx->state_len;
    const View none{nullptr, 0, 0};
    auto dense = [](const double* p, int m) { return View{p, (long)kFeat * m * m, (long)m * m}; };
    auto dense_out = [](double* p, int m) { return OutView{p, (long)kFeat * m * m, (long)m * m}; };
    int rc = launch_dc(ctx, View{in6, (long)kInCh * n * n, (long)n * n}, none, dense_out(u.a[0], n), u.inc, n, n, batch, s);
    for (int d = 0; d < depth && rc == HN_OK; ++d) {
        const int m = n >> d;
        const View state{st_in + ctx->state_off[d], kState * L, L};
        rc = launch_dc(ctx, dense(u.a[d], m), state, dense_out(u.o[d], m), u.sig[d], m, m, batch, s);
        if (rc == HN_OK) rc = launch_dc(ctx, dense(u.o[d], m), state, OutView{st_out + ctx->state_off[d], kState * L, L}, u.st[d], m, m, batch, s);
        const int mo = m >> 1;
        hipLaunchKernelGGL(k_conv8_f64<false>, dim3((mo + kT - 1) / kT, (mo + kT - 1) / kT, batch), dim3(256), 0, s, u.o[d], u.a[d + 1], u.down[d], m, m);
    }
    if (rc == HN_OK) rc = launch_dc(ctx, dense(u.a[depth], n >> depth), none, dense_out(u.y[depth], n >> depth), u.dec[depth], n >> depth, n >> depth, batch, s);
    for (int d = depth - 1; d >= 0 && rc == HN_OK; --d) {
        const int m = n >> d, mi = m >> 1;
        hipLaunchKernelGGL(k_conv8_f64<true>, dim3((mi + kT - 1) / kT, (mi + kT - 1) / kT, batch), dim3(256), 0, s, u.y[d + 1], u.a[d], u.up[d], mi, mi);
        rc = launch_dc(ctx, dense(u.a[d], m), dense(u.o[d], m), dense_out(u.y[d], m), u.dec[d], m, m, batch, s);
    }
    if (rc != HN_OK) return rc;
    const long plane = (long)n * n;
    hipLaunchKernelGGL(k_outc_f64, dim3((unsigned)((plane + 255) / 256), batch), dim3(256), 0, s, u.y[0], u.outc_w, u.outc_b, d_out, plane);
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

int check_f64_ready(hn_ctx* ctx, int batch) {
    if (ctx->rect) return rect_unsupported(ctx, "hn_unet_f64 / hn_step_f64");
    if (!ctx->have_weights) return fail(ctx, HN_ERR_STATE, "hn_load_weights has not been called");
    if (ctx->tab.n == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    if (batch <= 0) return fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    if (ctx->tab.n % (1 << ctx->depth) != 0)
        return fail(ctx, HN_ERR_ARG, "domain size %d is not divisible by 2^depth = %d", ctx->tab.n, 1 << ctx->depth);
    return HN_OK;
}

}  // namespace

void unet_f64_free(hn_ctx* ctx) {
    F64Unet* u = ctx->f64;
    if (u == nullptr) return;
    (void)hipFree(u->w);
    u->block.free();
    delete u;
    ctx->f64 = nullptr;
}

}  // namespace hn

using namespace hn;

extern "C" {

int hn_unet_f64(hn_ctx* ctx, const double* in6, const double* states_in, double* states_out, double* d_out, int batch, void* stream) {
    if (!ctx || !in6 || !states_in || !states_out || !d_out) return fail(ctx, HN_ERR_ARG, "hn_unet_f64: NULL argument");
    int rc = check_f64_ready(ctx, batch);
    if (rc != HN_OK) return rc;
    const size_t plane = kD * ctx->tab.n * ctx->tab.n, sl = kD * batch * kState * ctx->state_len;   // bytes
    const MemRange r[] = {{in6, batch * kInCh * plane, false, "in6"}, {states_in, sl, false, "states_in"}, {states_out, sl, true, "states_out"},
                          {d_out, batch * 2 * plane, true, "d_out"}};
    const char *who, *other;
    if (first_overlap(r, 4, &who, &other)) return fail(ctx, HN_ERR_ARG, "hn_unet_f64: %s overlaps %s", who, other);
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = prepare(ctx, batch, s)) != HN_OK) return rc;
    return forward(ctx, in6, states_in, states_out, d_out, batch, s);
}

int hn_step_f64(hn_ctx* ctx, double* wf, double* res, double* states, const double* k_sq, const double* src, int src_batch, int batch, int n_iter,
                double* res_hist, double* wf_hist, double* st_hist, double* rmse_hist, void* stream) {
    if (!ctx || !wf || !res || !states || !k_sq || !src) return fail(ctx, HN_ERR_ARG, "hn_step_f64: NULL argument");
    if (n_iter < 0) return fail(ctx, HN_ERR_ARG, "n_iter must be >= 0");
    int rc = check_f64_ready(ctx, batch);
    if (rc != HN_OK) return rc;
    if (src_batch != 1 && src_batch != batch) return fail(ctx, HN_ERR_ARG, "source batch %d must be 1 or equal to the batch %d", src_batch, batch);
    const int n = ctx->tab.n;
    const size_t plane = (size_t)n * n, L = (size_t)ctx->state_len;
    const size_t fc = (size_t)batch * 2 * plane, sc = (size_t)batch * kState * L;
    const MemRange r[] = {{wf, kD * fc, true, "wf"}, {res, kD * fc, true, "res"}, {states, kD * sc, true, "states"}, {k_sq, kD * batch * plane, false, "k_sq"},
                          {src, kD * src_batch * 2 * plane, false, "src"}, {res_hist, kD * n_iter * fc, true, "res_hist"},
                          {wf_hist, kD * n_iter * fc, true, "wf_hist"}, {st_hist, kD * n_iter * sc, true, "st_hist"},
                          {rmse_hist, kD * n_iter * batch, true, "rmse_hist"}};
    const char *who, *other;
    if (first_overlap(r, 9, &who, &other)) return fail(ctx, HN_ERR_ARG, "hn_step_f64: %s overlaps %s", who, other);
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = prepare(ctx, batch, s)) != HN_OK) return rc;
    if (n_iter == 0) return HN_OK;
    // f64_apply builds the domain's float64 tables and grows its partial sums at its first call and refuses that under capture -- by then this call
    // would have enqueued a UNet: build (or be refused) here, before anything is enqueued
    if ((rc = f64_reserve(ctx, batch, rmse_hist != nullptr, s)) != HN_OK) return rc;
    F64Unet& u = *ctx->f64;
    for (int it = 0; it < n_iter; ++it) {
        const double* st_in = (it & 1) ? u.st_tmp : states;   // the hidden states ping-pong between the caller's buffer and the library's
        double* st_out = (it & 1) ? states : u.st_tmp;
        hipLaunchKernelGGL(k_in6_f64, dim3((unsigned)((2 * plane + 255) / 256), batch), dim3(256), 0, s, wf, res, ctx->tab.sigmas, u.in6, (long)plane);
        if ((rc = forward(ctx, u.in6, st_in, st_out, u.d, batch, s)) != HN_OK) return rc;
        hipLaunchKernelGGL(k_update_f64, dim3((unsigned)((fc + 255) / 256)), dim3(256), 0, s, wf, u.d, (long)fc);
        if ((rc = f64_apply(ctx, wf, res, k_sq, src, src_batch, rmse_hist ? rmse_hist + (size_t)it * batch : nullptr, batch, s)) != HN_OK) return rc;
        if (res_hist) HN_HIP(ctx, hipMemcpyAsync(res_hist + it * fc, res, fc * sizeof(double), hipMemcpyDeviceToDevice, s));
        if (wf_hist) HN_HIP(ctx, hipMemcpyAsync(wf_hist + it * fc, wf, fc * sizeof(double), hipMemcpyDeviceToDevice, s));
        if (st_hist) HN_HIP(ctx, hipMemcpyAsync(st_hist + it * sc, st_out, sc * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (n_iter & 1) HN_HIP(ctx, hipMemcpyAsync(states, u.st_tmp, sc * sizeof(double), hipMemcpyDeviceToDevice, s));
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

}  // extern "C"
