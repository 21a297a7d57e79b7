// hn_jvp.hip -- forward mode of the solver loop: the tangents of n_iter iterations of hn_step, linearised at the trajectory hn_step wrote.
//
//   d  = HybridNet(in6),  wf = d / 1e3 + wf,  res = L(wf) + k_sq . wf - src          (single_step, hybridnet.py:558-584)
//   d' = J_net(in6, st) [in6', st'],  wf' = d' / 1e3 + wf',  res' = L(wf') + k_sq . wf' - (src' - k_sq' . wf)
//
// Modelled on hn_unet_f64.hip: the reference's layers one by one, every launch on the caller's stream, no side stream, no flags, no atomics, every sum in
// a fixed order, the weights of the last hn_load_weights in the blob's own PyTorch layout (walked with raw_layout() / for_each_layer()).  Arithmetic is fp32
// on PACKED DUALS: an activation is a float2 (primal, tangent) in the workspace and in LDS, an accumulator an f32x2, and a weight multiplies both halves, so
// a tap is one packed FMA.  Biases enter the primal half only; between the convolutions the primal half gets act(z) and the tangent half act'(z) . z'.
// The primal half is recomputed from the tape slot in front of each iteration and discarded: only tangents leave an iteration.
//
//   k_dc_dual<CIN_A, CIN_B, CM, CO>   one DoubleConv of cat[a, b] per 16 x 16 output tile: input tile (halo 2) and mid tile (halo 1) as duals in LDS;
//                                     mid positions outside the image are zero in both halves (as k_dc_f64)
//   k_conv8_dual<TRANSPOSED>          the 8 x 8 stride-2 convolution and its transpose, one input channel staged at a time (as k_conv8_f64)
//   k_in6_dual                        primal [wf, 1e3 res, sigma] beside tangent [wf', 1e3 res', 0, 0]
//   k_outc_dual / k_update_tan        the 1x1 out-conv's tangent d', wf' <- div1000(d') + wf' (hn_step's correctly rounded division)
//   k_jvp_src                         s~[b] = src'[b or 0] - k_sq'[b] . wf_t[b]: the tangent residual is then the EXISTING residual launch (spec_apply) on
//                                     (wf', k_sq, s~), whatever spectral route the domain has; without k_sq' and src' its source is a page of zeros
//
// Tensors of the caller are read and written with scalar (4-byte) accesses: any 4-byte-aligned pointer is accepted.  Nothing here is tuned.
#include <new>

#include "hn_internal.h"
#include "hn_vec.h"

namespace hn {

using vec::f32x2;

// the layers' weights as pointers into the device copy of the blob (members named as for_each_layer wants them)
struct JvpDc { const float *w1, *b1, *slope, *w2, *b2; int cin, cm, co; };   // w1 [cm][cin][3][3], w2 [co][cm][3][3]
struct JvpK8 { const float *w, *b; };                                          // down [out][in][8][8], up [in][out][8][8]
struct JvpWs {
    float* w = nullptr;           // [raw_layout(depth).total]
    JvpDc inc{}, sig[kMaxDepth]{}, st[kMaxDepth]{}, dec[kMaxDepth + 1]{};
    JvpK8 down[kMaxDepth]{}, up[kMaxDepth]{};
    const float *outc_w = nullptr, *outc_b = nullptr;
    // workspace for `cap` samples (pieces of `block`): the dual input, per level x_d (later the upsampled u_d), y_d and out_d (none at the bottleneck)
    // with 8 dual channels each, d', the second tangent-state buffer, s~, and one sample's page of zeros
    int cap = 0;
    DeviceBlock block;
    float2 *a[kMaxDepth + 1]{}, *o[kMaxDepth]{}, *y[kMaxDepth + 1]{}, *in6 = nullptr;
    float *td = nullptr, *st_tmp = nullptr, *stilde = nullptr, *zero = nullptr;
};

namespace {

constexpr int kT = 16;              // output tile
constexpr int kInW = kT + 4;        // input tile with halo 2
constexpr int kMidW = kT + 2;       // mid tile with halo 1

// element (b, c, y, x) at [b * sb + c * sc + y * W + x]: of the packed tensor d, or (d == nullptr) of two planar tensors, primal p and tangent t
struct DualIn { const float2* d; const float* p; const float* t; long sb, sc; };
// the packed tensor d, or (d == nullptr) the tangent half alone to the planar tensor t (the primal half is discarded)
struct DualOut { float2* d; float* t; long sb, sc; };

// wave-uniform weight reads through the constant address space: scalar loads (hn_vec.h)
typedef const float __attribute__((address_space(4))) * CfPtr;
__device__ __forceinline__ CfPtr cf(const float* p) { return (CfPtr)(uintptr_t)p; }

__device__ __forceinline__ f32x2 load_dual(const DualIn& v, long off) {
    if (v.d != nullptr) { const float2 q = v.d[off]; return (f32x2){q.x, q.y}; }
    return (f32x2){v.p[off], v.t[off]};
}
__device__ __forceinline__ f32x2 pk_fma(float w, f32x2 v, f32x2 acc) { return __builtin_elementwise_fma((f32x2){w, w}, v, acc); }

// (act(z), act'(z) . z').  The piecewise-linear kinds: derivative 1 for z > 0 and the slope otherwise (what torch differentiates at z == 0).
__device__ __forceinline__ f32x2 act_dual(f32x2 z, int act, float slope) {
    if (act <= HN_ACT_LEAKYRELU) {
        const bool pos = z.x > 0.f;
        return (f32x2){pos ? z.x : slope * z.x, pos ? z.y : slope * z.y};
    }
    return (f32x2){act_general(z.x, act), act_grad<true>(z.x, act, slope) * z.y};
}

template <int CIN_A, int CIN_B, int CM, int CO>
constexpr size_t dc_lds_bytes() { return sizeof(float2) * ((size_t)(CIN_A + CIN_B) * kInW * kInW + (size_t)CM * kMidW * kMidW); }

template <int CIN_A, int CIN_B, int CM, int CO>
__global__ __launch_bounds__(256) void k_dc_dual(DualIn a, DualIn b, DualOut out, JvpDc w, int act, int H, int W) {
    constexpr int CIN = CIN_A + CIN_B;
    extern __shared__ float2 lds_dual[];
    f32x2* s_in = reinterpret_cast<f32x2*>(lds_dual);   // [CIN][kInW][kInW]: image rows y0 - 2 .., columns x0 - 2 ..
    f32x2* s_mid = s_in + CIN * kInW * kInW;            // [CM][kMidW][kMidW]: image rows y0 - 1 .., columns x0 - 1 ..
    const int tid = threadIdx.x, bz = blockIdx.z;
    const int y0 = blockIdx.y * kT, x0 = blockIdx.x * kT;
    for (int e = tid; e < CIN * kInW * kInW; e += 256) {
        const int c = e / (kInW * kInW), r = e - c * (kInW * kInW);
        const int y = y0 - 2 + r / kInW, x = x0 - 2 + r % kInW;
        f32x2 v = {0.f, 0.f};
        if (y >= 0 && y < H && x >= 0 && x < W)
            v = c < CIN_A ? load_dual(a, bz * a.sb + c * a.sc + (long)y * W + x) : load_dual(b, bz * b.sb + (c - CIN_A) * b.sc + (long)y * W + x);
        s_in[e] = v;
    }
    __syncthreads();
    const float slope = w.slope[0];
    const CfPtr w1 = cf(w.w1), b1 = cf(w.b1), w2 = cf(w.w2), b2 = cf(w.b2);
    for (int p = tid; p < kMidW * kMidW; p += 256) {
        const int my = p / kMidW, mx = p - my * kMidW;
        const int y = y0 - 1 + my, x = x0 - 1 + mx;
        f32x2 acc[CM];
#pragma unroll
        for (int m = 0; m < CM; ++m) acc[m] = (f32x2){b1[m], 0.f};   // the bias enters the primal half only
        const bool inside = y >= 0 && y < H && x >= 0 && x < W;
        if (inside) {
#pragma unroll 1
            for (int c = 0; c < CIN; ++c) {
                const f32x2* sp = s_in + c * (kInW * kInW) + my * kInW + mx;
                const CfPtr wp = w1 + c * 9;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const f32x2 v = sp[ky * kInW + kx];
#pragma unroll
                        for (int m = 0; m < CM; ++m) acc[m] = pk_fma(wp[m * (CIN * 9) + ky * 3 + kx], v, acc[m]);
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < CM; ++m) s_mid[m * (kMidW * kMidW) + p] = inside ? act_dual(acc[m], act, slope) : (f32x2){0.f, 0.f};
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    f32x2 acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = (f32x2){b2[o], 0.f};
#pragma unroll 1
    for (int m = 0; m < CM; ++m) {
        const f32x2* sp = s_mid + m * (kMidW * kMidW) + ty * kMidW + tx;
        const CfPtr wp = w2 + m * 9;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x2 v = sp[ky * kMidW + kx];
#pragma unroll
                for (int o = 0; o < CO; ++o) acc[o] = pk_fma(wp[o * (CM * 9) + ky * 3 + kx], v, acc[o]);
            }
    }
    if (out.d != nullptr) {
#pragma unroll
        for (int o = 0; o < CO; ++o) out.d[bz * out.sb + o * out.sc + (long)y * W + x] = make_float2(acc[o].x, acc[o].y);
    } else {
#pragma unroll
        for (int o = 0; o < CO; ++o) out.t[bz * out.sb + o * out.sc + (long)y * W + x] = acc[o].y;
    }
}

// in [B][8][Hin][Win] -> out [B][8][Hout][Wout], dense duals; index arithmetic as k_conv8_f64 (hn_unet_f64.hip)
constexpr int kDownW = 2 * kT + 6;   // input rows / columns under a 16 x 16 output tile of the stride-2 convolution
constexpr int kUpW = kT + 4;         // input rows / columns under 16 x 16 output quads of the transposed one: quad q reads rows q - 2 .. q + 2
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void k_conv8_dual(const float2* __restrict__ in, float2* __restrict__ out, JvpK8 w, int Hin, int Win) {
    __shared__ float2 s_raw[TRANSPOSED ? kUpW * kUpW : kDownW * kDownW];   // one input channel
    f32x2* s_in = reinterpret_cast<f32x2*>(s_raw);
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long pin = (long)Hin * Win;
    const float2* src = in + (long)blockIdx.z * kFeat * pin;
    const CfPtr ww = cf(w.w), wb = cf(w.b);
    if (!TRANSPOSED) {
        const int Hout = Hin >> 1, Wout = Win >> 1;
        const int oy = blockIdx.y * kT + ty, ox = blockIdx.x * kT + tx;
        const int iy0 = 2 * (int)blockIdx.y * kT - 3, ix0 = 2 * (int)blockIdx.x * kT - 3;
        f32x2 acc[kFeat];
#pragma unroll
        for (int o = 0; o < kFeat; ++o) acc[o] = (f32x2){wb[o], 0.f};
#pragma unroll 1
        for (int c = 0; c < kFeat; ++c) {
            __syncthreads();
            for (int e = tid; e < kDownW * kDownW; e += 256) {
                const int y = iy0 + e / kDownW, x = ix0 + e % kDownW;
                f32x2 v = {0.f, 0.f};
                if (y >= 0 && y < Hin && x >= 0 && x < Win) { const float2 q = src[c * pin + (long)y * Win + x]; v = (f32x2){q.x, q.y}; }
                s_in[e] = v;
            }
            __syncthreads();
#pragma unroll 1
            for (int ky = 0; ky < 8; ++ky) {
                const f32x2* sp = s_in + (2 * ty + ky) * kDownW + 2 * tx;
                const CfPtr wp = ww + (c * 8 + ky) * 8;
#pragma unroll
                for (int kx = 0; kx < 8; ++kx) {
                    const f32x2 v = sp[kx];
#pragma unroll
                    for (int o = 0; o < kFeat; ++o) acc[o] = pk_fma(wp[o * (kFeat * 64) + kx], v, acc[o]);
                }
            }
        }
        if (oy < Hout && ox < Wout) {
            float2* dst = out + (long)blockIdx.z * kFeat * Hout * Wout + (long)oy * Wout + ox;
#pragma unroll
            for (int o = 0; o < kFeat; ++o) dst[(long)o * Hout * Wout] = make_float2(acc[o].x, acc[o].y);
        }
    } else {
        const int Hout = 2 * Hin, Wout = 2 * Win;
        const int qy = blockIdx.y * kT + ty, qx = blockIdx.x * kT + tx;   // the thread's quad: outputs (2 qy + py, 2 qx + px)
        const int iy0 = (int)blockIdx.y * kT - 2, ix0 = (int)blockIdx.x * kT - 2;
        f32x2 acc[2][2][kFeat];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px)
#pragma unroll
                for (int o = 0; o < kFeat; ++o) acc[py][px][o] = (f32x2){wb[o], 0.f};
#pragma unroll 1
        for (int c = 0; c < kFeat; ++c) {
            __syncthreads();
            for (int e = tid; e < kUpW * kUpW; e += 256) {
                const int y = iy0 + e / kUpW, x = ix0 + e % kUpW;
                f32x2 v = {0.f, 0.f};
                if (y >= 0 && y < Hin && x >= 0 && x < Win) { const float2 q = src[c * pin + (long)y * Win + x]; v = (f32x2){q.x, q.y}; }
                s_in[e] = v;
            }
            __syncthreads();
            // parity py takes ky = 1 - py + 2 j, j = 0 .. 3, from input row qy + 1 + py - j (row ty + 3 + py - j of the tile)
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const int ky = 1 - py + 2 * j;
                    const f32x2* sp = s_in + (ty + 3 + py - j) * kUpW + tx;
                    const CfPtr wp = ww + (long)c * (kFeat * 64) + ky * 8;
#pragma unroll
                    for (int px = 0; px < 2; ++px)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const f32x2 v = sp[3 + px - i];
#pragma unroll
                            for (int o = 0; o < kFeat; ++o) acc[py][px][o] = pk_fma(wp[o * 64 + 1 - px + 2 * i], v, acc[py][px][o]);
                        }
                }
        }
        if (qy < Hin && qx < Win) {
            float2* dst = out + (long)blockIdx.z * kFeat * Hout * Wout;
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int o = 0; o < kFeat; ++o)
                        dst[(long)o * Hout * Wout + (long)(2 * qy + py) * Wout + 2 * qx + px] = make_float2(acc[py][px][o].x, acc[py][px][o].y);
        }
    }
}

// in6[b] = (cat[wf[b], 1e3 res[b], sigmas], cat[wf'[b], 1e3 res'[b], 0, 0])   (hybridnet.py:564-566)
__global__ __launch_bounds__(256) void k_in6_dual(const float* __restrict__ wf, const float* __restrict__ res, const float* __restrict__ t_wf,
                                                  const float* __restrict__ t_res, const float* __restrict__ sig, float2* __restrict__ in6, long plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * plane) return;
    const long b = blockIdx.y, f = b * 2 * plane + i;
    float2* o = in6 + b * kInCh * plane;
    o[i] = make_float2(wf[f], t_wf[f]);
    o[2 * plane + i] = make_float2(1e3f * res[f], 1e3f * t_res[f]);
    o[4 * plane + i] = make_float2(sig[i], 0.f);
}
// the tangent of the 1x1 out-conv: d'[b][c] = sum_k wo[c][k] y'[b][k] (the bias rides in the discarded primal half)
__global__ __launch_bounds__(256) void k_outc_dual(const float2* __restrict__ y, const float* wo, const float* bo, float* __restrict__ td, long plane) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= plane) return;
    const long b = blockIdx.y;
    const float2* p = y + b * kFeat * plane + i;
    const CfPtr cw = cf(wo), cb = cf(bo);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        f32x2 acc = {cb[c], 0.f};
#pragma unroll
        for (int k = 0; k < kFeat; ++k) { const float2 q = p[k * plane]; acc = pk_fma(cw[c * kFeat + k], (f32x2){q.x, q.y}, acc); }
        td[(b * 2 + c) * plane + i] = acc.y;
    }
}
// wf' = d' / 1e3 + wf': divide (correctly rounded, as hn_step), then add, as the reference writes it
__global__ __launch_bounds__(256) void k_update_tan(float* __restrict__ t_wf, const float* __restrict__ td, long count) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) t_wf[i] = vec::div1000(td[i]) + t_wf[i];
}
// s~[b] = src'[b or 0] - k_sq'[b] . wf_t[b], both channels: one rounded product, one rounded difference (no contraction: a caller composes the same bits)
__global__ __launch_bounds__(256) void k_jvp_src(const float* __restrict__ t_src, long src_sb, const float* __restrict__ t_k_sq, const float* __restrict__ wf_t,
                                                 float* __restrict__ stilde, long plane) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * plane) return;
    const long b = blockIdx.y;
    const long pix = i < plane ? i : i - plane;
    const float s = t_src != nullptr ? t_src[b * src_sb + i] : 0.f;
    const float k = t_k_sq != nullptr ? t_k_sq[b * plane + pix] : 0.f;
    const float kw = k * wf_t[b * 2 * plane + i];
    stilde[b * 2 * plane + i] = s - kw;
}

template <int CIN_A, int CIN_B, int CM, int CO>
int dc_attr(hn_ctx* ctx) {
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_dc_dual<CIN_A, CIN_B, CM, CO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dc_lds_bytes<CIN_A, CIN_B, CM, CO>()));
    return HN_OK;
}
template <int CIN_A, int CIN_B, int CM, int CO>
void dc_launch(DualIn a, DualIn b, DualOut out, const JvpDc& w, int act, int H, int W, int batch, hipStream_t s) {
    const dim3 grid((W + kT - 1) / kT, (H + kT - 1) / kT, batch);
    constexpr size_t lds = dc_lds_bytes<CIN_A, CIN_B, CM, CO>();
    hipLaunchKernelGGL((k_dc_dual<CIN_A, CIN_B, CM, CO>), grid, dim3(256), lds, s, a, b, out, w, act, H, W);
}
// one DoubleConv of cat[a, b] (6- and 8-channel inputs: of a alone), by the channel shapes of for_each_layer
int launch_dc(hn_ctx* ctx, DualIn a, DualIn b, DualOut out, const JvpDc& w, int H, int W, int batch, hipStream_t s) {
    const int act = ctx->act_kind;
    if (w.cin == kInCh && w.co == kFeat) dc_launch<kInCh, 0, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat + kState && w.co == kFeat) dc_launch<kFeat, kState, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat + kState && w.co == kState) dc_launch<kFeat, kState, kState, kState>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == 2 * kFeat && w.co == kFeat) dc_launch<kFeat, kFeat, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else if (w.cin == kFeat && w.co == kFeat) dc_launch<kFeat, 0, kFeat, kFeat>(a, b, out, w, act, H, W, batch, s);
    else return fail(ctx, HN_ERR_UNSUPPORTED, "dual DoubleConv %d -> %d -> %d is not one of the UNet's", w.cin, w.cm, w.co);
    return HN_OK;
}

int build(hn_ctx* ctx, int batch) {
    const int depth = ctx->depth, n = ctx->tab.n;
    if (ctx->jvp == nullptr) {
        const RawLayout L = raw_layout(depth);
        if (ctx->raw_blob.size() != L.total) return fail(ctx, HN_ERR_STATE, "internal: no weight blob of depth %d is held", depth);
        JvpWs* u = new (std::nothrow) JvpWs();
        if (!u) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
        ctx->jvp = u;   // (from here on jvp_free releases whatever exists)
        HN_HIP(ctx, hipMalloc((void**)&u->w, L.total * sizeof(float)));
        HN_HIP(ctx, hipMemcpy(u->w, ctx->raw_blob.data(), L.total * sizeof(float), hipMemcpyHostToDevice));
        const float* w = u->w;
        for_each_layer(depth,
            [&](int, int, int, const RawDc& r, JvpDc& l) { l = JvpDc{w + r.w1, w + r.b1, w + r.slope, w + r.w2, w + r.b2, r.cin, r.cm, r.co}; },
            [&](bool, const RawK8& r, JvpK8& l) { l = JvpK8{w + r.w, w + r.b}; }, L, *u);
        u->outc_w = w + L.outc_w;
        u->outc_b = w + L.outc_b;
        int rc = dc_attr<kInCh, 0, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kState, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kState, kState, kState>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, kFeat, kFeat, kFeat>(ctx);
        if (rc == HN_OK) rc = dc_attr<kFeat, 0, kFeat, kFeat>(ctx);
        if (rc != HN_OK) return rc;
    }
    JvpWs* u = ctx->jvp;
    if (batch > u->cap) {
        u->cap = 0;
        const size_t plane = (size_t)n * n, per2 = sizeof(float2) * batch, per = sizeof(float) * batch;
        std::vector<size_t> sizes{per2 * kInCh * plane};
        for (int d = 0; d <= depth; ++d) sizes.insert(sizes.end(), d < depth ? 3 : 2, per2 * kFeat * (n >> d) * (n >> d));
        sizes.insert(sizes.end(), {per * 2 * plane, per * kState * ctx->state_len, per * 2 * plane, sizeof(float) * 2 * plane});
        if (const int rc = u->block.alloc(ctx, "forward-mode loop", sizes.data(), (int)sizes.size()); rc != HN_OK) return rc;
        u->in6 = static_cast<float2*>(u->block.take());
        for (int d = 0; d <= depth; ++d) {
            u->a[d] = static_cast<float2*>(u->block.take());
            u->y[d] = static_cast<float2*>(u->block.take());
            if (d < depth) u->o[d] = static_cast<float2*>(u->block.take());
        }
        u->td = static_cast<float*>(u->block.take());
        u->st_tmp = static_cast<float*>(u->block.take());
        u->stilde = static_cast<float*>(u->block.take());
        u->zero = static_cast<float*>(u->block.take());   // (the block comes zeroed and nothing writes here)
        u->cap = batch;
    }
    return HN_OK;
}
// weights and workspace for `batch` samples: built by the first call, grown by a larger batch -- never under stream capture
int prepare(hn_ctx* ctx, int batch, hipStream_t s) {
    if (ctx->jvp != nullptr && batch <= ctx->jvp->cap) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "hn_step_jvp: the workspace (or a larger batch's) is built by the first call, which must not be under stream capture");
    const int rc = build(ctx, batch);
    if (rc != HN_OK) jvp_free(ctx);   // nothing half-built stays behind
    return rc;
}

// the tangent of one HybridNet forward, layer by layer: the states' primal half from the tape (st), their tangents planar (tst_in -> tst_out)
int forward(hn_ctx* ctx, const float* st, const float* tst_in, float* tst_out, int batch, hipStream_t s) {
    const JvpWs& u = *ctx->jvp;
    const int n = ctx->tab.n, depth = ctx->depth;
    const long L = ctx->state_len;
    const DualIn none{nullptr, nullptr, nullptr, 0, 0};
    auto dense = [](const float2* p, int m) { return DualIn{p, nullptr, nullptr, (long)kFeat * m * m, (long)m * m}; };
    auto dense_out = [](float2* p, int m) { return DualOut{p, nullptr, (long)kFeat * m * m, (long)m * m}; };
    int rc = launch_dc(ctx, DualIn{u.in6, nullptr, nullptr, (long)kInCh * n * n, (long)n * n}, none, dense_out(u.a[0], n), u.inc, n, n, batch, s);
    for (int d = 0; d < depth && rc == HN_OK; ++d) {
        const int m = n >> d;
        const DualIn state{nullptr, st + ctx->state_off[d], tst_in + ctx->state_off[d], kState * L, L};
        rc = launch_dc(ctx, dense(u.a[d], m), state, dense_out(u.o[d], m), u.sig[d], m, m, batch, s);
        if (rc == HN_OK) rc = launch_dc(ctx, dense(u.o[d], m), state, DualOut{nullptr, tst_out + ctx->state_off[d], kState * L, L}, u.st[d], m, m, batch, s);
        const int mo = m >> 1;
        hipLaunchKernelGGL(k_conv8_dual<false>, dim3((mo + kT - 1) / kT, (mo + kT - 1) / kT, batch), dim3(256), 0, s, u.o[d], u.a[d + 1], u.down[d], m, m);
    }
    if (rc == HN_OK) rc = launch_dc(ctx, dense(u.a[depth], n >> depth), none, dense_out(u.y[depth], n >> depth), u.dec[depth], n >> depth, n >> depth, batch, s);
    for (int d = depth - 1; d >= 0 && rc == HN_OK; --d) {
        const int m = n >> d, mi = m >> 1;
        hipLaunchKernelGGL(k_conv8_dual<true>, dim3((mi + kT - 1) / kT, (mi + kT - 1) / kT, batch), dim3(256), 0, s, u.y[d + 1], u.a[d], u.up[d], mi, mi);
        rc = launch_dc(ctx, dense(u.a[d], m), dense(u.o[d], m), dense_out(u.y[d], m), u.dec[d], m, m, batch, s);
    }
    if (rc != HN_OK) return rc;
    const long plane = (long)n * n;
    hipLaunchKernelGGL(k_outc_dual, dim3((unsigned)((plane + 255) / 256), batch), dim3(256), 0, s, u.y[0], u.outc_w, u.outc_b, u.td, plane);
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

}  // namespace

void jvp_free(hn_ctx* ctx) {
    JvpWs* u = ctx->jvp;
    if (u == nullptr) return;
    (void)hipFree(u->w);
    u->block.free();
    delete u;
    ctx->jvp = nullptr;
}

}  // namespace hn

using namespace hn;

extern "C" {

int hn_step_jvp(hn_ctx* ctx, const float* wf0, const float* res0, const float* states0, const float* k_sq, int src_batch, int batch, int n_iter,
                const float* wf_hist, const float* res_hist, const float* st_hist, float* t_wf, float* t_res, float* t_states, const float* t_k_sq,
                const float* t_src, float* t_wf_hist, float* t_res_hist, float* t_st_hist, void* stream) {
    if (!ctx || !wf0 || !res0 || !states0 || !k_sq || !wf_hist || !res_hist || !st_hist || !t_wf || !t_res || !t_states)
        return fail(ctx, HN_ERR_ARG, "hn_step_jvp: NULL argument (the inputs, the three histories and the three tangents are required)");
    if (ctx->rect) return rect_unsupported(ctx, "hn_step_jvp");
    if (!ctx->have_weights) return fail(ctx, HN_ERR_STATE, "hn_load_weights has not been called");
    if (ctx->tab.n == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    if (n_iter < 1) return fail(ctx, HN_ERR_ARG, "hn_step_jvp: n_iter must be >= 1 (got %d)", n_iter);
    if (batch < 1) return fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    if (src_batch != 1 && src_batch != batch) return fail(ctx, HN_ERR_ARG, "source batch %d must be 1 or equal to the batch %d", src_batch, batch);
    const int n = ctx->tab.n;
    if (n % (1 << ctx->depth) != 0) return fail(ctx, HN_ERR_ARG, "domain size %d is not divisible by 2^depth = %d", n, 1 << ctx->depth);
    if (ctx->precision != HN_PREC_FP32 && ctx->precision != HN_PREC_FP32_VALU)
        return fail(ctx, HN_ERR_UNSUPPORTED, "hn_step_jvp: tangents are computed for the fp32 UNet only (the context is set to a 16-bit mode)");
    const size_t plane = (size_t)n * n, L = (size_t)ctx->state_len, F = sizeof(float);
    const size_t fc = (size_t)batch * 2 * plane, sc = (size_t)batch * kState * L, T = (size_t)n_iter;
    const MemRange r[] = {{wf0, F * fc, false, "wf0"}, {res0, F * fc, false, "res0"}, {states0, F * sc, false, "states0"}, {k_sq, F * batch * plane, false, "k_sq"},
                          {wf_hist, F * T * fc, false, "wf_hist"}, {res_hist, F * T * fc, false, "res_hist"}, {st_hist, F * T * sc, false, "st_hist"},
                          {t_wf, F * fc, true, "t_wf"}, {t_res, F * fc, true, "t_res"}, {t_states, F * sc, true, "t_states"},
                          {t_k_sq, F * batch * plane, false, "t_k_sq"}, {t_src, F * src_batch * 2 * plane, false, "t_src"},
                          {t_wf_hist, F * T * fc, true, "t_wf_hist"}, {t_res_hist, F * T * fc, true, "t_res_hist"}, {t_st_hist, F * T * sc, true, "t_st_hist"}};
    const char *who, *other;
    if (first_overlap(r, 15, &who, &other)) return fail(ctx, HN_ERR_ARG, "hn_step_jvp: %s overlaps %s", who, other);
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    int rc = prepare(ctx, batch, s);
    if (rc != HN_OK) return rc;
    JvpWs& u = *ctx->jvp;
    const bool have_src = t_k_sq != nullptr || t_src != nullptr;
    const dim3 field((unsigned)((2 * plane + 255) / 256), batch);
    for (int it = 0; it < n_iter; ++it) {
        // the linearisation point: the tape slot in front of this iteration (the caller's inputs for the first one)
        const float* wf_p = it ? wf_hist + (size_t)(it - 1) * fc : wf0;
        const float* res_p = it ? res_hist + (size_t)(it - 1) * fc : res0;
        const float* st_p = it ? st_hist + (size_t)(it - 1) * sc : states0;
        const float* tst_in = (it & 1) ? u.st_tmp : t_states;   // the state tangents ping-pong between the caller's buffer and the library's
        float* tst_out = (it & 1) ? t_states : u.st_tmp;
        hipLaunchKernelGGL(k_in6_dual, field, dim3(256), 0, s, wf_p, res_p, t_wf, t_res, ctx->tab.sigmas, u.in6, (long)plane);
        if ((rc = forward(ctx, st_p, tst_in, tst_out, batch, s)) != HN_OK) return rc;
        hipLaunchKernelGGL(k_update_tan, dim3((unsigned)((fc + 255) / 256)), dim3(256), 0, s, t_wf, u.td, (long)fc);
        if (have_src) {
            hipLaunchKernelGGL(k_jvp_src, field, dim3(256), 0, s, t_src, src_batch == 1 ? 0L : (long)(2 * plane), t_k_sq, wf_hist + (size_t)it * fc, u.stilde,
                               (long)plane);
            rc = spec_apply(ctx, t_wf, t_res, k_sq, u.stilde, batch, batch, nullptr, s);
        } else {
            rc = spec_apply(ctx, t_wf, t_res, k_sq, u.zero, 1, batch, nullptr, s);   // the zero-source form of the GMRES operator
        }
        if (rc != HN_OK) return rc;
        if (t_wf_hist) HN_HIP(ctx, hipMemcpyAsync(t_wf_hist + (size_t)it * fc, t_wf, F * fc, hipMemcpyDeviceToDevice, s));
        if (t_res_hist) HN_HIP(ctx, hipMemcpyAsync(t_res_hist + (size_t)it * fc, t_res, F * fc, hipMemcpyDeviceToDevice, s));
        if (t_st_hist) HN_HIP(ctx, hipMemcpyAsync(t_st_hist + (size_t)it * sc, tst_out, F * sc, hipMemcpyDeviceToDevice, s));
    }
    if (n_iter & 1) HN_HIP(ctx, hipMemcpyAsync(t_states, u.st_tmp, F * sc, hipMemcpyDeviceToDevice, s));
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

}  // extern "C"
