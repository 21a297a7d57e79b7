// Spectral Laplacian on a rectangular h x w domain (hn_set_domain_rect, h != w): the algorithm of k_spec_mixed (hn_spectral_mixed.hip; read its header comment)
// with the line length, the line count and the row pitch as three arguments instead of one n, forward operator only.
//   column pass   lines of length h, w of them, element stride w:   out  = ay d/dy + by d2/dy2
//   row pass      lines of length w, h of them:                      out += ax d/dx + bx d2/dx2 [+ k_sq u - src], per-sample sum of squares
// Each axis is factored on its own, len = P * Q with P odd in [1, 127] and Q = 2^k in [16, 2048] (every multiple of 16 up to 2048), and has its own tables; a line
// lives in LDS as [P][Q].  P = 1 (a power of two) has no P-point DFT: the derivative multipliers are applied where the forward transforms left the spectrum and
// the inverse transforms run on those two buffers, so such a line needs three buffers instead of four.  The longest line, 2048 points in three buffers plus its
// twiddles, takes 64 KB; the longest four-buffer line, 2032 = 127 * 16, 63.6 KB + 1.1 KB: both inside the 96 KB attribute.
// All 256 threads of a block work through the items of all its lines between block barriers; which thread computes an element does not change the element's
// arithmetic, so a sample's bits do not depend on the lines per block (and with it not on the batch).
// Lines are independent: no flags, no cross-workgroup waits, no atomics but the row pass's sum of squares (one per block).
#include <cmath>
#include <vector>

#include "hn_internal.h"

namespace hn {
namespace {

#include "hn_spectral_lds.inc"

constexpr int kRectLdsAttr = 96 * 1024;    // dynamic LDS the two kernels may ask for
constexpr int kRectLdsLines = 80 * 1024;   // budget of a block's line buffers: two blocks per CU

struct RectTabs {
    const float2* tw_q;   // exp(-2 pi i m / Q)
    const float2* wp;     // exp(-2 pi i m / P)
    const float* k1m;     // [P][Q]: k at (k1, position r)
    const float* k2m;     // -k^2 likewise
    const float2* a;      // PML coefficients of this axis, natural order
    const float2* b;
    const int* slot;      // [len]: n1 * Q + n2 of element i
};

// One kernel for both axes; L = 1 << logl lines per block, len = P << logq points per line, `count` lines, rows of the tensor `pitch` floats apart.
//   AXIS 0: along x (row pass: line `r` is row r; adds the column part with flags & 1, the residual terms with flags & 2, the sum of squares)
//   AXIS 1: along y (column pass: line `c` is column c; the block's L adjacent columns are loaded and stored as row segments of L floats)
// Dynamic LDS: (P == 1 ? 3 : 4) buffers of L * len float2, then the Q and P twiddles.
// KsqIm: empty (the lossless kernels, whose instantiations <0> and <1> are what they were before the pack existed), or one const float*: the row pass of
// hn_residual_lossy / hn_step_lossy / hn_fgmres_cycle_lossy, whose pointwise term is complex, (ksq + i ksq_im) u.
template <int AXIS, typename... KsqIm>
__global__ __launch_bounds__(kMixThreads) void k_spec_rect(const float* __restrict__ wf, float* out, const float* __restrict__ ksq,
                                                           const float* __restrict__ src, long src_sb, RectTabs t, int len, int count, int pitch, int P,
                                                           int logq, int logl, int flags, float* __restrict__ sumsq,
                                                           const int* __restrict__ it_counter, int sumsq_stride, KsqIm... ksq_im) {
    extern __shared__ float2 rbuf[];
    __shared__ float red[kMixThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Q = 1 << logq, L = 1 << logl, PH = (P + 1) >> 1;
    const int ln = L * len;               // float2 per buffer
    float2* const B0 = rbuf;
    float2* const B1 = rbuf + ln;
    float2* const B2 = rbuf + 2 * ln;
    float2* const B3 = rbuf + 3 * ln;     // (P > 1 only)
    float2* const twq = rbuf + (P == 1 ? 3 : 4) * ln;
    float2* const wp = twq + Q;
    const long plane = AXIS == 0 ? (long)count * pitch : (long)len * pitch;
    const int line0 = blockIdx.x * L;
    for (int i = tid; i < Q; i += kMixThreads) twq[i] = t.tw_q[i];
    for (int i = tid; i < P; i += kMixThreads) wp[i] = t.wp[i];
    // ---- 1: load
    const float* pre = wf + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kMixThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        float2 u = make_float2(0.f, 0.f);       // a block's lines past the last one carry zeros and are not stored
        if (line < count) {
            const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
            u = make_float2(pre[o], pre[o + plane]);
        }
        B0[l * len + t.slot[i]] = u;
    }
    __syncthreads();
    // ---- 2: Q-point transforms of the L * P sub-sequences
    fft_inplace<false>(B0, B1, 1, L * P, logq, twq, tid);
    // the buffers the inverse transforms run on and the results are read from: first- and second-derivative spectrum
    float2* const D1 = P == 1 ? B1 : B0;
    float2* const D2 = P == 1 ? B2 : B3;
    if (P == 1) {
        // ---- 3 (P = 1): derivative multipliers in place of the P-point DFT pair
        for (int e = tid; e < ln; e += kMixThreads) {
            const int r = e & (Q - 1);
            const float kk1 = t.k1m[r], kk2 = t.k2m[r];
            const float2 Y = B0[e];
            B1[e] = make_float2(-Y.y * kk1, Y.x * kk1);   // (0, k) * U     (spectral.py:50, 281)
            B2[e] = make_float2(kk2 * Y.x, kk2 * Y.y);    // (-k^2, 0) * U  (spectral.py:52, 283)
        }
        __syncthreads();
    } else {
        // ---- 3: direct P-point DFT, derivative multipliers
        for (int item = tid; item < (L * PH) << logq; item += kMixThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, k1 = lk - l * PH;
            const int base = l * len + r;
            float2 A[1], Bv[1];
            pdft_sums<1>(B0 + base, B0 + base, Q, P, k1, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {            // output k1, then its mirror P - k1
                if (m == 1 && k1 == 0) break;
                const int kk = m == 0 ? k1 : P - k1;
                const float kk1 = t.k1m[(kk << logq) + r], kk2 = t.k2m[(kk << logq) + r];
                const float2 Y = m == 0 ? plus_i(A[0], Bv[0]) : minus_i(A[0], Bv[0]);
                const int o = base + (kk << logq);
                B1[o] = make_float2(-Y.y * kk1, Y.x * kk1);
                B2[o] = make_float2(kk2 * Y.x, kk2 * Y.y);
            }
        }
        __syncthreads();
        // ---- 4: inverse P-point DFT of both
        for (int item = tid; item < (L * PH) << logq; item += kMixThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, s = lk - l * PH;
            const int base = l * len + r;
            float2 A[2], Bv[2];
            pdft_sums<2>(B1 + base, B2 + base, Q, P, s, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (m == 1 && s == 0) break;
                const int o = base + ((m == 0 ? s : P - s) << logq);
                B0[o] = m == 0 ? minus_i(A[0], Bv[0]) : plus_i(A[0], Bv[0]);
                B3[o] = m == 0 ? minus_i(A[1], Bv[1]) : plus_i(A[1], Bv[1]);
            }
        }
        __syncthreads();
    }
    // ---- 5: inverse Q-point transforms
    fft_inplace<true>(D1, D2, 2, L * P, logq, twq, tid);
    // ---- 6: PML coefficients, the pass's other terms, store
    const float inv_n = 1.0f / (float)len;
    float ss = 0.f;
    float* po = out + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kMixThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        if (line >= count) continue;
        const int sl = l * len + t.slot[i];
        const float2 p = cmul(t.a[i], D1[sl]), r = cmul(t.b[i], D2[sl]);
        float re = (p.x + r.x) * inv_n;
        float im = (p.y + r.y) * inv_n;
        const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
        if (AXIS == 0) {
            if (flags & 1) { re += po[o]; im += po[o + plane]; }
            if (flags & 2) {
                const float kq = ksq[(long)b * plane + o];
                if constexpr (sizeof...(KsqIm) != 0) {
                    const float* const kim[] = {ksq_im...};
                    const float ki = kim[0][(long)b * plane + o];
                    const float ur = pre[o], ui = pre[o + plane];
                    re = re + (kq * ur - ki * ui);
                    im = im + (kq * ui + ki * ur);
                } else {
                    re = re + kq * pre[o];          // the line itself again (an L2 hit) instead of a copy held through the transforms
                    im = im + kq * pre[o + plane];
                }
                if (src != nullptr) {
                    const float* ps = src + (long)b * src_sb + o;
                    re -= ps[0];
                    im -= ps[plane];
                }
            }
        }
        po[o] = re;
        po[o + plane] = im;
        ss += re * re + im * im;
    }
    if (AXIS == 0 && sumsq != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = ss;
        __syncthreads();
        if (tid == 0) {
            const long row = it_counter != nullptr ? (long)(*it_counter - 1) * sumsq_stride : 0;
            atomicAdd(&sumsq[row + b], (red[0] + red[1]) + (red[2] + red[3]));
        }
    }
}

__global__ void k_rect_bump(int* counter) { atomicAdd(counter, 1); }

int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

int axis_buffers(const RectAxis& ax) { return ax.P == 1 ? 3 : 4; }

// Lines per block (a power of two), the rule of mixed_lines applied to (length, count, batch): at most 16 -- the column pass then moves 64-byte row
// segments -- and at most kRectLdsLines of line buffers; fewer while the launch would not give every CU two blocks.
int rect_lines(int len, int count, int nbuf, int batch) {
    int L = 16;
    while (L > 1 && (size_t)L * nbuf * len * sizeof(float2) > (size_t)kRectLdsLines) L >>= 1;
    while (L > 1 && (long)((count + L - 1) / L) * batch < 512) L >>= 1;
    return L;
}

size_t axis_lds(const RectAxis& ax, int L) { return ((size_t)L * axis_buffers(ax) * ax.len + ax.Q + ax.P) * sizeof(float2); }

template <typename T>
int upload(hn_ctx* ctx, T** dst, const std::vector<T>& h) {
    HN_HIP(ctx, hipMalloc((void**)dst, h.size() * sizeof(T)));
    HN_HIP(ctx, hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return HN_OK;
}

// one axis' tables: spec_mixed_build's, with P = 1 allowed (identity input map, the spectrum in bit-reversed order)
int build_axis(hn_ctx* ctx, RectAxis& t, const AxisHost& ax, int P, int Q) {
    const int n = P * Q, logq = ilog2(Q);
    const double pi = 3.14159265358979323846;
    int qinv = 0, pinv = 1;
    if (P > 1) { qinv = 1; while ((Q * qinv) % P != 1) ++qinv; }
    while ((P * pinv) % Q != 1) ++pinv;
    std::vector<float2> twq(Q), wp(P);
    for (int m = 0; m < Q; ++m) twq[m] = make_float2((float)std::cos(2.0 * pi * m / Q), (float)-std::sin(2.0 * pi * m / Q));
    for (int m = 0; m < P; ++m) wp[m] = make_float2((float)std::cos(2.0 * pi * m / P), (float)-std::sin(2.0 * pi * m / P));
    std::vector<int> slot(n);
    for (int i = 0; i < n; ++i) slot[i] = (((i % P) * qinv) % P) * Q + ((i % Q) * pinv) % Q;   // i = (Q n1 + P n2) mod n
    std::vector<float> k1m((size_t)n), k2m((size_t)n);
    for (int a1 = 0; a1 < P; ++a1)
        for (int r = 0; r < Q; ++r) {
            int a2 = 0;                                    // position r of an in-place transform holds k2 = bitrev(r)
            for (int bit = 0; bit < logq; ++bit) a2 |= ((r >> bit) & 1) << (logq - 1 - bit);
            const int kk = (int)(((long)Q * qinv * a1 + (long)P * pinv * a2) % n);   // Good-Thomas output map
            k1m[(size_t)a1 * Q + r] = ax.k1[kk];
            k2m[(size_t)a1 * Q + r] = ax.k2[kk];
        }
    int rc;
    if ((rc = upload(ctx, &t.tw_q, twq)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.wp, wp)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.slot, slot)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.k1m, k1m)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.k2m, k2m)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.a, ax.fa)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.b, ax.fb)) != HN_OK) return rc;
    t.len = n;
    t.P = P;
    t.Q = Q;
    return HN_OK;
}

void free_axis(RectAxis& t) {
    for (void* p : {(void*)t.tw_q, (void*)t.wp, (void*)t.slot, (void*)t.k1m, (void*)t.k2m, (void*)t.a, (void*)t.b}) (void)hipFree(p);
    t = RectAxis{};
}

}  // namespace

bool spec_rect_factor(int len, int* P, int* Q) {
    if (len <= 0) return false;
    int q = 1;
    while ((len & q) == 0) q <<= 1;     // the largest power of two that divides len
    const int p = len / q;
    if (p > 127 || q < 16 || q > 2048) return false;
    *P = p;
    *Q = q;
    return true;
}

void spec_rect_free(hn_ctx* ctx) {
    if (ctx->rect == nullptr) return;
    free_axis(ctx->rect->cols);
    free_axis(ctx->rect->rows);
    (void)hipFree(ctx->rect->sigmas);
    delete ctx->rect;
    ctx->rect = nullptr;
}

int spec_rect_build(hn_ctx* ctx, int h, int w, int pml, double sigma_max, double k) {
    int ph = 0, qh = 0, pw = 0, qw = 0;
    if (!spec_rect_factor(h, &ph, &qh) || !spec_rect_factor(w, &pw, &qw))
        return fail(ctx, HN_ERR_ARG, "internal: no factorisation of the rectangular domain %d x %d", h, w);
    spec_rect_free(ctx);
    RectDomain* r = new (std::nothrow) RectDomain();
    if (r == nullptr) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    ctx->rect = r;   // (a failure below leaves a domain whose launches are refused: spec_rect_apply checks the tables)
    r->h = h;
    r->w = w;
    const AxisHost ah = spec_axis_host(h, pml, sigma_max, k), aw = spec_axis_host(w, pml, sigma_max, k);
    std::vector<float> sig((size_t)2 * h * w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            sig[(size_t)y * w + x] = (float)aw.sigma[x];                  // sigma_x[i, j] = sigma_w[j]
            sig[(size_t)h * w + (size_t)y * w + x] = (float)ah.sigma[y];  // sigma_y[i, j] = sigma_h[i]
        }
    int rc;
    if ((rc = upload(ctx, &r->sigmas, sig)) != HN_OK || (rc = build_axis(ctx, r->cols, ah, ph, qh)) != HN_OK ||
        (rc = build_axis(ctx, r->rows, aw, pw, qw)) != HN_OK) {
        spec_rect_free(ctx);
        return rc;
    }
    // here and not at the first launch: a first call under stream capture is then nothing but launches
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_rect<0>), hipFuncAttributeMaxDynamicSharedMemorySize, kRectLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_rect<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kRectLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_rect<0, const float*>), hipFuncAttributeMaxDynamicSharedMemorySize, kRectLdsAttr));
    return HN_OK;
}

namespace {

// both passes on `s` for an h x w field: `cols` lines of length h, `rows` lines of length w.  ksq_im nullptr: the launches of spec_rect_apply as they have
// always been; else the row pass is k_spec_rect<0, const float*> (ksq non-null)
int rect_launch(hn_ctx* ctx, const RectAxis& cols, const RectAxis& rows, int h, int w, const float* wf, float* out, const float* ksq, const float* ksq_im,
                const float* src, int src_batch, int batch, float* sumsq, hipStream_t s, int* it_counter, int sumsq_stride) {
    const bool resid = ksq != nullptr;
    const long src_sb = src_batch == 1 ? 0 : 2L * h * w;
    const int Lc = rect_lines(h, w, axis_buffers(cols), batch), Lr = rect_lines(w, h, axis_buffers(rows), batch);
    const size_t lds_c = axis_lds(cols, Lc), lds_r = axis_lds(rows, Lr);
    if (lds_c > (size_t)kRectLdsAttr || lds_r > (size_t)kRectLdsAttr)
        return fail(ctx, HN_ERR_ARG, "internal: rectangular spectral kernel needs %zu / %zu bytes of LDS at %d x %d", lds_c, lds_r, h, w);
    const RectTabs tc{cols.tw_q, cols.wp, cols.k1m, cols.k2m, cols.a, cols.b, cols.slot};
    const RectTabs tr{rows.tw_q, rows.wp, rows.k1m, rows.k2m, rows.a, rows.b, rows.slot};
    ProfScope pair(ctx, KID_SPEC_PAIR, s);
    if (it_counter != nullptr) hipLaunchKernelGGL(k_rect_bump, dim3(1), dim3(1), 0, s, it_counter);
    {
        ProfScope ps(ctx, KID_SPEC_COLS, s);
        hipLaunchKernelGGL((k_spec_rect<1>), dim3((w + Lc - 1) / Lc, batch), dim3(kMixThreads), lds_c, s, wf, out, nullptr, nullptr, 0L, tc, h, w, w, cols.P,
                           ilog2(cols.Q), ilog2(Lc), 0, nullptr, nullptr, 0);
    }
    {
        ProfScope ps(ctx, KID_SPEC_ROWS, s);
        if (ksq_im != nullptr)
            hipLaunchKernelGGL((k_spec_rect<0, const float*>), dim3((h + Lr - 1) / Lr, batch), dim3(kMixThreads), lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P,
                               ilog2(rows.Q), ilog2(Lr), 1 | 2, sumsq, it_counter, sumsq_stride, ksq_im);
        else
            hipLaunchKernelGGL((k_spec_rect<0>), dim3((h + Lr - 1) / Lr, batch), dim3(kMixThreads), lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P,
                               ilog2(rows.Q), ilog2(Lr), 1 | (resid ? 2 : 0), sumsq, it_counter, sumsq_stride);
    }
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

}  // namespace

int spec_rect_apply(hn_ctx* ctx, const float* wf, float* out, const float* ksq, const float* src, int src_batch, int batch, float* sumsq,
                    hipStream_t s, int* it_counter, int sumsq_stride) {
    const RectDomain* r = ctx->rect;
    if (r == nullptr || r->rows.len == 0 || r->cols.len == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain_rect has not been called");
    if (batch <= 0) return HN_OK;
    return rect_launch(ctx, r->cols, r->rows, r->h, r->w, wf, out, ksq, nullptr, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride);
}

// ---- the lossy operator: res = L(u) + (ksq + i ksq_im) u - src on either kind of domain ----
// A rectangular domain has its tables.  A square one gets ONE axis' tables of this file's kernels (both axes of an n x n domain are the same axis), built
// by the first lossy call -- never under stream capture -- and held in ctx->lossy_axis beside ctx->rect, which stays null: the domain stays square.
void spec_lossy_free(hn_ctx* ctx) {
    if (ctx->lossy_axis == nullptr) return;
    free_axis(*ctx->lossy_axis);
    delete ctx->lossy_axis;
    ctx->lossy_axis = nullptr;
}

int spec_lossy_reserve(hn_ctx* ctx, const char* who, hipStream_t s) {
    if (ctx->rect != nullptr) return HN_OK;
    const SpecTables& t = ctx->tab;
    if (t.n == 0) return fail(ctx, HN_ERR_STATE, "%s: hn_set_domain has not been called", who);
    if (ctx->lossy_axis != nullptr && ctx->lossy_axis->len == t.n) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "%s: the tables of the lossy operator on a square domain are built by the first lossy call, which must not be under "
                    "stream capture", who);
    int P = 0, Q = 0;
    if (!spec_rect_factor(t.n, &P, &Q)) return fail(ctx, HN_ERR_ARG, "internal: no factorisation of the domain size %d", t.n);
    spec_lossy_free(ctx);
    RectAxis* ax = new (std::nothrow) RectAxis();
    if (ax == nullptr) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    int rc = build_axis(ctx, *ax, spec_axis_host(t.n, t.pml, t.sigma_max, t.k), P, Q);
    for (const void* k : {reinterpret_cast<const void*>(k_spec_rect<1>), reinterpret_cast<const void*>(k_spec_rect<0, const float*>)})
        if (rc == HN_OK && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kRectLdsAttr) != hipSuccess)
            rc = fail(ctx, HN_ERR_HIP, "%s: hipFuncSetAttribute failed", who);
    if (rc != HN_OK) {
        free_axis(*ax);
        delete ax;
        return rc;
    }
    ctx->lossy_axis = ax;
    return HN_OK;
}

int spec_apply_lossy(hn_ctx* ctx, const char* who, const float* wf, float* out, const float* ksq, const float* ksq_im, const float* src, int src_batch,
                     int batch, float* sumsq, hipStream_t s, int* it_counter, int sumsq_stride) {
    if (ksq == nullptr || ksq_im == nullptr) return fail(ctx, HN_ERR_ARG, "internal: %s: the lossy operator needs both planes of k_sq", who);
    if (const int rc = spec_lossy_reserve(ctx, who, s); rc != HN_OK) return rc;
    if (batch <= 0) return HN_OK;
    if (const RectDomain* r = ctx->rect) {
        if (r->rows.len == 0 || r->cols.len == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain_rect has not been called");
        return rect_launch(ctx, r->cols, r->rows, r->h, r->w, wf, out, ksq, ksq_im, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride);
    }
    const RectAxis& ax = *ctx->lossy_axis;
    return rect_launch(ctx, ax, ax, ax.len, ax.len, wf, out, ksq, ksq_im, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride);
}

int rect_unsupported(hn_ctx* ctx, const char* who) {
    return fail(ctx, HN_ERR_UNSUPPORTED, "%s: not implemented on a rectangular domain (%d x %d, hn_set_domain_rect): the rectangular path covers hn_reserve, "
                "hn_get_sigmas, hn_laplacian, hn_residual, hn_rmse, hn_unet and hn_step in the fp32 precision modes", who, ctx->rect ? ctx->rect->h : 0,
                ctx->rect ? ctx->rect->w : 0);
}

}  // namespace hn
