// Spectral Laplacian for n = P * Q with a RUNTIME odd factor P (HN_OPT_SPECTRAL_MIXED): the sizes 144, 240, 400, 576, 1040, ... that
// neither the power-of-two kernels nor k_spec_pfa<Q, P> (P = 3, 5, 7 held in registers) of hn_spectral.hip take, and that otherwise
// run the dense n x n operator.  Same operator, same Good-Thomas maps as k_spec_pfa (read its header comment):
//   input map   i = (Q n1 + P n2) mod n        output map   k = (Q (Q^-1 mod P) k1 + P (P^-1 mod Q) k2) mod n
//   X[k(k1, k2)] = sum_n1 W_P^(n1 k1) sum_n2 W_Q^(n2 k2) x[i(n1, n2)]          (no twiddles between the factors)
// The difference: a line lives in LDS as [P][Q] (element i at slot n1 * Q + n2, a host table), not in registers.
//   1  load the line(s) of the block into buffer 0 at their slots (adjoint: times conj(a) and conj(b) into buffers 0 and 1)
//   2  P * lines Q-point transforms IN PLACE: decimation in frequency, two radix-2 stages per LDS round trip, no reordering -- position r of a
//      transform then holds k2 = bitrev(r); the host bakes that, like the output map, into the k tables (k1m / k2m)
//   3  direct P-point DFT across the sub-sequences, times i k and -k^2: buffers 1 and 2 (adjoint: of both, combined as (-i k) Z1 + (-k^2) Z2)
//   4  inverse P-point DFT: buffers 0 and 3 (adjoint: buffer 0)
//   5  inverse Q-point transforms in place: decimation in time from bit-reversed input, the mirror image of 2
//   6  PML coefficients at the natural index, the row pass's residual terms and sum of squares, store the way the line was loaded
// The P-point DFT uses W_P^(s (P - k)) = conj(W_P^(s k)): one work item computes A = sum x cos and B = sum x (-+sin) once and emits outputs k and P - k
// (A +- i B): half the multiply-adds and half the LDS reads of the plain double loop.  Each sum runs in two interleaved partial
// accumulators (even and odd terms): at P = 127 that halves the length of the longest fp32 chain.
// All 256 threads of a block work through the items of all its lines between block barriers; which thread computes an element
// does not change the element's arithmetic, so a sample's bits do not depend on the lines per block (and with it not on the batch).
// Lines are independent: no flags, no cross-workgroup waits, no atomics but the row pass's sum of squares (one per block).
#include <cmath>
#include <vector>

#include "hn_internal.h"

namespace hn {
namespace {

#include "hn_spectral_lds.inc"

constexpr int kMixLdsAttr = 96 * 1024;    // dynamic LDS the four kernels may ask for
constexpr int kMixLdsLines = 80 * 1024;   // budget of a block's line buffers: two blocks per CU

struct MixTabs {
    const float2* tw_q;   // exp(-2 pi i m / Q)
    const float2* wp;     // exp(-2 pi i m / P)
    const float* k1m;     // [P][Q]: k at (k1, position r)
    const float* k2m;     // -k^2 likewise
    const float2* a;      // PML coefficients, natural order
    const float2* b;
    const int* slot;      // [n]: n1 * Q + n2 of element i
};

// One kernel for both axes and both directions; L = 1 << logl lines per block, n = P << logq.
//   AXIS 0: along W (row pass: adds the column part with flags & 1, the residual terms with flags & 2, the sum of squares)
//   AXIS 1: along H (column pass: the block's L adjacent columns are loaded and stored as row segments of L floats)
// Dynamic LDS: (ADJ ? 3 : 4) buffers of L * n float2, then the Q and P twiddles.
template <int AXIS, bool ADJ>
__global__ __launch_bounds__(kMixThreads) void k_spec_mixed(const float* __restrict__ wf, float* out, const float* __restrict__ ksq,
                                                            const float* __restrict__ src, long src_sb, MixTabs t, int n, int P, int logq, int logl,
                                                            int flags, float* __restrict__ sumsq, const int* __restrict__ it_counter,
                                                            int sumsq_stride, const float* add) {
    constexpr int NBUF = ADJ ? 3 : 4;
    extern __shared__ float2 mbuf[];
    __shared__ float red[kMixThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Q = 1 << logq, L = 1 << logl, PH = (P + 1) >> 1;
    const int ln = L * n;                 // float2 per buffer
    float2* const B0 = mbuf;
    float2* const B1 = mbuf + ln;
    float2* const B2 = mbuf + 2 * ln;
    float2* const B3 = mbuf + 3 * ln;     // (forward only)
    float2* const twq = mbuf + NBUF * ln;
    float2* const wp = twq + Q;
    const long plane = (long)n * n;
    const int line0 = blockIdx.x * L;
    for (int i = tid; i < Q; i += kMixThreads) twq[i] = t.tw_q[i];
    for (int i = tid; i < P; i += kMixThreads) wp[i] = t.wp[i];
    // ---- 1: load
    const float* pre = wf + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kMixThreads) {
        const int l = AXIS == 0 ? e / n : e & (L - 1);
        const int i = AXIS == 0 ? e - l * n : e >> logl;
        const int line = line0 + l;
        float2 u = make_float2(0.f, 0.f);       // a block's lines past the last one carry zeros and are not stored
        if (line < n) {
            const long o = AXIS == 0 ? (long)line * n + i : (long)i * n + line;
            u = make_float2(pre[o], pre[o + plane]);
        }
        const int sl = l * n + t.slot[i];
        if (!ADJ) {
            B0[sl] = u;
        } else {
            B0[sl] = cmulc(u, t.a[i]);
            B1[sl] = cmulc(u, t.b[i]);
        }
    }
    __syncthreads();
    // ---- 2: Q-point transforms of the L * P sub-sequences
    fft_inplace<false>(B0, B1, ADJ ? 2 : 1, L * P, logq, twq, tid);
    // ---- 3: P-point DFT, derivative multipliers
    for (int item = tid; item < (L * PH) << logq; item += kMixThreads) {
        const int r = item & (Q - 1), lk = item >> logq;
        const int l = lk / PH, k1 = lk - l * PH;
        const int base = l * n + r;
        float2 A[ADJ ? 2 : 1], Bv[ADJ ? 2 : 1];
        pdft_sums<ADJ ? 2 : 1>(B0 + base, B1 + base, Q, P, k1, wp, A, Bv);
#pragma unroll
        for (int m = 0; m < 2; ++m) {            // output k1, then its mirror P - k1
            if (m == 1 && k1 == 0) break;
            const int kk = m == 0 ? k1 : P - k1;
            const float kk1 = t.k1m[(kk << logq) + r], kk2 = t.k2m[(kk << logq) + r];
            const float2 Y = m == 0 ? plus_i(A[0], Bv[0]) : minus_i(A[0], Bv[0]);
            const int o = base + (kk << logq);
            if (!ADJ) {
                B1[o] = make_float2(-Y.y * kk1, Y.x * kk1);   // (0, k) * U     (spectral.py:50, 281)
                B2[o] = make_float2(kk2 * Y.x, kk2 * Y.y);    // (-k^2, 0) * U  (spectral.py:52, 283)
            } else {                                          // (-i k) Z1 + (-k^2) Z2
                const float2 Y2 = m == 0 ? plus_i(A[ADJ ? 1 : 0], Bv[ADJ ? 1 : 0]) : minus_i(A[ADJ ? 1 : 0], Bv[ADJ ? 1 : 0]);
                B2[o] = make_float2(kk1 * Y.y + kk2 * Y2.x, -kk1 * Y.x + kk2 * Y2.y);
            }
        }
    }
    __syncthreads();
    // ---- 4: inverse P-point DFT
    for (int item = tid; item < (L * PH) << logq; item += kMixThreads) {
        const int r = item & (Q - 1), lk = item >> logq;
        const int l = lk / PH, s = lk - l * PH;
        const int base = l * n + r;
        float2 A[ADJ ? 1 : 2], Bv[ADJ ? 1 : 2];
        pdft_sums<ADJ ? 1 : 2>(ADJ ? B2 + base : B1 + base, B2 + base, Q, P, s, wp, A, Bv);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (m == 1 && s == 0) break;
            const int o = base + ((m == 0 ? s : P - s) << logq);
            B0[o] = m == 0 ? minus_i(A[0], Bv[0]) : plus_i(A[0], Bv[0]);
            if (!ADJ) B3[o] = m == 0 ? minus_i(A[ADJ ? 0 : 1], Bv[ADJ ? 0 : 1]) : plus_i(A[ADJ ? 0 : 1], Bv[ADJ ? 0 : 1]);
        }
    }
    __syncthreads();
    // ---- 5: inverse Q-point transforms
    fft_inplace<true>(B0, B3, ADJ ? 1 : 2, L * P, logq, twq, tid);
    // ---- 6: PML coefficients, the pass's other terms, store
    const float inv_n = 1.0f / (float)n;
    float ss = 0.f;
    float* po = out + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kMixThreads) {
        const int l = AXIS == 0 ? e / n : e & (L - 1);
        const int i = AXIS == 0 ? e - l * n : e >> logl;
        const int line = line0 + l;
        if (line >= n) continue;
        const int sl = l * n + t.slot[i];
        float re, im;
        if (ADJ) {
            re = B0[sl].x * inv_n;
            im = B0[sl].y * inv_n;
        } else {
            const float2 p = cmul(t.a[i], B0[sl]), r = cmul(t.b[i], B3[sl]);
            re = (p.x + r.x) * inv_n;
            im = (p.y + r.y) * inv_n;
        }
        const long o = AXIS == 0 ? (long)line * n + i : (long)i * n + line;
        if (AXIS == 0) {
            if (flags & 1) { re += po[o]; im += po[o + plane]; }
            if (flags & 2) {
                const float kq = ksq[(long)b * plane + o];
                re = re + kq * pre[o];          // the line itself again (an L2 hit) instead of a copy held through the transforms
                im = im + kq * pre[o + plane];
                if (src != nullptr) {
                    const float* ps = src + (long)b * src_sb + o;
                    re -= ps[0];
                    im -= ps[plane];
                }
            }
        } else if (ADJ && add != nullptr) {     // `add` may alias `out`: the same thread reads and writes the element
            const float* pa = add + (long)b * 2 * plane;
            re += pa[o];
            im += pa[o + plane];
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

__global__ void k_mixed_bump(int* counter) { atomicAdd(counter, 1); }

int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Lines per block (a power of two): at most 16 -- the column pass then moves 64-byte row segments -- and at most kMixLdsLines of line buffers;
// fewer while the launch would not give every CU two blocks (small problems: latency, not throughput).  With four buffers: 16 lines up to
// n = 160, 8 up to 320, 4 up to 640, 2 up to 1280, then 1; halved while ceil(n / lines) * batch < 512.
int mixed_lines(int n, int nbuf, int batch) {
    int L = 16;
    while (L > 1 && (size_t)L * nbuf * n * sizeof(float2) > (size_t)kMixLdsLines) L >>= 1;
    while (L > 1 && (long)((n + L - 1) / L) * batch < 512) L >>= 1;
    return L;
}

template <bool ADJ>
int launch_mixed(hn_ctx* ctx, const float* wf, float* out, const float* ksq, const float* src, long src_sb, int batch, bool resid, float* sumsq,
                 hipStream_t s, int* it_counter, int sumsq_stride, const float* add) {
    const SpecTables& t = ctx->tab;
    const int n = t.n, P = t.mix_p, Q = t.mix_q, nbuf = ADJ ? 3 : 4;
    const int L = mixed_lines(n, nbuf, batch);
    const size_t lds = ((size_t)L * nbuf * n + Q + P) * sizeof(float2);
    if (lds > (size_t)kMixLdsAttr) return fail(ctx, HN_ERR_ARG, "internal: mixed spectral kernel needs %zu bytes of LDS at n = %d", lds, n);
    const MixTabs mt{t.tw_q, t.mix_wp, t.k1_pfa, t.k2_pfa, t.a, t.b, t.mix_slot};
    const dim3 grid((n + L - 1) / L, batch);
    if (it_counter != nullptr) hipLaunchKernelGGL(k_mixed_bump, dim3(1), dim3(1), 0, s, it_counter);
    {
        ProfScope ps(ctx, KID_SPEC_COLS, s);
        hipLaunchKernelGGL((k_spec_mixed<1, ADJ>), grid, dim3(kMixThreads), lds, s, wf, out, nullptr, nullptr, 0L, mt, n, P, ilog2(Q), ilog2(L), 0,
                           nullptr, nullptr, 0, add);
    }
    ProfScope ps(ctx, KID_SPEC_ROWS, s);
    hipLaunchKernelGGL((k_spec_mixed<0, ADJ>), grid, dim3(kMixThreads), lds, s, wf, out, ksq, src, src_sb, mt, n, P, ilog2(Q), ilog2(L),
                       1 | (resid ? 2 : 0), sumsq, it_counter, sumsq_stride, nullptr);
    return HN_OK;
}

template <typename T>
int upload(hn_ctx* ctx, T** dst, const std::vector<T>& h) {
    HN_HIP(ctx, hipMalloc((void**)dst, h.size() * sizeof(T)));
    HN_HIP(ctx, hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return HN_OK;
}

}  // namespace

bool spec_mixed_factor(int n, int* P, int* Q) {
    if (n <= 0) return false;
    int q = 1;
    while ((n & q) == 0) q <<= 1;     // the largest power of two that divides n
    const int p = n / q;
    if (p < 3 || p > 127 || q < 16 || q > 512) return false;
    *P = p;
    *Q = q;
    return true;
}

int spec_mixed_build(hn_ctx* ctx, const AxisHost& ax, int P, int Q) {
    SpecTables& t = ctx->tab;
    const int n = P * Q, logq = ilog2(Q);
    const double pi = 3.14159265358979323846;
    int qinv = 1, pinv = 1;
    while ((Q * qinv) % P != 1) ++qinv;
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
    if ((rc = upload(ctx, &t.mix_wp, wp)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.mix_slot, slot)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.k1_pfa, k1m)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.k2_pfa, k2m)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.a, ax.fa)) != HN_OK) return rc;
    if ((rc = upload(ctx, &t.b, ax.fb)) != HN_OK) return rc;
    // here and not at the first launch: a first call under stream capture is then nothing but launches
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_mixed<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kMixLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_mixed<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kMixLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_mixed<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMixLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_mixed<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMixLdsAttr));
    t.mix_p = P;
    t.mix_q = Q;
    return HN_OK;
}

int spec_mixed_apply(hn_ctx* ctx, const float* wf, float* out, const float* ksq, const float* src, long src_sb, int batch, bool resid,
                     float* sumsq, hipStream_t s, int* it_counter, int sumsq_stride) {
    return launch_mixed<false>(ctx, wf, out, ksq, src, src_sb, batch, resid, sumsq, s, it_counter, sumsq_stride, nullptr);
}

int spec_mixed_adjoint(hn_ctx* ctx, const float* g, float* out, const float* ksq, const float* add, int batch, hipStream_t s) {
    return launch_mixed<true>(ctx, g, out, ksq, nullptr, 0L, batch, true, nullptr, s, nullptr, 0, add);
}

}  // namespace hn
