// Spectral Laplacian on lines of any legal length len = P * Q, P odd in [1, 127] with a RUNTIME value, Q = 2^k in [16, 2048], held in LDS.  One kernel,
// k_spec_line, serves three routes:
//   the mixed route of a square domain (HN_OPT_SPECTRAL_MIXED): the sizes 144, 240, 400, 576, 1040, ... that neither the power-of-two kernels nor
//       k_spec_pfa<Q, P> (P = 3, 5, 7 held in registers) of hn_spectral.hip take, and that otherwise run the dense n x n operator; forward and adjoint
//   a rectangular h x w domain (hn_set_domain_rect, h != w): each axis factored on its own, with its own tables; the lossless operator forward only
//   the lossy operator (complex k_sq) on either kind of domain; forward and adjoint
//       and on its tables the variable-density operator (rho_grad: a - q b on the first derivative, one more plane read per pass) -- forward in step 6,
//       adjoint at the load -- and k_spec_line_d1, the first-derivative pass of hn_adjoint_grad_medium (behind k_spec_line)
// Line length, line count and row pitch are three arguments:
//   column pass   lines of length h, w of them, element stride w:   out  = ay d/dy + by d2/dy2
//   row pass      lines of length w, h of them:                      out += ax d/dx + bx d2/dx2 [+ k_sq u - src], per-sample sum of squares
// Same operator, same Good-Thomas maps as k_spec_pfa (read its header comment):
//   input map   i = (Q n1 + P n2) mod len        output map   k = (Q (Q^-1 mod P) k1 + P (P^-1 mod Q) k2) mod len
//   X[k(k1, k2)] = sum_n1 W_P^(n1 k1) sum_n2 W_Q^(n2 k2) x[i(n1, n2)]          (no twiddles between the factors)
// The difference: a line lives in LDS as [P][Q] (element i at slot n1 * Q + n2, a host table), not in registers.
//   1  load the line(s) of the block into buffer 0 at their slots (adjoint: times conj(a) and conj(b) into buffers 0 and 1)
//   2  P * lines Q-point transforms IN PLACE: decimation in frequency, two radix-2 stages per LDS round trip, no reordering -- position r of a
//      transform then holds k2 = bitrev(r); the host bakes that, like the output map, into the k tables (k1m / k2m)
//   3  direct P-point DFT across the sub-sequences, times i k and -k^2: buffers 1 and 2 (adjoint: of both, combined as (-i k) Z1 + (-k^2) Z2 in buffer 2)
//   4  inverse P-point DFT: buffers 0 and 3 (adjoint: buffer 0)
//   5  inverse Q-point transforms in place: decimation in time from bit-reversed input, the mirror image of 2
//   6  PML coefficients at the natural index (forward), the row pass's residual terms and sum of squares, store the way the line was loaded
// P = 1 (a power of two) has no P-point DFT: the derivative multipliers are applied where the forward transforms left the spectrum and the
// inverse transforms run on those two buffers, so such a line needs three buffers instead of four, as the adjoint does.  (The adjoint of such a line
// combines its two spectra in place in buffer 0 and runs the one inverse transform there; it is sized like every adjoint pass, as three.)  The longest line, 2048 points in
// three buffers plus its twiddles, takes 64 KB; the longest four-buffer line, 2032 = 127 * 16, 63.6 KB + 1.1 KB: both inside the 96 KB attribute.
// The P-point DFT uses W_P^(s (P - k)) = conj(W_P^(s k)): one work item computes A = sum x cos and B = sum x (-+sin) once and emits outputs k and P - k
// (A +- i B): half the multiply-adds and half the LDS reads of the plain double loop.  Each sum runs in two interleaved partial
// accumulators (even and odd terms): at P = 127 that halves the length of the longest fp32 chain.
// All 256 threads of a block work through the items of all its lines between block barriers; which thread computes an element does not change the element's
// arithmetic, so a sample's bits do not depend on the lines per block (and with it not on the batch).
// Lines are independent: no flags, no cross-workgroup waits, no atomics but the row pass's sum of squares (one per block).
#include <cmath>
#include <optional>
#include <vector>

#include "hn_internal.h"

namespace hn {
namespace {

constexpr int kLineThreads = 256;
constexpr int kLineLdsAttr = 96 * 1024;    // dynamic LDS the kernels may ask for
constexpr int kLineLdsLines = 80 * 1024;   // budget of a block's line buffers: two blocks per CU

__device__ __forceinline__ float2 cadd(float2 x, float2 y) { return make_float2(x.x + y.x, x.y + y.y); }
__device__ __forceinline__ float2 csub(float2 x, float2 y) { return make_float2(x.x - y.x, x.y - y.y); }
__device__ __forceinline__ float2 cmul(float2 x, float2 y) { return make_float2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x); }
__device__ __forceinline__ float2 cmulc(float2 x, float2 y) { return make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y); }   // x * conj(y)
__device__ __forceinline__ float2 plus_i(float2 a, float2 b) { return make_float2(a.x - b.y, a.y + b.x); }    // a + i b
__device__ __forceinline__ float2 minus_i(float2 a, float2 b) { return make_float2(a.x + b.y, a.y - b.x); }   // a - i b

// Q-point transforms in place on `nseq` contiguous sequences of each of `nbuf` (1 or 2) buffers.  !INV: decimation in frequency, natural in,
// bit-reversed out.  INV: the transposed flow graph with conjugate twiddles, bit-reversed in, natural out, unnormalised.  One item = the four
// elements {a, a + h/2, a + h, a + 3h/2} that two consecutive radix-2 stages (spans 2h and h) keep among themselves; an odd log2 Q leaves the
// span-2 stage (twiddle 1) on its own.  Ends with a barrier; the caller provides the one in front.
template <bool INV>
__device__ __forceinline__ void fft_inplace(float2* b0, float2* b1, int nbuf, int nseq, int logq, const float2* twq, int tid) {
    const int Q = 1 << logq;
    const int per4 = nseq << (logq - 2), per2 = nseq << (logq - 1);
    auto pairs = [&]() {
        for (int item = tid; item < nbuf * per2; item += kLineThreads) {
            float2* p = (item < per2 ? b0 + 2 * item : b1 + 2 * (item - per2));
            const float2 x0 = p[0], x1 = p[1];
            p[0] = cadd(x0, x1);
            p[1] = csub(x0, x1);
        }
        __syncthreads();
    };
    if (INV && (logq & 1)) pairs();
    // lh = log2 h: logq - 1, logq - 3, ... down to 1 or 2 (forward), the same values upwards (inverse)
    const int lh_last = (logq & 1) ? 2 : 1;
    for (int lh = INV ? lh_last : logq - 1; INV ? lh <= logq - 1 : lh >= lh_last; lh += INV ? 2 : -2) {
        const int h = 1 << lh, hh = h >> 1;
        for (int item = tid; item < nbuf * per4; item += kLineThreads) {
            const int it = item < per4 ? item : item - per4;
            const int seq = it >> (logq - 2), q = it & ((Q >> 2) - 1);
            const int off = q & (hh - 1), blk = q >> (lh - 1);
            float2* p = (item < per4 ? b0 : b1) + (seq << logq) + (blk << (lh + 1)) + off;
            const float2 wa = twq[off << (logq - lh - 1)];          // W_2h^off
            const float2 wb = twq[(off + hh) << (logq - lh - 1)];   // W_2h^(off + h/2)
            const float2 wc = twq[off << (logq - lh)];              // W_h^off
            const float2 x0 = p[0], x1 = p[hh], x2 = p[h], x3 = p[h + hh];
            if (!INV) {
                const float2 y0 = cadd(x0, x2), y2 = cmul(csub(x0, x2), wa);
                const float2 y1 = cadd(x1, x3), y3 = cmul(csub(x1, x3), wb);
                p[0] = cadd(y0, y1);
                p[hh] = cmul(csub(y0, y1), wc);
                p[h] = cadd(y2, y3);
                p[h + hh] = cmul(csub(y2, y3), wc);
            } else {
                const float2 t1 = cmulc(x1, wc), t3 = cmulc(x3, wc);
                const float2 y0 = cadd(x0, t1), y1 = csub(x0, t1), y2 = cadd(x2, t3), y3 = csub(x2, t3);
                const float2 u2 = cmulc(y2, wa), u3 = cmulc(y3, wb);
                p[0] = cadd(y0, u2);
                p[h] = csub(y0, u2);
                p[hh] = cadd(y1, u3);
                p[h + hh] = csub(y1, u3);
            }
        }
        __syncthreads();
    }
    if (!INV && (logq & 1)) pairs();
}

// A[i] = sum_s x_i[s Q] Re w_s, B[i] = sum_s x_i[s Q] Im w_s over the P sub-sequences, w_s = wp[(s kk) mod P], for NIN inputs that share the
// twiddle reads.  With wp = exp(-2 pi i m / P): the forward DFT's outputs kk and P - kk are A + i B and A - i B, the inverse DFT's A - i B and A + i B.
template <int NIN>
__device__ __forceinline__ void pdft_sums(const float2* in0, const float2* in1, int Q, int P, int kk, const float2* wp, float2 (&A)[NIN],
                                          float2 (&B)[NIN]) {
    float2 a0[NIN], b0[NIN], a1[NIN], b1[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) a0[i] = b0[i] = a1[i] = b1[i] = make_float2(0.f, 0.f);
    int idx = 0, s = 0;
    for (; s + 1 < P; s += 2) {
        const float2 w0 = wp[idx];
        idx += kk;
        if (idx >= P) idx -= P;
        const float2 w1 = wp[idx];
        idx += kk;
        if (idx >= P) idx -= P;
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const float2* in = i == 0 ? in0 : in1;
            const float2 x0 = in[s * Q], x1 = in[(s + 1) * Q];
            a0[i].x += x0.x * w0.x; a0[i].y += x0.y * w0.x;
            b0[i].x += x0.x * w0.y; b0[i].y += x0.y * w0.y;
            a1[i].x += x1.x * w1.x; a1[i].y += x1.y * w1.x;
            b1[i].x += x1.x * w1.y; b1[i].y += x1.y * w1.y;
        }
    }
    const float2 w0 = wp[idx];   // P is odd: one term left
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const float2 x0 = (i == 0 ? in0 : in1)[s * Q];
        a0[i].x += x0.x * w0.x; a0[i].y += x0.y * w0.x;
        b0[i].x += x0.x * w0.y; b0[i].y += x0.y * w0.y;
        A[i] = cadd(a0[i], a1[i]);
        B[i] = cadd(b0[i], b1[i]);
    }
}

// what the kernel reads of a LineAxis
struct LineTabs {
    const float2* tw_q;   // exp(-2 pi i m / Q)
    const float2* wp;     // exp(-2 pi i m / P)
    const float* k1m;     // [P][Q]: k at (k1, position r)
    const float* k2m;     // -k^2 likewise
    const float2* a;      // PML coefficients of this axis, natural order
    const float2* b;
    const int* slot;      // [len]: n1 * Q + n2 of element i
};

// One kernel for both axes and both directions; L = 1 << logl lines per block, len = P << logq points per line, `count` lines, rows of the tensor `pitch`
// floats apart.
//   AXIS 0: along x (row pass: line `r` is row r; adds the column part with flags & 1, the residual terms with flags & 2, the sum of squares)
//   AXIS 1: along y (column pass: line `c` is column c; the block's L adjacent columns are loaded and stored as row segments of L floats)
// Dynamic LDS: (ADJ || P == 1 ? 3 : 4) buffers of L * len float2, then the Q and P twiddles.
// ADJ: the adjoint operator; `add` (nullable, may alias `out`) is added by its column pass and read by nothing else.
// KsqIm: empty (the lossless kernels), or one const float*: the row pass of the lossy operator, whose pointwise term is complex -- (ksq + i ksq_im) u
// forward (hn_residual_lossy / hn_step_lossy / hn_fgmres_cycle_lossy), conj(ksq + i ksq_im) g with ADJ (hn_residual_vjp_lossy /
// hn_fgmres_adjoint_cycle_lossy).  The pack stands in front of `add` (legal: every use names the template arguments) so that the forward
// kernels' arguments keep the offsets they had before `add` existed.
// KsqIm of TWO pointers, (ksq_im, rho_grad): the forward passes of the variable-density operator (hn_residual_medium / hn_step_medium /
// hn_fgmres_cycle_medium).  rho_grad is [B][2][h][w], q = d ln rho along x in plane 0 and along y in plane 1; the pass of AXIS reads plane AXIS at the
// element it stores, and step 6 multiplies the first derivative with a[i] - q b[i] instead of a[i]: rho (1/gamma) d((1/rho)(1/gamma) du) in expanded
// form is a du + b d2u - b q du.  ksq_im may then be null (a lossless medium: the plane is not read, the pointwise term is the lossless kernels');
// the column pass is handed null.  Nothing else differs: no further LDS, no further transform.
// The same two pointers with ADJ: the adjoint of that operator (hn_residual_vjp_medium / hn_fgmres_adjoint_cycle_medium),
// L^H g - D^H(conj(b) q g) per axis: the first of the two loads is conj(a - q b) g, q from plane AXIS at the element LOADED (the multiplication stands in
// front of the transposed derivative), the pointwise term conj(ksq + i ksq_im) g or, ksq_im null, ksq g.  LDS and lines per block are the adjoint pass's.
template <int AXIS, bool ADJ, typename... KsqIm>
__global__ __launch_bounds__(kLineThreads) void k_spec_line(const float* __restrict__ wf, float* out, const float* __restrict__ ksq,
                                                            const float* __restrict__ src, long src_sb, LineTabs t, int len, int count, int pitch, int P,
                                                            int logq, int logl, int flags, float* __restrict__ sumsq,
                                                            const int* __restrict__ it_counter, int sumsq_stride, KsqIm... ksq_im, const float* add) {
    constexpr int NF = ADJ ? 2 : 1;       // buffers through the forward transforms
    constexpr bool RHO = sizeof...(KsqIm) == 2;
    static_assert(sizeof...(KsqIm) <= 2, "k_spec_line: (ksq_im) or (ksq_im, rho_grad)");
    extern __shared__ float2 lbuf[];
    __shared__ float red[kLineThreads / 64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Q = 1 << logq, L = 1 << logl, PH = (P + 1) >> 1;
    const int ln = L * len;               // float2 per buffer
    float2* const B0 = lbuf;
    float2* const B1 = lbuf + ln;
    float2* const B2 = lbuf + 2 * ln;
    float2* const B3 = lbuf + 3 * ln;     // (forward, P > 1 only)
    float2* const twq = lbuf + (ADJ || P == 1 ? 3 : 4) * ln;
    float2* const wp = twq + Q;
    const long plane = AXIS == 0 ? (long)count * pitch : (long)len * pitch;
    const int line0 = blockIdx.x * L;
    for (int i = tid; i < Q; i += kLineThreads) twq[i] = t.tw_q[i];
    for (int i = tid; i < P; i += kLineThreads) wp[i] = t.wp[i];
    // ---- 1: load
    const float* pre = wf + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kLineThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        float2 u = make_float2(0.f, 0.f);       // a block's lines past the last one carry zeros and are not stored
        [[maybe_unused]] float q = 0.f;         // (ADJ && RHO) q of this axis at the element loaded
        if (line < count) {
            const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
            u = make_float2(pre[o], pre[o + plane]);
            if constexpr (ADJ && RHO) {
                const float* const kr[] = {ksq_im...};
                q = kr[1][((long)b * 2 + AXIS) * plane + o];
            }
        }
        const int sl = l * len + t.slot[i];
        if constexpr (!ADJ) {
            B0[sl] = u;
        } else if constexpr (RHO) {             // conj(a - q b) g: the forward pass's step-6 coefficient, conjugated
            const float2 ca = t.a[i], cb = t.b[i];
            B0[sl] = cmulc(u, make_float2(ca.x - q * cb.x, ca.y - q * cb.y));
            B1[sl] = cmulc(u, cb);
        } else {
            B0[sl] = cmulc(u, t.a[i]);
            B1[sl] = cmulc(u, t.b[i]);
        }
    }
    __syncthreads();
    // ---- 2: Q-point transforms of the L * P sub-sequences
    fft_inplace<false>(B0, B1, NF, L * P, logq, twq, tid);
    // the buffers the inverse transforms run on and the results are read from: first- and second-derivative spectrum (adjoint: D1 alone, their sum)
    float2* const D1 = !ADJ && P == 1 ? B1 : B0;
    float2* const D2 = !ADJ && P == 1 ? B2 : B3;
    if (P == 1) {
        // ---- 3 (P = 1): derivative multipliers in place of the P-point DFT pair
        for (int e = tid; e < ln; e += kLineThreads) {
            const int r = e & (Q - 1);
            const float kk1 = t.k1m[r], kk2 = t.k2m[r];
            const float2 Y = B0[e];
            if constexpr (!ADJ) {
                B1[e] = make_float2(-Y.y * kk1, Y.x * kk1);   // (0, k) * U     (spectral.py:50, 281)
                B2[e] = make_float2(kk2 * Y.x, kk2 * Y.y);    // (-k^2, 0) * U  (spectral.py:52, 283)
            } else {                                          // (-i k) Z1 + (-k^2) Z2, in place: the element is this thread's alone.  Buffer 2 stays
                                                              // unused here: the launcher sizes every adjoint pass as three buffers, which at
                                                              // len = 256 gives a block 8 lines where two buffers would allow 16 (rect_lines)
                const float2 Y2 = B1[e];
                B0[e] = make_float2(kk1 * Y.y + kk2 * Y2.x, -kk1 * Y.x + kk2 * Y2.y);
            }
        }
        __syncthreads();
    } else {
        // ---- 3: direct P-point DFT, derivative multipliers
        for (int item = tid; item < (L * PH) << logq; item += kLineThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, k1 = lk - l * PH;
            const int base = l * len + r;
            float2 A[NF], Bv[NF];
            pdft_sums<NF>(B0 + base, B1 + base, Q, P, k1, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {            // output k1, then its mirror P - k1
                if (m == 1 && k1 == 0) break;
                const int kk = m == 0 ? k1 : P - k1;
                const float kk1 = t.k1m[(kk << logq) + r], kk2 = t.k2m[(kk << logq) + r];
                const float2 Y = m == 0 ? plus_i(A[0], Bv[0]) : minus_i(A[0], Bv[0]);
                const int o = base + (kk << logq);
                if constexpr (!ADJ) {
                    B1[o] = make_float2(-Y.y * kk1, Y.x * kk1);
                    B2[o] = make_float2(kk2 * Y.x, kk2 * Y.y);
                } else {                                      // (-i k) Z1 + (-k^2) Z2
                    const float2 Y2 = m == 0 ? plus_i(A[NF - 1], Bv[NF - 1]) : minus_i(A[NF - 1], Bv[NF - 1]);
                    B2[o] = make_float2(kk1 * Y.y + kk2 * Y2.x, -kk1 * Y.x + kk2 * Y2.y);
                }
            }
        }
        __syncthreads();
        // ---- 4: inverse P-point DFT (forward: of both)
        constexpr int NI = ADJ ? 1 : 2;
        for (int item = tid; item < (L * PH) << logq; item += kLineThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, s = lk - l * PH;
            const int base = l * len + r;
            float2 A[NI], Bv[NI];
            pdft_sums<NI>(ADJ ? B2 + base : B1 + base, B2 + base, Q, P, s, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (m == 1 && s == 0) break;
                const int o = base + ((m == 0 ? s : P - s) << logq);
                B0[o] = m == 0 ? minus_i(A[0], Bv[0]) : plus_i(A[0], Bv[0]);
                if constexpr (!ADJ) B3[o] = m == 0 ? minus_i(A[NI - 1], Bv[NI - 1]) : plus_i(A[NI - 1], Bv[NI - 1]);
            }
        }
        __syncthreads();
    }
    // ---- 5: inverse Q-point transforms
    fft_inplace<true>(D1, D2, ADJ ? 1 : 2, L * P, logq, twq, tid);
    // ---- 6: PML coefficients, the pass's other terms, store
    const float inv_n = 1.0f / (float)len;
    float ss = 0.f;
    float* po = out + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kLineThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        if (line >= count) continue;
        const int sl = l * len + t.slot[i];
        float2 v;
        if constexpr (ADJ) {                    // (the coefficients went in with the load)
            v = B0[sl];
        } else if constexpr (RHO) {             // a - q b on the first derivative, q from this axis' plane at the element stored below
            const float* const kr[] = {ksq_im...};
            const float q = kr[1][((long)b * 2 + AXIS) * plane + (AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line)];
            const float2 ca = t.a[i], cb = t.b[i];
            const float2 p = cmul(make_float2(ca.x - q * cb.x, ca.y - q * cb.y), D1[sl]), r = cmul(cb, D2[sl]);
            v = make_float2(p.x + r.x, p.y + r.y);
        } else {
            const float2 p = cmul(t.a[i], D1[sl]), r = cmul(t.b[i], D2[sl]);
            v = make_float2(p.x + r.x, p.y + r.y);
        }
        float re = v.x * inv_n;
        float im = v.y * inv_n;
        const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
        if (AXIS == 0) {
            if (flags & 1) { re += po[o]; im += po[o + plane]; }
            if (flags & 2) {
                const float kq = ksq[(long)b * plane + o];
                if constexpr (sizeof...(KsqIm) != 0) {
                    const float* const kim[] = {ksq_im...};
                    if (RHO && kim[0] == nullptr) { // a lossless medium with density: the branch below
                        re = re + kq * pre[o];
                        im = im + kq * pre[o + plane];
                    } else {
                        const float ki = kim[0][(long)b * plane + o];
                        const float ur = pre[o], ui = pre[o + plane];
                        if constexpr (!ADJ) {
                            re = re + (kq * ur - ki * ui);
                            im = im + (kq * ui + ki * ur);
                        } else {                    // conj(ksq + i ksq_im) g: `pre` is the cotangent
                            re = re + (kq * ur + ki * ui);
                            im = im + (kq * ui - ki * ur);
                        }
                    }
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

// The first-derivative pass of the density gradient (hn_adjoint_grad_medium): per line D u = F^-1 (i k) F u on k_spec_line's maps, tables, transforms
// and row-segment addressing, and at the store out[b][AXIS] = Re(conj(lam) * b[i] * D u / len) = dJ/dq of this axis, `lam` read at the element stored;
// `out` is the real [B][2][h][w] field, plane 0 written by the row pass (x), plane 1 by the column pass (y).  A sibling of k_spec_line and not a mode of it:
// there is no second-derivative spectrum, so a line needs ONE buffer at P = 1 (the multiplier goes on in place between the two in-place transforms) and
// two otherwise (the P-point DFTs go from one to the other and back).  Dynamic LDS: (P == 1 ? 1 : 2) buffers of L * len float2, then the Q and P twiddles.
template <int AXIS>
__global__ __launch_bounds__(kLineThreads) void k_spec_line_d1(const float* __restrict__ u, const float* __restrict__ lam, float* __restrict__ out, LineTabs t,
                                                               int len, int count, int pitch, int P, int logq, int logl) {
    extern __shared__ float2 lbuf[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int Q = 1 << logq, L = 1 << logl, PH = (P + 1) >> 1;
    const int ln = L * len;
    float2* const B0 = lbuf;
    float2* const B1 = lbuf + ln;             // (P > 1 only)
    float2* const twq = lbuf + (P == 1 ? 1 : 2) * ln;
    float2* const wp = twq + Q;
    const long plane = AXIS == 0 ? (long)count * pitch : (long)len * pitch;
    const int line0 = blockIdx.x * L;
    for (int i = tid; i < Q; i += kLineThreads) twq[i] = t.tw_q[i];
    for (int i = tid; i < P; i += kLineThreads) wp[i] = t.wp[i];
    const float* pre = u + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kLineThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        float2 v = make_float2(0.f, 0.f);
        if (line < count) {
            const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
            v = make_float2(pre[o], pre[o + plane]);
        }
        B0[l * len + t.slot[i]] = v;
    }
    __syncthreads();
    fft_inplace<false>(B0, B0, 1, L * P, logq, twq, tid);
    if (P == 1) {
        for (int e = tid; e < ln; e += kLineThreads) {
            const float kk1 = t.k1m[e & (Q - 1)];
            const float2 Y = B0[e];
            B0[e] = make_float2(-Y.y * kk1, Y.x * kk1);       // (0, k) * U, in place: the element is this thread's alone
        }
        __syncthreads();
    } else {
        for (int item = tid; item < (L * PH) << logq; item += kLineThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, k1 = lk - l * PH;
            const int base = l * len + r;
            float2 A[1], Bv[1];
            pdft_sums<1>(B0 + base, B0 + base, Q, P, k1, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (m == 1 && k1 == 0) break;
                const int kk = m == 0 ? k1 : P - k1;
                const float kk1 = t.k1m[(kk << logq) + r];
                const float2 Y = m == 0 ? plus_i(A[0], Bv[0]) : minus_i(A[0], Bv[0]);
                B1[base + (kk << logq)] = make_float2(-Y.y * kk1, Y.x * kk1);
            }
        }
        __syncthreads();
        for (int item = tid; item < (L * PH) << logq; item += kLineThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, s = lk - l * PH;
            const int base = l * len + r;
            float2 A[1], Bv[1];
            pdft_sums<1>(B1 + base, B1 + base, Q, P, s, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (m == 1 && s == 0) break;
                B0[base + ((m == 0 ? s : P - s) << logq)] = m == 0 ? minus_i(A[0], Bv[0]) : plus_i(A[0], Bv[0]);
            }
        }
        __syncthreads();
    }
    fft_inplace<true>(B0, B0, 1, L * P, logq, twq, tid);
    const float inv_n = 1.0f / (float)len;
    const float* pl = lam + (long)b * 2 * plane;
    float* po = out + ((long)b * 2 + AXIS) * plane;
    for (int e = tid; e < ln; e += kLineThreads) {
        const int l = AXIS == 0 ? e / len : e & (L - 1);
        const int i = AXIS == 0 ? e - l * len : e >> logl;
        const int line = line0 + l;
        if (line >= count) continue;
        const float2 z = cmul(t.b[i], B0[l * len + t.slot[i]]);
        const long o = AXIS == 0 ? (long)line * pitch + i : (long)i * pitch + line;
        po[o] = pl[o] * (z.x * inv_n) + pl[o + plane] * (z.y * inv_n);
    }
}

__global__ void k_line_bump(int* counter) { atomicAdd(counter, 1); }

int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Lines per block (a power of two) of a pass over `count` lines of `len` points in `nbuf` buffers: at most 16 -- the column pass then moves 64-byte row
// segments -- and at most kLineLdsLines of line buffers; fewer while the launch would not give every CU two blocks (small problems: latency, not
// throughput).  With four buffers: 16 lines up to len = 160, 8 up to 320, 4 up to 640, 2 up to 1280, then 1; halved while ceil(count / lines) * batch < 512.
int rect_lines(int len, int count, int nbuf, int batch) {
    int L = 16;
    while (L > 1 && (size_t)L * nbuf * len * sizeof(float2) > (size_t)kLineLdsLines) L >>= 1;
    while (L > 1 && (long)((count + L - 1) / L) * batch < 512) L >>= 1;
    return L;
}

// here, where an axis is built, and not at the first launch: a first call under stream capture is then nothing but launches
int line_kernels_lds_attr(hn_ctx* ctx) {
    for (const void* k : {reinterpret_cast<const void*>(k_spec_line<1, false>), reinterpret_cast<const void*>(k_spec_line<0, false>),
                          reinterpret_cast<const void*>(k_spec_line<0, false, const float*>), reinterpret_cast<const void*>(k_spec_line<1, true>),
                          reinterpret_cast<const void*>(k_spec_line<0, true>), reinterpret_cast<const void*>(k_spec_line<0, true, const float*>),
                          reinterpret_cast<const void*>(k_spec_line<1, false, const float*, const float*>),
                          reinterpret_cast<const void*>(k_spec_line<0, false, const float*, const float*>),
                          reinterpret_cast<const void*>(k_spec_line<1, true, const float*, const float*>),
                          reinterpret_cast<const void*>(k_spec_line<0, true, const float*, const float*>),
                          reinterpret_cast<const void*>(k_spec_line_d1<1>), reinterpret_cast<const void*>(k_spec_line_d1<0>)})
        HN_HIP(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kLineLdsAttr));
    return HN_OK;
}

// one axis' tables (P = 1: identity input map, the spectrum in bit-reversed order) and the kernels' dynamic-LDS attribute
int build_axis(hn_ctx* ctx, LineAxis& t, const AxisHost& ax, int P, int Q) {
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
    if ((rc = line_kernels_lds_attr(ctx)) != HN_OK) return rc;
    t.len = n;
    t.P = P;
    t.Q = Q;
    return HN_OK;
}

void free_axis(LineAxis& t) {
    for (void* p : {(void*)t.tw_q, (void*)t.wp, (void*)t.slot, (void*)t.k1m, (void*)t.k2m, (void*)t.a, (void*)t.b}) (void)hipFree(p);
    t = LineAxis{};
}

// The axes the domain's lines run on: a rectangle's two, or a square domain's one (both axes of an n x n domain are the same axis) for both.
struct LineDomain {
    const LineAxis *cols = nullptr, *rows = nullptr;   // cols: lines of length h (the y axis); rows: lines of length w (the x axis)
    int h = 0, w = 0;
};
bool line_domain(const hn_ctx* ctx, LineDomain* d) {
    if (const RectDomain* r = ctx->rect) *d = LineDomain{&r->cols, &r->rows, r->h, r->w};
    else if (const LineAxis* ax = ctx->sq_axis) *d = LineDomain{ax, ax, ax->len, ax->len};
    else return false;
    return d->cols->len != 0 && d->rows->len != 0;
}

// Both passes on `s`: the counter's bump, the column pass, the row pass.
//   forward           ksq nullptr: the Laplacian alone; ksq_im non-null (ksq too): the row pass with the complex pointwise term
//   adj               out = L^H(wf) + ksq wf [+ add]: three buffers, `add` on the column pass, no sum of squares; ksq_im non-null: the row pass with the
//                     conjugate pointwise term, conj(ksq + i ksq_im) wf
//   rho_grad          non-null (with ksq; ksq_im may be null): both passes of the variable-density operator, or with adj of its adjoint
int rect_launch(hn_ctx* ctx, const LineDomain& d, const float* wf, float* out, const float* ksq, const float* ksq_im, const float* src, int src_batch,
                int batch, float* sumsq, hipStream_t s, int* it_counter, int sumsq_stride, bool adj = false, const float* add = nullptr,
                const float* rho_grad = nullptr) {
    const LineAxis &cols = *d.cols, &rows = *d.rows;
    const int h = d.h, w = d.w;
    if (adj && (ksq == nullptr || src != nullptr || sumsq != nullptr || it_counter != nullptr))
        return fail(ctx, HN_ERR_ARG, "internal: the adjoint LDS-line kernels (%d x %d) take k_sq and neither a source, a sum of squares nor a counter", h, w);
    if (rho_grad != nullptr && ksq == nullptr)
        return fail(ctx, HN_ERR_ARG, "internal: the variable-density LDS-line kernels (%d x %d) take k_sq", h, w);
    const bool resid = ksq != nullptr;
    const long src_sb = src_batch == 1 ? 0 : 2L * h * w;
    const int nbuf_c = adj || cols.P == 1 ? 3 : 4, nbuf_r = adj || rows.P == 1 ? 3 : 4;
    const int Lc = rect_lines(h, w, nbuf_c, batch), Lr = rect_lines(w, h, nbuf_r, batch);
    const size_t lds_c = ((size_t)Lc * nbuf_c * h + cols.Q + cols.P) * sizeof(float2), lds_r = ((size_t)Lr * nbuf_r * w + rows.Q + rows.P) * sizeof(float2);
    if (lds_c > (size_t)kLineLdsAttr || lds_r > (size_t)kLineLdsAttr)
        return fail(ctx, HN_ERR_ARG, "internal: LDS-line spectral kernel needs %zu / %zu bytes of LDS at %d x %d", lds_c, lds_r, h, w);
    const LineTabs tc{cols.tw_q, cols.wp, cols.k1m, cols.k2m, cols.a, cols.b, cols.slot};
    const LineTabs tr{rows.tw_q, rows.wp, rows.k1m, rows.k2m, rows.a, rows.b, rows.slot};
    const dim3 grid_c((w + Lc - 1) / Lc, batch), grid_r((h + Lr - 1) / Lr, batch), block(kLineThreads);
    const int logq_c = ilog2(cols.Q), logl_c = ilog2(Lc), logq_r = ilog2(rows.Q), logl_r = ilog2(Lr), rflags = 1 | (resid ? 2 : 0);
    std::optional<ProfScope> pair;   // both passes under one event pair (when selected); the adjoint has none on any route
    if (!adj) pair.emplace(ctx, KID_SPEC_PAIR, s);
    if (it_counter != nullptr) hipLaunchKernelGGL(k_line_bump, dim3(1), dim3(1), 0, s, it_counter);
    {
        ProfScope ps(ctx, KID_SPEC_COLS, s);
        if (adj && rho_grad != nullptr)
            hipLaunchKernelGGL((k_spec_line<1, true, const float*, const float*>), grid_c, block, lds_c, s, wf, out, nullptr, nullptr, 0L, tc, h, w, w, cols.P,
                               logq_c, logl_c, 0, nullptr, nullptr, 0, nullptr, rho_grad, add);
        else if (adj)
            hipLaunchKernelGGL((k_spec_line<1, true>), grid_c, block, lds_c, s, wf, out, nullptr, nullptr, 0L, tc, h, w, w, cols.P, logq_c, logl_c, 0, nullptr,
                               nullptr, 0, add);
        else if (rho_grad != nullptr)
            hipLaunchKernelGGL((k_spec_line<1, false, const float*, const float*>), grid_c, block, lds_c, s, wf, out, nullptr, nullptr, 0L, tc, h, w, w, cols.P,
                               logq_c, logl_c, 0, nullptr, nullptr, 0, nullptr, rho_grad, nullptr);
        else
            hipLaunchKernelGGL((k_spec_line<1, false>), grid_c, block, lds_c, s, wf, out, nullptr, nullptr, 0L, tc, h, w, w, cols.P, logq_c, logl_c, 0, nullptr,
                               nullptr, 0, nullptr);
    }
    {
        ProfScope ps(ctx, KID_SPEC_ROWS, s);
        if (adj && rho_grad != nullptr)
            hipLaunchKernelGGL((k_spec_line<0, true, const float*, const float*>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P,
                               logq_r, logl_r, rflags, sumsq, it_counter, sumsq_stride, ksq_im, rho_grad, nullptr);
        else if (adj && ksq_im != nullptr)
            hipLaunchKernelGGL((k_spec_line<0, true, const float*>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P, logq_r, logl_r,
                               rflags, sumsq, it_counter, sumsq_stride, ksq_im, nullptr);
        else if (rho_grad != nullptr)
            hipLaunchKernelGGL((k_spec_line<0, false, const float*, const float*>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P,
                               logq_r, logl_r, rflags, sumsq, it_counter, sumsq_stride, ksq_im, rho_grad, nullptr);
        else if (adj)
            hipLaunchKernelGGL((k_spec_line<0, true>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P, logq_r, logl_r, rflags, sumsq,
                               it_counter, sumsq_stride, nullptr);
        else if (ksq_im != nullptr)
            hipLaunchKernelGGL((k_spec_line<0, false, const float*>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P, logq_r, logl_r,
                               rflags, sumsq, it_counter, sumsq_stride, ksq_im, nullptr);
        else
            hipLaunchKernelGGL((k_spec_line<0, false>), grid_r, block, lds_r, s, wf, out, ksq, src, src_sb, tr, w, h, w, rows.P, logq_r, logl_r, rflags, sumsq,
                               it_counter, sumsq_stride, nullptr);
    }
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

// dJ/dq of both axes (k_spec_line_d1): the column pass writes plane 1 of `out`, the row pass plane 0; the two are independent
int rect_launch_d1(hn_ctx* ctx, const LineDomain& d, const float* u, const float* lam, float* out, int batch, hipStream_t s) {
    const LineAxis &cols = *d.cols, &rows = *d.rows;
    const int h = d.h, w = d.w;
    const int nbuf_c = cols.P == 1 ? 1 : 2, nbuf_r = rows.P == 1 ? 1 : 2;
    const int Lc = rect_lines(h, w, nbuf_c, batch), Lr = rect_lines(w, h, nbuf_r, batch);
    const size_t lds_c = ((size_t)Lc * nbuf_c * h + cols.Q + cols.P) * sizeof(float2), lds_r = ((size_t)Lr * nbuf_r * w + rows.Q + rows.P) * sizeof(float2);
    if (lds_c > (size_t)kLineLdsAttr || lds_r > (size_t)kLineLdsAttr)
        return fail(ctx, HN_ERR_ARG, "internal: LDS-line first-derivative kernel needs %zu / %zu bytes of LDS at %d x %d", lds_c, lds_r, h, w);
    const LineTabs tc{cols.tw_q, cols.wp, cols.k1m, cols.k2m, cols.a, cols.b, cols.slot};
    const LineTabs tr{rows.tw_q, rows.wp, rows.k1m, rows.k2m, rows.a, rows.b, rows.slot};
    const dim3 grid_c((w + Lc - 1) / Lc, batch), grid_r((h + Lr - 1) / Lr, batch), block(kLineThreads);
    hipLaunchKernelGGL((k_spec_line_d1<1>), grid_c, block, lds_c, s, u, lam, out, tc, h, w, w, cols.P, ilog2(cols.Q), ilog2(Lc));
    hipLaunchKernelGGL((k_spec_line_d1<0>), grid_r, block, lds_r, s, u, lam, out, tr, w, h, w, rows.P, ilog2(rows.Q), ilog2(Lr));
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
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
    ctx->rect = r;   // (a failure below leaves a domain whose launches are refused: line_domain checks the tables)
    r->h = h;
    r->w = w;
    r->pml = pml;
    r->sigma_max = sigma_max;
    r->k = k;
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
    return HN_OK;
}

// ---- a square domain's one axis: ctx->sq_axis, the tables of ctx->tab's (n, pml, sigma_max, k) ----
// Built by spec_build where the domain goes on the mixed route (tab.mixed), else by the first lossy call (spec_lossy_reserve); freed by spec_free, with tab
// and nowhere else: it does not outlive the domain it was built for, and does not go while tab.mixed still points the lossless operator at it.
void spec_sq_axis_free(hn_ctx* ctx) {
    if (ctx->sq_axis == nullptr) return;
    free_axis(*ctx->sq_axis);
    delete ctx->sq_axis;
    ctx->sq_axis = nullptr;
}

int spec_sq_axis_build(hn_ctx* ctx) {
    const SpecTables& t = ctx->tab;
    int P = 0, Q = 0;
    if (!spec_rect_factor(t.n, &P, &Q)) return fail(ctx, HN_ERR_ARG, "internal: no factorisation of the domain size %d", t.n);
    spec_sq_axis_free(ctx);
    LineAxis* ax = new (std::nothrow) LineAxis();
    if (ax == nullptr) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    if (const int rc = build_axis(ctx, *ax, spec_axis_host(t.n, t.pml, t.sigma_max, t.k), P, Q); rc != HN_OK) {
        free_axis(*ax);
        delete ax;
        return rc;
    }
    ctx->sq_axis = ax;
    return HN_OK;
}

int spec_line_apply(hn_ctx* ctx, const float* wf, float* out, const float* ksq, const float* src, int src_batch, int batch, float* sumsq,
                    hipStream_t s, int* it_counter, int sumsq_stride) {
    LineDomain d;
    if (!line_domain(ctx, &d)) return fail(ctx, HN_ERR_STATE, "hn_set_domain_rect has not been called");
    if (batch <= 0) return HN_OK;
    return rect_launch(ctx, d, wf, out, ksq, nullptr, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride);
}

int spec_line_adjoint(hn_ctx* ctx, const float* g, float* out, const float* ksq, const float* add, int batch, hipStream_t s) {
    LineDomain d;
    if (ctx->rect != nullptr || !line_domain(ctx, &d)) return fail(ctx, HN_ERR_ARG, "internal: the adjoint LDS-line kernels run on a square domain's mixed route alone");
    return rect_launch(ctx, d, g, out, ksq, nullptr, nullptr, 1, batch, nullptr, s, nullptr, 0, true, add);
}

// ---- the lossy operator, res = L(u) + (ksq + i ksq_im) u - src, and the variable-density one, which subtracts b_x q_x d_x u + b_y q_y d_y u: one set of tables ----
// A rectangular domain has its tables, and so has a square one on the mixed route.  Any other square domain gets its axis here, at the first lossy call --
// never under stream capture; ctx->rect stays null: the domain stays square.
int spec_lossy_reserve(hn_ctx* ctx, const char* who, hipStream_t s) {
    if (ctx->rect != nullptr || ctx->sq_axis != nullptr) return HN_OK;
    if (ctx->tab.n == 0) return fail(ctx, HN_ERR_STATE, "%s: hn_set_domain has not been called", who);
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "%s: the tables of the lossy operator on a square domain are built by the first lossy call, which must not be under "
                    "stream capture", who);
    return spec_sq_axis_build(ctx);
}

// the operator of medium m (hn_internal.h): a lossless one is spec_apply's, with its own choice of route; the other two run here, on either kind of domain
int spec_forward(hn_ctx* ctx, const char* who, const Medium& m, const float* wf, float* out, const float* src, int src_batch, int batch, float* sumsq,
                 hipStream_t s, int* it_counter, int sumsq_stride) {
    const Medium::Kind kind = m.kind();
    if (kind == Medium::Kind::Lossless) return spec_apply(ctx, wf, out, m.k_sq, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride);
    if (m.k_sq == nullptr)
        return kind == Medium::Kind::Density ? fail(ctx, HN_ERR_ARG, "internal: %s: the variable-density operator needs k_sq and rho_grad", who)
                                             : fail(ctx, HN_ERR_ARG, "internal: %s: the lossy operator needs both planes of k_sq", who);
    if (const int rc = spec_lossy_reserve(ctx, who, s); rc != HN_OK) return rc;
    if (batch <= 0) return HN_OK;
    LineDomain d;
    if (!line_domain(ctx, &d)) return fail(ctx, HN_ERR_STATE, "hn_set_domain_rect has not been called");
    return rect_launch(ctx, d, wf, out, m.k_sq, m.k_sq_im, src, src_batch, batch, sumsq, s, it_counter, sumsq_stride, false, nullptr, m.rho_grad);
}

// out = A^H g [+ add]: spec_adjoint for a lossless medium; for a lossy one L^H(g) + (ksq - i ksq_im) g on the tables of spec_forward, and for a
// variable-density one that minus D_x^H(conj(b_x) q_x g) + D_y^H(conj(b_y) q_y g) (k_sq_im may be null)
int spec_backward(hn_ctx* ctx, const char* who, const Medium& m, const float* g, float* out, const float* add, int batch, hipStream_t s) {
    const Medium::Kind kind = m.kind();
    if (kind == Medium::Kind::Lossless) return spec_adjoint(ctx, g, out, m.k_sq, add, batch, s);
    if (m.k_sq == nullptr)
        return kind == Medium::Kind::Density ? fail(ctx, HN_ERR_ARG, "internal: %s: the variable-density operator needs k_sq and rho_grad", who)
                                             : fail(ctx, HN_ERR_ARG, "internal: %s: the lossy operator needs both planes of k_sq", who);
    if (g == out) return fail(ctx, HN_ERR_ARG, "%s: input and output must not alias", who);
    if (const int rc = spec_lossy_reserve(ctx, who, s); rc != HN_OK) return rc;
    if (batch <= 0) return HN_OK;
    LineDomain d;
    if (!line_domain(ctx, &d)) return fail(ctx, HN_ERR_STATE, "hn_set_domain_rect has not been called");
    return rect_launch(ctx, d, g, out, m.k_sq, m.k_sq_im, nullptr, 1, batch, nullptr, s, nullptr, 0, true, add, m.rho_grad);
}

int spec_density_grad(hn_ctx* ctx, const char* who, const float* lam, const float* u, float* g_rho_grad, int batch, hipStream_t s) {
    if (batch <= 0) return HN_OK;
    LineDomain d;
    if (!line_domain(ctx, &d)) return fail(ctx, HN_ERR_STATE, "%s: the line tables have not been built (spec_lossy_reserve)", who);
    return rect_launch_d1(ctx, d, u, lam, g_rho_grad, batch, s);
}

int rect_unsupported(hn_ctx* ctx, const char* who) {
    return fail(ctx, HN_ERR_UNSUPPORTED, "%s: not implemented on a rectangular domain (%d x %d, hn_set_domain_rect): the rectangular path covers hn_reserve, "
                "hn_get_sigmas, hn_laplacian, hn_residual, hn_rmse, hn_unet and hn_step in the fp32 precision modes", who, ctx->rect ? ctx->rect->h : 0,
                ctx->rect ? ctx->rect->w : 0);
}

}  // namespace hn
