// hn_f64_fft.hip -- the float64 Helmholtz operator of hn_f64.hip by FFT (HN_OPT_F64_FFT 1; always for hn_residual_f64_lossy): two line passes in the
// algorithm of k_spec_line (hn_spectral_line.hip; read its header comment), in double, on an h x w field (h == w: a square domain).
//   column pass   w lines of length h along the first spatial axis:   mid = ay . D1y u + by . D2y u
//   row pass      h lines of length w along the second:               out = mid + ax . D1x u + bx . D2x u [+ k_sq . u - src], one sum of squares per line
//   lossy row pass (absorbing media, LOSSY): the value above formed exactly as above, then re -= k_sq_im . u_im and im += k_sq_im . u_re as two further
//                 operations of their own -- with k_sq_im == 0 the lossless bits on finite inputs
// Each axis has its own tables (a square domain: one set for both), its own lines per block, buffer count and dynamic LDS, and is normalised by its own length.
// Every legal length n = P * Q, P odd in [1, 127], Q = 2^k in [16, 2048] (spec_rect_factor).  A line lives in LDS as [P][Q] double2 (Good-Thomas input map): in-place
// Q-point transforms (natural in, bit-reversed out), a direct P-point DFT across them, the derivative multipliers i k and -k^2 in the order the spectrum is met,
// and the inverses.  P = 1 has no P-point DFT and needs three line buffers instead of four.  The operator values are k_helm_f64's: the fp32 wavenumber grid
// up-cast, its fp32 square up-cast, the fp32-rounded PML coefficients up-cast.  The Nyquist bin keeps k = -pi as the reference does; as a multiplier on the
// spectrum it needs no term of its own (the dense form's Im g1 is this bin's inverse transform).  Twiddles come from the host in double; 1 / n is applied once,
// to the finished line.
//
// LDS (16 bytes per point): 2048: 3 x 32 KiB + 32 KiB of twiddles = 128 KiB; 2032 = 127 * 16: 4 x 31.75 KiB + 2.2 KiB = 129.2 KiB (the largest);
// 1536 = 3 * 512: 96 KiB + 8 KiB.  A workgroup may declare 160 KiB, so every legal length fits and the long ones run one line and one block per CU; short
// lines run up to 16 per block inside an 80 KiB budget (two blocks per CU), fewer while the launch would not give every CU two blocks (the rule of rect_lines).
// All 512 threads of a block work through the items of all its lines between block barriers; which thread computes an element does not change the element's
// arithmetic.  The row pass leaves the squares of a line's results in a line buffer that is free by then, and ONE wave adds a line in a fixed order (lane j:
// elements j, j + 64, ... in turn, then a fixed butterfly): a line's partial sum, and with it a sample's rmse (k_rmse_f64 adds the h partials in its fixed
// order), depends neither on the lines per block nor on the batch.
// Lines are independent: no flags, no cross-workgroup waits, no atomics.  Plain C++ on v_fma_f64; the caller's tensors are read and written as scalar doubles
// (8-byte alignment is all they need).
#include <cmath>
#include <new>
#include <vector>

#include "hn_internal.h"

namespace hn {

// what the first FFT-route call on a domain builds (f64_fft_reserve) and hn_set_domain / hn_set_domain_rect / hn_destroy free (f64_fft_free)
struct F64Axis {
    int n = 0, P = 0, Q = 0;    // lines of length n = P * Q
    char* tabs = nullptr;       // one allocation: tw_q [Q], wp [P], a [n], b [n] (double2), k1m [n], k2m [n] (double), slot [n] (int)
};
struct F64Fft {
    int h = 0, w = 0;
    F64Axis cols, rows;         // cols: lines of length h (the y axis); rows: lines of length w (the x axis).  h == w: rows.tabs == cols.tabs, one allocation
    double* part = nullptr;     // [part_cap]: one sum of squares per row and sample, [batch][h]
    long part_cap = 0;
    double* mid = nullptr;      // [mid_cap]: the column pass's result [batch, 2, h, w] of a call that returns no field (res == NULL)
    long mid_cap = 0;
};

namespace {

constexpr int kThreads = 512;
constexpr int kLdsAttr = 160 * 1024;    // dynamic LDS the two kernels may ask for: all a workgroup can declare on this chip
constexpr int kLdsLines = 80 * 1024;    // budget of a block's line buffers while more than one line shares a block: two blocks per CU

__device__ __forceinline__ double2 cadd(double2 x, double2 y) { return make_double2(x.x + y.x, x.y + y.y); }
__device__ __forceinline__ double2 csub(double2 x, double2 y) { return make_double2(x.x - y.x, x.y - y.y); }
__device__ __forceinline__ double2 cmul(double2 x, double2 y) { return make_double2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x); }
__device__ __forceinline__ double2 cmulc(double2 x, double2 y) { return make_double2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y); }   // x * conj(y)
__device__ __forceinline__ double2 plus_i(double2 a, double2 b) { return make_double2(a.x - b.y, a.y + b.x); }    // a + i b
__device__ __forceinline__ double2 minus_i(double2 a, double2 b) { return make_double2(a.x + b.y, a.y - b.x); }   // a - i b

// Q-point transforms in place on `nseq` contiguous sequences of each of `nbuf` (1 or 2) buffers.  !INV: decimation in frequency, natural in, bit-reversed
// out.  INV: the transposed flow graph with conjugate twiddles, bit-reversed in, natural out, unnormalised.  One item = the four elements
// {a, a + h/2, a + h, a + 3h/2} that two consecutive radix-2 stages (spans 2h and h) keep among themselves; an odd log2 Q leaves the span-2 stage (twiddle 1)
// on its own.  Ends with a barrier; the caller provides the one in front.
template <bool INV>
__device__ __forceinline__ void fft_inplace(double2* b0, double2* b1, int nbuf, int nseq, int logq, const double2* twq, int tid) {
    const int Q = 1 << logq;
    const int per4 = nseq << (logq - 2), per2 = nseq << (logq - 1);
    auto pairs = [&]() {
        for (int item = tid; item < nbuf * per2; item += kThreads) {
            double2* p = (item < per2 ? b0 + 2 * item : b1 + 2 * (item - per2));
            const double2 x0 = p[0], x1 = p[1];
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
        for (int item = tid; item < nbuf * per4; item += kThreads) {
            const int it = item < per4 ? item : item - per4;
            const int seq = it >> (logq - 2), q = it & ((Q >> 2) - 1);
            const int off = q & (hh - 1), blk = q >> (lh - 1);
            double2* p = (item < per4 ? b0 : b1) + (seq << logq) + (blk << (lh + 1)) + off;
            const double2 wa = twq[off << (logq - lh - 1)];          // W_2h^off
            const double2 wb = twq[(off + hh) << (logq - lh - 1)];   // W_2h^(off + h/2)
            const double2 wc = twq[off << (logq - lh)];              // W_h^off
            const double2 x0 = p[0], x1 = p[hh], x2 = p[h], x3 = p[h + hh];
            if (!INV) {
                const double2 y0 = cadd(x0, x2), y2 = cmul(csub(x0, x2), wa);
                const double2 y1 = cadd(x1, x3), y3 = cmul(csub(x1, x3), wb);
                p[0] = cadd(y0, y1);
                p[hh] = cmul(csub(y0, y1), wc);
                p[h] = cadd(y2, y3);
                p[h + hh] = cmul(csub(y2, y3), wc);
            } else {
                const double2 t1 = cmulc(x1, wc), t3 = cmulc(x3, wc);
                const double2 y0 = cadd(x0, t1), y1 = csub(x0, t1), y2 = cadd(x2, t3), y3 = csub(x2, t3);
                const double2 u2 = cmulc(y2, wa), u3 = cmulc(y3, wb);
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

// A[i] = sum_s x_i[s Q] Re w_s, B[i] = sum_s x_i[s Q] Im w_s over the P sub-sequences, w_s = wp[(s kk) mod P], for NIN inputs that share the twiddle
// reads; two accumulator chains, the odd term last.  With wp = exp(-2 pi i m / P): the forward DFT's outputs kk and P - kk are A + i B and A - i B, the
// inverse DFT's A - i B and A + i B.
template <int NIN>
__device__ __forceinline__ void pdft_sums(const double2* in0, const double2* in1, int Q, int P, int kk, const double2* wp, double2 (&A)[NIN],
                                          double2 (&B)[NIN]) {
    double2 a0[NIN], b0[NIN], a1[NIN], b1[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) a0[i] = b0[i] = a1[i] = b1[i] = make_double2(0.0, 0.0);
    int idx = 0, s = 0;
    for (; s + 1 < P; s += 2) {
        const double2 w0 = wp[idx];
        idx += kk;
        if (idx >= P) idx -= P;
        const double2 w1 = wp[idx];
        idx += kk;
        if (idx >= P) idx -= P;
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const double2* in = i == 0 ? in0 : in1;
            const double2 x0 = in[s * Q], x1 = in[(s + 1) * Q];
            a0[i].x += x0.x * w0.x; a0[i].y += x0.y * w0.x;
            b0[i].x += x0.x * w0.y; b0[i].y += x0.y * w0.y;
            a1[i].x += x1.x * w1.x; a1[i].y += x1.y * w1.x;
            b1[i].x += x1.x * w1.y; b1[i].y += x1.y * w1.y;
        }
    }
    const double2 w0 = wp[idx];   // P is odd: one term left
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const double2 x0 = (i == 0 ? in0 : in1)[s * Q];
        a0[i].x += x0.x * w0.x; a0[i].y += x0.y * w0.x;
        b0[i].x += x0.x * w0.y; b0[i].y += x0.y * w0.y;
        A[i] = cadd(a0[i], a1[i]);
        B[i] = cadd(b0[i], b1[i]);
    }
}

struct Tabs {
    const double2* tw_q;   // exp(-2 pi i m / Q)
    const double2* wp;     // exp(-2 pi i m / P)
    const double2* a;      // PML coefficients, natural order
    const double2* b;
    const double* k1m;     // [P][Q]: k at (k1, position r)
    const double* k2m;     // -k^2 likewise
    const int* slot;       // [n]: n1 * Q + n2 of element i
};

// One kernel for both axes of the h x w field; n = the line's length (AXIS 1: h, AXIS 0: w), t, P, logq that axis' tables and factors; L = 1 << logl lines
// per block (L divides 16 and with it the number of lines, a multiple of 16: no block has lines past the last one).
//   AXIS 1: along y (column pass: line c is column c; the block's L adjacent columns are loaded and stored as row segments of L doubles); dst = the pass's result
//   AXIS 0: along x (row pass: line r is row r): dst (nullable) = mid + the pass's result [+ k_sq u - src with RESID]; part (nullable): [batch][h] sums of
//           squares of a line.  mid may be dst: every element is read and then written by one thread.
//   LOSSY (AXIS 0 with resid): ksq_im, the imaginary part of k_sq, applied to the finished lossless value.
// Dynamic LDS: (P == 1 ? 3 : 4) buffers of L * n double2, then the Q and P twiddles.
template <int AXIS, bool LOSSY>
__global__ __launch_bounds__(kThreads) void k_f64_fft(const double* __restrict__ wf, const double* mid, double* dst, const double* ksq, const double* ksq_im,
                                                       const double* src, long src_sb, Tabs t, int h, int w, int P, int logq, int logl, int resid,
                                                       double* __restrict__ part) {
    extern __shared__ double2 fbuf[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int n = AXIS == 0 ? w : h;
    const int Q = 1 << logq, L = 1 << logl, PH = (P + 1) >> 1;
    const int ln = L * n;                 // double2 per buffer
    double2* const B0 = fbuf;
    double2* const B1 = fbuf + ln;
    double2* const B2 = fbuf + 2 * ln;
    double2* const B3 = fbuf + 3 * ln;    // (P > 1 only)
    double2* const twq = fbuf + (P == 1 ? 3 : 4) * ln;
    double2* const wp = twq + Q;
    const long plane = (long)h * w;
    const int line0 = blockIdx.x * L;
    for (int i = tid; i < Q; i += kThreads) twq[i] = t.tw_q[i];
    for (int i = tid; i < P; i += kThreads) wp[i] = t.wp[i];
    // ---- 1: load
    const double* pre = wf + (long)b * 2 * plane;
    for (int e = tid; e < ln; e += kThreads) {
        const int l = AXIS == 0 ? e / n : e & (L - 1);
        const int i = AXIS == 0 ? e - l * n : e >> logl;
        const long o = AXIS == 0 ? (long)(line0 + l) * w + i : (long)i * w + line0 + l;
        B0[l * n + t.slot[i]] = make_double2(pre[o], pre[o + plane]);
    }
    __syncthreads();
    // ---- 2: Q-point transforms of the L * P sub-sequences
    fft_inplace<false>(B0, B1, 1, L * P, logq, twq, tid);
    // the buffers the inverse transforms run on and the results are read from: first- and second-derivative spectrum
    double2* const D1 = P == 1 ? B1 : B0;
    double2* const D2 = P == 1 ? B2 : B3;
    if (P == 1) {
        // ---- 3 (P = 1): derivative multipliers in place of the P-point DFT pair
        for (int e = tid; e < ln; e += kThreads) {
            const int r = e & (Q - 1);
            const double kk1 = t.k1m[r], kk2 = t.k2m[r];
            const double2 Y = B0[e];
            B1[e] = make_double2(-Y.y * kk1, Y.x * kk1);   // (0, k) * U
            B2[e] = make_double2(kk2 * Y.x, kk2 * Y.y);    // (-k^2, 0) * U
        }
        __syncthreads();
    } else {
        // ---- 3: direct P-point DFT, derivative multipliers
        for (int item = tid; item < (L * PH) << logq; item += kThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, k1 = lk - l * PH;
            const int base = l * n + r;
            double2 A[1], Bv[1];
            pdft_sums<1>(B0 + base, B0 + base, Q, P, k1, wp, A, Bv);
#pragma unroll
            for (int m = 0; m < 2; ++m) {            // output k1, then its mirror P - k1
                if (m == 1 && k1 == 0) break;
                const int kk = m == 0 ? k1 : P - k1;
                const double kk1 = t.k1m[(kk << logq) + r], kk2 = t.k2m[(kk << logq) + r];
                const double2 Y = m == 0 ? plus_i(A[0], Bv[0]) : minus_i(A[0], Bv[0]);
                const int o = base + (kk << logq);
                B1[o] = make_double2(-Y.y * kk1, Y.x * kk1);
                B2[o] = make_double2(kk2 * Y.x, kk2 * Y.y);
            }
        }
        __syncthreads();
        // ---- 4: inverse P-point DFT of both
        for (int item = tid; item < (L * PH) << logq; item += kThreads) {
            const int r = item & (Q - 1), lk = item >> logq;
            const int l = lk / PH, s = lk - l * PH;
            const int base = l * n + r;
            double2 A[2], Bv[2];
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
    // ---- 6: PML coefficients, the pass's other terms, store; the squares go to a buffer nothing reads any more
    double* const sq = reinterpret_cast<double*>(P == 1 ? B0 : B1);
    const double inv_n = 1.0 / (double)n;
    double* po = dst != nullptr ? dst + (long)b * 2 * plane : nullptr;
    for (int e = tid; e < ln; e += kThreads) {
        const int l = AXIS == 0 ? e / n : e & (L - 1);
        const int i = AXIS == 0 ? e - l * n : e >> logl;
        const int sl = l * n + t.slot[i];
        const double2 p = cmul(t.a[i], D1[sl]), r = cmul(t.b[i], D2[sl]);
        double re = (p.x + r.x) * inv_n;
        double im = (p.y + r.y) * inv_n;
        const long o = AXIS == 0 ? (long)(line0 + l) * w + i : (long)i * w + line0 + l;
        if (AXIS == 0) {
            const double* pm = mid + (long)b * 2 * plane;
            re += pm[o];
            im += pm[o + plane];
            if (resid) {
                const double kq = ksq[(long)b * plane + o];
                const double* ps = src + (long)b * src_sb + o;
                re += kq * pre[o] - ps[0];          // the line itself again (an L2 hit) instead of a copy held through the transforms
                im += kq * pre[o + plane] - ps[plane];
                if constexpr (LOSSY) {                  // (k_sq + i k_sq_im) u: the imaginary part's share, after the lossless value is complete
                    const double ki = ksq_im[(long)b * plane + o];
                    const double lre = ki * pre[o + plane], lim = ki * pre[o];
                    re = __dsub_rn(re, lre);
                    im = __dadd_rn(im, lim);
                }
            }
            sq[l * n + i] = re * re + im * im;
        }
        if (po != nullptr) {
            po[o] = re;
            po[o + plane] = im;
        }
    }
    if (AXIS == 0 && part != nullptr) {
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;
        for (int l = wave; l < L; l += kThreads / 64) {
            double s = 0.0;
            for (int i = lane; i < n; i += 64) s += sq[l * n + i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) part[(long)b * h + line0 + l] = s;
        }
    }
}

int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Lines per block (a power of two), the rule of rect_lines with 16-byte points: at most 16 -- the column pass then moves 128-byte row segments -- and at most
// kLdsLines of line buffers; fewer while the launch would not give every CU two blocks.  One line per block may take more than kLdsLines (the long lines).
// Per pass: `lines` lines of length n (a square domain: lines == n in both).
int lines_per_block(int n, int lines, int nbuf, int batch) {
    int L = 16;
    while (L > 1 && (size_t)L * nbuf * n * sizeof(double2) > (size_t)kLdsLines) L >>= 1;
    while (L > 1 && (long)(lines / L) * batch < 512) L >>= 1;
    return L;
}

size_t lds_bytes(int n, int P, int Q, int L) { return ((size_t)L * (P == 1 ? 3 : 4) * n + Q + P) * sizeof(double2); }

Tabs tabs_of(const F64Axis& f) {
    const int n = f.n;
    const double2* c = reinterpret_cast<const double2*>(f.tabs);
    const double* d = reinterpret_cast<const double*>(c + f.Q + f.P + 2 * (size_t)n);
    return Tabs{c, c + f.Q, c + f.Q + f.P, c + f.Q + f.P + n, d, d + n, reinterpret_cast<const int*>(d + 2 * (size_t)n)};
}

// the tables of build_axis (hn_spectral_line.hip) in double: the twiddles computed in double, the operator values up-cast from what the reference holds in fp32
int build_tables(hn_ctx* ctx, F64Axis& f, int n, int P, int Q) {
    // what the domain was set with: a square one keeps it in tab, a rectangular one in rect
    const int pml = ctx->rect ? ctx->rect->pml : ctx->tab.pml;
    const double sigma_max = ctx->rect ? ctx->rect->sigma_max : ctx->tab.sigma_max, k = ctx->rect ? ctx->rect->k : ctx->tab.k;
    const AxisHost ax = spec_axis_host(n, pml, sigma_max, k);
    const int logq = ilog2(Q);
    const double pi = 3.14159265358979323846;
    int qinv = 0, pinv = 1;
    if (P > 1) { qinv = 1; while ((Q * qinv) % P != 1) ++qinv; }
    while ((P * pinv) % Q != 1) ++pinv;
    const size_t n_c = (size_t)Q + P + 2 * (size_t)n, bytes = n_c * sizeof(double2) + 2 * (size_t)n * sizeof(double) + (size_t)n * sizeof(int);
    std::vector<char> h(bytes);
    double2* c = reinterpret_cast<double2*>(h.data());
    double* d = reinterpret_cast<double*>(c + n_c);
    int* slot = reinterpret_cast<int*>(d + 2 * (size_t)n);
    for (int m = 0; m < Q; ++m) c[m] = make_double2(std::cos(2.0 * pi * m / Q), -std::sin(2.0 * pi * m / Q));
    for (int m = 0; m < P; ++m) c[Q + m] = make_double2(std::cos(2.0 * pi * m / P), -std::sin(2.0 * pi * m / P));
    for (int i = 0; i < n; ++i) {
        c[Q + P + i] = make_double2((double)ax.fa[i].x, (double)ax.fa[i].y);
        c[Q + P + n + i] = make_double2((double)ax.fb[i].x, (double)ax.fb[i].y);
        slot[i] = (((i % P) * qinv) % P) * Q + ((i % Q) * pinv) % Q;   // i = (Q n1 + P n2) mod n
    }
    for (int a1 = 0; a1 < P; ++a1)
        for (int r = 0; r < Q; ++r) {
            int a2 = 0;                                    // position r of an in-place transform holds k2 = bitrev(r)
            for (int bit = 0; bit < logq; ++bit) a2 |= ((r >> bit) & 1) << (logq - 1 - bit);
            const int kk = (int)(((long)Q * qinv * a1 + (long)P * pinv * a2) % n);   // Good-Thomas output map
            d[(size_t)a1 * Q + r] = (double)ax.k1[kk];
            d[(size_t)n + (size_t)a1 * Q + r] = (double)ax.k2[kk];
        }
    // here and not at the first launch: the launches themselves are then capturable
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_f64_fft<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_f64_fft<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsAttr));
    HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_f64_fft<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsAttr));
    char* dev = nullptr;
    HN_HIP(ctx, hipMalloc((void**)&dev, bytes));
    if (hipError_t e = hipMemcpy(dev, h.data(), bytes, hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(dev);
        return fail(ctx, HN_ERR_HIP, "upload of the float64 FFT tables failed: %s", hipGetErrorString(e));
    }
    f.tabs = dev;
    f.n = n;
    f.P = P;
    f.Q = Q;
    return HN_OK;
}

int grow(hn_ctx* ctx, double** p, long* cap, long needed) {
    if (needed <= *cap) return HN_OK;
    (void)hipFree(*p);   // (waits for the launches that still use it)
    *p = nullptr;
    *cap = 0;
    HN_HIP(ctx, hipMalloc((void**)p, (size_t)needed * sizeof(double)));
    *cap = needed;
    return HN_OK;
}

}  // namespace

void f64_fft_free(hn_ctx* ctx) {
    if (ctx->f64fft == nullptr) return;
    F64Fft& f = *ctx->f64fft;
    if (f.rows.tabs != f.cols.tabs) (void)hipFree(f.rows.tabs);   // (a square domain's one allocation serves both axes)
    for (void* p : {(void*)f.cols.tabs, (void*)f.part, (void*)f.mid}) (void)hipFree(p);
    delete ctx->f64fft;
    ctx->f64fft = nullptr;
}

int f64_fft_reserve(hn_ctx* ctx, int batch, bool want_rmse, bool want_out, hipStream_t s) {
    const int h = ctx->geo.h, w = ctx->geo.w;
    const long part_needed = want_rmse ? (long)batch * h : 0, mid_needed = want_out ? 0 : (long)batch * 2 * h * w;
    F64Fft* f = ctx->f64fft;
    if (f != nullptr && f->cols.tabs != nullptr && f->rows.tabs != nullptr && part_needed <= f->part_cap && mid_needed <= f->mid_cap) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "the float64 FFT tables of this domain (or a larger batch's partial sums or intermediate field) are built by the first call, which must not be under stream capture");
    if (f == nullptr) {
        f = new (std::nothrow) F64Fft();
        if (f == nullptr) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
        ctx->f64fft = f;
    }
    f->h = h;
    f->w = w;
    for (F64Axis* ax : {&f->cols, &f->rows}) {
        if (ax->tabs != nullptr) continue;
        const int n = ax == &f->cols ? h : w;
        if (ax == &f->rows && h == w) { f->rows = f->cols; continue; }   // (the same pointer: freed once)
        int P = 0, Q = 0;
        if (!spec_rect_factor(n, &P, &Q)) return fail(ctx, HN_ERR_ARG, "internal: no factorisation of the domain size %d", n);
        if (lds_bytes(n, P, Q, 1) > (size_t)kLdsAttr)
            return fail(ctx, HN_ERR_UNSUPPORTED, "float64 FFT route: a line of %d = %d * %d points needs %zu bytes of LDS, more than a workgroup may declare", n, P, Q,
                        lds_bytes(n, P, Q, 1));
        if (int rc = build_tables(ctx, *ax, n, P, Q); rc != HN_OK) return rc;
    }
    if (int rc = grow(ctx, &f->part, &f->part_cap, part_needed); rc != HN_OK) return rc;
    return grow(ctx, &f->mid, &f->mid_cap, mid_needed);
}

int f64_fft_launch(hn_ctx* ctx, const double* wf, double* out, const double* ksq, const double* ksq_im, const double* src, long src_sb, bool want_part,
                   int batch, hipStream_t s, double** part) {
    const F64Fft& f = *ctx->f64fft;
    const int h = f.h, w = f.w;
    double* mid = out != nullptr ? out : f.mid;
    *part = want_part ? f.part : nullptr;
    // each pass by its own axis: lines per block, buffers, LDS
    const F64Axis &ay = f.cols, &ax = f.rows;
    const int Ly = lines_per_block(h, w, ay.P == 1 ? 3 : 4, batch), Lx = lines_per_block(w, h, ax.P == 1 ? 3 : 4, batch);
    hipLaunchKernelGGL((k_f64_fft<1, false>), dim3(w / Ly, batch), dim3(kThreads), lds_bytes(h, ay.P, ay.Q, Ly), s, wf, nullptr, mid, nullptr, nullptr, nullptr,
                       0L, tabs_of(ay), h, w, ay.P, ilog2(ay.Q), ilog2(Ly), 0, nullptr);
    const dim3 grid(h / Lx, batch);
    const size_t lds = lds_bytes(w, ax.P, ax.Q, Lx);
    const int logq = ilog2(ax.Q), logl = ilog2(Lx);
    if (ksq_im != nullptr)
        hipLaunchKernelGGL((k_f64_fft<0, true>), grid, dim3(kThreads), lds, s, wf, mid, out, ksq, ksq_im, src, src_sb, tabs_of(ax), h, w, ax.P, logq, logl, 1, *part);
    else
        hipLaunchKernelGGL((k_f64_fft<0, false>), grid, dim3(kThreads), lds, s, wf, mid, out, ksq, nullptr, src, src_sb, tabs_of(ax), h, w, ax.P, logq, logl,
                           ksq != nullptr ? 1 : 0, *part);
    return HN_OK;
}

}  // namespace hn
