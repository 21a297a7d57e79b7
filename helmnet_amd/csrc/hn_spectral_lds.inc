// LDS-resident line transforms shared by the runtime-factor spectral kernels (hn_spectral_mixed.hip, hn_spectral_rect.hip): complex helpers, the in-place
// Q-point transforms and the partial sums of the direct P-point DFT.  Included inside an anonymous namespace of namespace hn.
#pragma once

constexpr int kMixThreads = 256;

__device__ __forceinline__ float2 cadd(float2 x, float2 y) { return make_float2(x.x + y.x, x.y + y.y); }
__device__ __forceinline__ float2 csub(float2 x, float2 y) { return make_float2(x.x - y.x, x.y - y.y); }
__device__ __forceinline__ float2 cmul(float2 x, float2 y) { return make_float2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x); }
__device__ __forceinline__ float2 cmulc(float2 x, float2 y) { return make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y); }   // x * conj(y)

// Q-point transforms in place on `nseq` contiguous sequences of each of `nbuf` (1 or 2) buffers.  !INV: decimation in frequency, natural in,
// bit-reversed out.  INV: the transposed flow graph with conjugate twiddles, bit-reversed in, natural out, unnormalised.  One item = the four
// elements {a, a + h/2, a + h, a + 3h/2} that two consecutive radix-2 stages (spans 2h and h) keep among themselves; an odd log2 Q leaves the
// span-2 stage (twiddle 1) on its own.  Ends with a barrier; the caller provides the one in front.
template <bool INV>
__device__ __forceinline__ void fft_inplace(float2* b0, float2* b1, int nbuf, int nseq, int logq, const float2* twq, int tid) {
    const int Q = 1 << logq;
    const int per4 = nseq << (logq - 2), per2 = nseq << (logq - 1);
    auto pairs = [&]() {
        for (int item = tid; item < nbuf * per2; item += kMixThreads) {
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
        for (int item = tid; item < nbuf * per4; item += kMixThreads) {
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
__device__ __forceinline__ float2 plus_i(float2 a, float2 b) { return make_float2(a.x - b.y, a.y + b.x); }    // a + i b
__device__ __forceinline__ float2 minus_i(float2 a, float2 b) { return make_float2(a.x + b.y, a.y - b.x); }   // a - i b
