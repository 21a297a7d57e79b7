// One restart cycle of GMRES on the spectral Helmholtz operator, fused (hn_gmres_cycle).
//
// The method is the one helmnet_amd/gmres.py runs with torch (matlab/spectral_gmres_solver.m:86-115 is the reference's classical baseline):
// r = rhs - A x, v_0 = r / |r|; per inner step w = A v_k, two passes of classical Gram-Schmidt, H[:k+1, k] = h + h2, H[k+1, k] = |w|, v_{k+1} = w / |w|;
// progressive Givens rotations per sample with the residual estimate |g[k+1]| / sqrt(2 n^2).  A u = L(u) + k_sq * u is spec_apply, the launcher
// hn_residual uses, with a source of zeros (the 256- and 512-point row kernels read their source operand unconditionally: the zeros are a page of the
// workspace, and x - 0 is x bit for bit).  spec_apply's tensors have dense sample strides, the caller's basis has not: the operator reads v_k from and
// writes w to two dense fields of the workspace, and the scale kernel stores v_{k+1} into both places.
//
// Per inner step, besides the operator's own launches: k_dots (h = <v_j, w>), k_sub<0> (w -= sum h_j v_j, then h2 = <v_j, w>), k_sub<1> (the second
// subtraction, then the partial sums of |w|^2), k_small (one wavefront per sample: H column, rotations, g, the rmse row, the stop flag and, when the
// sample stops, the back-substitution) and k_scale.  A field is [re plane | im plane]; a block owns 1024 pixels of a sample, keeps its piece of w in
// registers (one float4 per plane and thread) and streams the k + 1 basis pieces past it; the multiplication by i is the choice of plane.
// Every sum has a fixed order: per-thread, a wavefront shuffle tree, the four wavefronts, then the blocks' partial sums in chunk order (in double) by
// whoever consumes them -- no float atomics, nothing depends on the batch a sample shares (grid.y is the sample), two calls give the same bits.
#include "hn_internal.h"

namespace hn {

constexpr int kKryMaxRestart = 64;
constexpr int kKryChunk = 1024;   // pixels per block: 256 threads x one float4 per plane

struct KrylovWs {
    int batch = 0, restart = 0, n = 0, nchunk = 0;
    void* block = nullptr;    // one allocation; the pointers below lead into it
    float* vin = nullptr;     // [B][2 n^2]  v_k, densely strided: the operator's input
    float* w = nullptr;       // [B][2 n^2]  the operator's output, orthogonalised in place
    float* zero = nullptr;    // [2 n^2]     the zero source
    float* part = nullptr;    // [B][2 passes][restart + 1][nchunk][2]  per-block partial inner products (re, im)
    float* npart = nullptr;   // [B][nchunk]  per-block partial sums of |w|^2
    float* scale = nullptr;   // [B]  |r| resp. |w|: the divisor of the next k_scale
    double* g = nullptr;      // [B][restart + 1][2]  the rotated right-hand side beta e_1
    double* cs = nullptr;     // [B][restart][4]      rotations (c, s), complex
    double* R = nullptr;      // [B][restart][restart + 1][2]  column k of the triangular factor in rows 0 .. k
    float* y = nullptr;       // [B][restart][2]      the back-substituted coefficients of the truncation the sample stopped at
    int* stopped = nullptr;   // [B]
};

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ float4 ld4(const float* p, bool on) { return on ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the blocks' partial sums of one inner product component, in chunk order
__device__ __forceinline__ float sum_chunks(const float* p, int nchunk, int stride) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += (double)p[(long)c * stride];
    return (float)s;
}

// <v_j, w> (conjugate on v) of this block's piece for j <= k -> out[j][chunk][2]; red: [kKryMaxRestart + 1][4][2]
__device__ __forceinline__ void piece_dots(const float* V, long P, long off, bool on, float4 wr, float4 wi, int k, float (*red)[4][2], float* out,
                                           int nchunk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = 0; j <= k; ++j) {
        const float* v = V + (long)j * 2 * P + off;
        const float4 vr = ld4(v, on), vi = ld4(v + P, on);
        const float re = wave_sum(dot4(vr, wr) + dot4(vi, wi));
        const float im = wave_sum(dot4(vr, wi) - dot4(vi, wr));
        if (lane == 0) { red[j][wave][0] = re; red[j][wave][1] = im; }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * (k + 1)) {
        const int j = threadIdx.x >> 1, comp = threadIdx.x & 1;
        out[((long)j * nchunk + blockIdx.x) * 2 + comp] = (red[j][0][comp] + red[j][1][comp]) + (red[j][2][comp] + red[j][3][comp]);
    }
}

// part: this sample's [2 passes][restart + 1][nchunk][2]
__global__ __launch_bounds__(256) void k_dots(const float* __restrict__ w, const float* __restrict__ basis, float* __restrict__ part, long P, int k,
                                              int restart, int nchunk) {
    __shared__ float red[kKryMaxRestart + 1][4][2];
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    const bool on = off < P;
    const float* pw = w + (long)b * 2 * P + off;
    const float4 wr = ld4(pw, on), wi = ld4(pw + P, on);
    piece_dots(basis + (long)b * (restart + 1) * 2 * P, P, off, on, wr, wi, k, red, part + (long)b * 2 * (restart + 1) * nchunk * 2, nchunk);
}

// w -= sum_j h_j v_j with h the summed partials of pass PASS; then PASS 0: the second pass's inner products of the new w, PASS 1: the partial sum of |w|^2
template <int PASS>
__global__ __launch_bounds__(256) void k_sub(float* __restrict__ w, const float* __restrict__ basis, float* __restrict__ part, float* __restrict__ npart,
                                             long P, int k, int restart, int nchunk) {
    __shared__ float red[kKryMaxRestart + 1][4][2];
    __shared__ float h[kKryMaxRestart + 1][2];
    const int b = blockIdx.y;
    float* sp = part + (long)b * 2 * (restart + 1) * nchunk * 2;
    if ((int)threadIdx.x < 2 * (k + 1)) {
        const int j = threadIdx.x >> 1, comp = threadIdx.x & 1;
        h[j][comp] = sum_chunks(sp + ((long)(PASS * (restart + 1) + j) * nchunk) * 2 + comp, nchunk, 2);
    }
    __syncthreads();
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    const bool on = off < P;
    float* pw = w + (long)b * 2 * P + off;
    float4 wr = ld4(pw, on), wi = ld4(pw + P, on);
    const float* V = basis + (long)b * (restart + 1) * 2 * P;
    float4 ar = make_float4(0.f, 0.f, 0.f, 0.f), ai = ar;
#pragma unroll 2
    for (int j = 0; j <= k; ++j) {
        const float* v = V + (long)j * 2 * P + off;
        const float4 vr = ld4(v, on), vi = ld4(v + P, on);
        const float hr = h[j][0], hi = h[j][1];
        ar.x += hr * vr.x - hi * vi.x; ar.y += hr * vr.y - hi * vi.y; ar.z += hr * vr.z - hi * vi.z; ar.w += hr * vr.w - hi * vi.w;
        ai.x += hr * vi.x + hi * vr.x; ai.y += hr * vi.y + hi * vr.y; ai.z += hr * vi.z + hi * vr.z; ai.w += hr * vi.w + hi * vr.w;
    }
    wr.x -= ar.x; wr.y -= ar.y; wr.z -= ar.z; wr.w -= ar.w;
    wi.x -= ai.x; wi.y -= ai.y; wi.z -= ai.z; wi.w -= ai.w;
    if (on) {
        *reinterpret_cast<float4*>(pw) = wr;
        *reinterpret_cast<float4*>(pw + P) = wi;
    }
    if (PASS == 0) {
        piece_dots(V, P, off, on, wr, wi, k, red, sp + (long)(restart + 1) * nchunk * 2, nchunk);
    } else {
        const float s = wave_sum(dot4(wr, wr) + dot4(wi, wi));
        if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6][0] = s;
        __syncthreads();
        if (threadIdx.x == 0) npart[(long)b * nchunk + blockIdx.x] = (red[0][0][0] + red[0][1][0]) + (red[0][2][0] + red[0][3][0]);
    }
}

__global__ __launch_bounds__(256) void k_norm_part(const float* __restrict__ w, float* __restrict__ npart, long P, int nchunk) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    const bool on = off < P;
    const float* pw = w + (long)b * 2 * P + off;
    const float4 wr = ld4(pw, on), wi = ld4(pw + P, on);
    const float s = wave_sum(dot4(wr, wr) + dot4(wi, wi));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) npart[(long)b * nchunk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// v = sign * w / max(scale, tiny) into the dense operator input and into slot `slot` of the caller's basis
__global__ __launch_bounds__(256) void k_scale(const float* __restrict__ w, const float* __restrict__ scale, float sign, float* __restrict__ vin,
                                               float* __restrict__ basis, long P, int slot, int restart) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const float d = fmaxf(scale[b], 1e-30f);
    const float* pw = w + (long)b * 2 * P + off;
    float4 wr = *reinterpret_cast<const float4*>(pw), wi = *reinterpret_cast<const float4*>(pw + P);
    wr.x = sign * wr.x / d; wr.y = sign * wr.y / d; wr.z = sign * wr.z / d; wr.w = sign * wr.w / d;
    wi.x = sign * wi.x / d; wi.y = sign * wi.y / d; wi.z = sign * wi.z / d; wi.w = sign * wi.w / d;
    float* pv = vin + (long)b * 2 * P + off;
    float* pb = basis + ((long)b * (restart + 1) + slot) * 2 * P + off;
    *reinterpret_cast<float4*>(pv) = wr; *reinterpret_cast<float4*>(pv + P) = wi;
    *reinterpret_cast<float4*>(pb) = wr; *reinterpret_cast<float4*>(pb + P) = wi;
}

struct SmallArgs {
    const float* part; const float* npart; float* scale; double* g; double* cs; double* R; float* y; int* stopped;
    float* hess; float* rmse; int32_t* k_used;
    int batch, restart, nchunk;
    double tol, inv_sqrt_npix;
};

// start of the cycle: beta, g = beta e_1, rmse row 0, the samples that start below the tolerance
__global__ __launch_bounds__(64) void k_small_init(SmallArgs a) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < a.nchunk; ++c) s += (double)a.npart[(long)b * a.nchunk + c];
    const float beta = (float)sqrt(s);
    a.scale[b] = beta;
    double* g = a.g + (long)b * (a.restart + 1) * 2;
    g[0] = (double)beta;
    g[1] = 0.0;
    const double est = (double)beta * a.inv_sqrt_npix;
    a.rmse[b] = (float)est;
    a.stopped[b] = est < a.tol ? 1 : 0;
    a.k_used[b] = 0;
}

// inner step k of one sample: H column, the rotations, g, the rmse row, the stop decision and (once) the back-substitution
__global__ __launch_bounds__(64) void k_small(SmallArgs a, int k) {
    __shared__ double col[kKryMaxRestart + 1][2];
    __shared__ double rot[kKryMaxRestart][4];
    __shared__ double ysh[2];
    __shared__ int back;
    const int b = blockIdx.x, lane = threadIdx.x, R = a.restart;
    const float* sp = a.part + (long)b * 2 * (R + 1) * a.nchunk * 2;
    float* hs = a.hess + (long)b * (R + 1) * R * 2;
    double* g = a.g + (long)b * (R + 1) * 2;
    double* cs = a.cs + (long)b * R * 4;
    double* Rm = a.R + (long)b * R * (R + 1) * 2;
    if (lane <= k) {
        const int j = lane;
        const float hr = sum_chunks(sp + (long)j * a.nchunk * 2, a.nchunk, 2) + sum_chunks(sp + (long)(R + 1 + j) * a.nchunk * 2, a.nchunk, 2);
        const float hi = sum_chunks(sp + (long)j * a.nchunk * 2 + 1, a.nchunk, 2) + sum_chunks(sp + (long)(R + 1 + j) * a.nchunk * 2 + 1, a.nchunk, 2);
        hs[((long)j * R + k) * 2] = hr;
        hs[((long)j * R + k) * 2 + 1] = hi;
        col[j][0] = (double)hr;
        col[j][1] = (double)hi;
    }
    for (int j = k + 2 + lane; j <= R; j += 64) { hs[((long)j * R + k) * 2] = 0.f; hs[((long)j * R + k) * 2 + 1] = 0.f; }
    if (lane < k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rot[lane][q] = cs[lane * 4 + q];
    }
    if (lane == 0) {
        double s = 0.0;
        for (int c = 0; c < a.nchunk; ++c) s += (double)a.npart[(long)b * a.nchunk + c];
        const float hn = (float)sqrt(s);
        hs[((long)(k + 1) * R + k) * 2] = hn;
        hs[((long)(k + 1) * R + k) * 2 + 1] = 0.f;
        a.scale[b] = hn;
        col[k + 1][0] = (double)hn;
        col[k + 1][1] = 0.0;
        back = 0;
    }
    __syncthreads();
    if (lane == 0) {
        // rotation j is [[conj(c), conj(s)], [-s, c]] on rows (j, j + 1)
        for (int j = 0; j < k; ++j) {
            const double cr = rot[j][0], ci = rot[j][1], sr = rot[j][2], si = rot[j][3];
            const double ar = col[j][0], ai = col[j][1], br = col[j + 1][0], bi = col[j + 1][1];
            col[j][0] = (cr * ar + ci * ai) + (sr * br + si * bi);
            col[j][1] = (cr * ai - ci * ar) + (sr * bi - si * br);
            col[j + 1][0] = -(sr * ar - si * ai) + (cr * br - ci * bi);
            col[j + 1][1] = -(sr * ai + si * ar) + (cr * bi + ci * br);
        }
        const double ar = col[k][0], ai = col[k][1], br = col[k + 1][0], bi = col[k + 1][1];
        double d = sqrt(ar * ar + ai * ai + br * br + bi * bi);
        if (d == 0.0) d = 1.0;
        const double cr = ar / d, ci = ai / d, sr = br / d, si = bi / d;
        col[k][0] = (cr * ar + ci * ai) + (sr * br + si * bi);
        col[k][1] = (cr * ai - ci * ar) + (sr * bi - si * br);
        cs[k * 4] = cr; cs[k * 4 + 1] = ci; cs[k * 4 + 2] = sr; cs[k * 4 + 3] = si;
        const double gr = g[2 * k], gi = g[2 * k + 1];
        g[2 * k] = cr * gr + ci * gi;
        g[2 * k + 1] = cr * gi - ci * gr;
        const double nr = -(sr * gr - si * gi), ni = -(sr * gi + si * gr);
        g[2 * k + 2] = nr;
        g[2 * k + 3] = ni;
        const double est = sqrt(nr * nr + ni * ni) * a.inv_sqrt_npix;
        float* row = a.rmse + (long)(k + 1) * a.batch;
        if (a.stopped[b]) {
            row[b] = row[b - a.batch];   // the value the sample stopped at
        } else {
            row[b] = (float)est;
            if (est < a.tol) back = k + 1;
            else if (k == R - 1) back = R;
        }
    }
    __syncthreads();
    if (lane <= k) { Rm[((long)k * (R + 1) + lane) * 2] = col[lane][0]; Rm[((long)k * (R + 1) + lane) * 2 + 1] = col[lane][1]; }
    __syncthreads();
    const int m = back;
    if (m == 0) return;
    // R[:m, :m] y = g[:m], column by column: lane r holds g_r
    double gr = 0.0, gi = 0.0;
    if (lane < m) { gr = g[2 * lane]; gi = g[2 * lane + 1]; }
    for (int i = m - 1; i >= 0; --i) {
        const double* ci = Rm + (long)i * (R + 1) * 2;
        if (lane == i) {
            double dr = ci[2 * i], di = ci[2 * i + 1];
            if (dr == 0.0 && di == 0.0) dr = 1.0;
            const double den = dr * dr + di * di;
            ysh[0] = (gr * dr + gi * di) / den;
            ysh[1] = (gi * dr - gr * di) / den;
        }
        __syncthreads();
        const double yr = ysh[0], yi = ysh[1];
        if (lane < i) {
            const double rr = ci[2 * lane], ri = ci[2 * lane + 1];
            gr -= rr * yr - ri * yi;
            gi -= rr * yi + ri * yr;
        }
        if (lane == i) { a.y[((long)b * R + i) * 2] = (float)yr; a.y[((long)b * R + i) * 2 + 1] = (float)yi; }
        __syncthreads();
    }
    if (lane == 0) { a.stopped[b] = 1; a.k_used[b] = m; }
}

// x += sum_{j < k_used} y_j v_j; a sample with k_used == 0 is not written
__global__ __launch_bounds__(256) void k_update(float* __restrict__ x, const float* __restrict__ basis, const float* __restrict__ y,
                                                const int32_t* __restrict__ k_used, long P, int restart) {
    const int b = blockIdx.y;
    const int m = k_used[b];
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (m <= 0 || off >= P) return;
    const float* V = basis + (long)b * (restart + 1) * 2 * P;
    const float* py = y + (long)b * restart * 2;
    float4 ar = make_float4(0.f, 0.f, 0.f, 0.f), ai = ar;
#pragma unroll 2
    for (int j = 0; j < m; ++j) {
        const float* v = V + (long)j * 2 * P + off;
        const float4 vr = *reinterpret_cast<const float4*>(v), vi = *reinterpret_cast<const float4*>(v + P);
        const float yr = py[2 * j], yi = py[2 * j + 1];
        ar.x += yr * vr.x - yi * vi.x; ar.y += yr * vr.y - yi * vi.y; ar.z += yr * vr.z - yi * vi.z; ar.w += yr * vr.w - yi * vi.w;
        ai.x += yr * vi.x + yi * vr.x; ai.y += yr * vi.y + yi * vr.y; ai.z += yr * vi.z + yi * vr.z; ai.w += yr * vi.w + yi * vr.w;
    }
    float* px = x + (long)b * 2 * P + off;
    float4 xr = *reinterpret_cast<float4*>(px), xi = *reinterpret_cast<float4*>(px + P);
    xr.x += ar.x; xr.y += ar.y; xr.z += ar.z; xr.w += ar.w;
    xi.x += ai.x; xi.y += ai.y; xi.z += ai.z; xi.w += ai.w;
    *reinterpret_cast<float4*>(px) = xr;
    *reinterpret_cast<float4*>(px + P) = xi;
}

bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return s != nullptr && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the workspace for (batch, restart) on the current domain: built by the first call, grown by a larger batch or restart -- never under stream capture
int prepare(hn_ctx* ctx, int batch, int restart, hipStream_t s) {
    const int n = ctx->tab.n;
    KrylovWs* ws = ctx->kry;
    if (ws != nullptr && ws->n == n && batch <= ws->batch && restart <= ws->restart) return HN_OK;
    if (capturing(s))
        return fail(ctx, HN_ERR_STATE, "hn_gmres_cycle: the workspace (or a larger batch's / restart's) is built by the first call, which must not be under stream capture");
    const int cb = ws != nullptr && ws->n == n && ws->batch > batch ? ws->batch : batch;
    const int cr = ws != nullptr && ws->n == n && ws->restart > restart ? ws->restart : restart;
    krylov_free(ctx);   // (hipFree waits for the launches that still use the old one)
    ws = new (std::nothrow) KrylovWs();
    if (!ws) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    ctx->kry = ws;
    const size_t P = (size_t)n * n, B = (size_t)cb, R = (size_t)cr;
    const size_t nchunk = (P + kKryChunk - 1) / kKryChunk;
    const size_t sizes[] = {B * 2 * P * 4, B * 2 * P * 4, 2 * P * 4, B * 2 * (R + 1) * nchunk * 2 * 4, B * nchunk * 4, B * 4,
                            B * (R + 1) * 2 * 8, B * R * 4 * 8, B * R * (R + 1) * 2 * 8, B * R * 2 * 4, B * 4};
    size_t total = 0;
    for (size_t v : sizes) total += up256(v);
    hipError_t e = hipMalloc(&ws->block, total);
    if (e == hipSuccess) e = hipMemset(ws->block, 0, total);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        krylov_free(ctx);
        return fail(ctx, e == hipErrorOutOfMemory ? HN_ERR_NOMEM : HN_ERR_HIP, "hn_gmres_cycle: workspace of %zu bytes: %s", total, hipGetErrorString(e));
    }
    char* p = static_cast<char*>(ws->block);
    int i = 0;
    auto take = [&]() { char* q = p; p += up256(sizes[i++]); return q; };
    ws->vin = (float*)take(); ws->w = (float*)take(); ws->zero = (float*)take(); ws->part = (float*)take(); ws->npart = (float*)take();
    ws->scale = (float*)take(); ws->g = (double*)take(); ws->cs = (double*)take(); ws->R = (double*)take(); ws->y = (float*)take();
    ws->stopped = (int*)take();
    ws->batch = cb; ws->restart = cr; ws->n = n; ws->nchunk = (int)nchunk;
    return HN_OK;
}

struct Range { const void* p; size_t bytes; const char* name; };

}  // namespace

void krylov_free(hn_ctx* ctx) {
    KrylovWs* ws = ctx->kry;
    if (ws == nullptr) return;
    (void)hipFree(ws->block);
    delete ws;
    ctx->kry = nullptr;
}

}  // namespace hn

using namespace hn;

extern "C" int hn_gmres_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                              float* basis, float* hess, float* rmse, int32_t* k_used, void* stream) {
    if (!ctx || !x || !k_sq || !rhs || !basis || !hess || !rmse || !k_used) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: NULL argument");
    if (ctx->tab.n == 0) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: hn_set_domain has not been called");
    if (batch < 1) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: batch must be positive (got %d)", batch);
    if (restart < 1 || restart > kKryMaxRestart) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: restart %d outside [1, %d]", restart, kKryMaxRestart);
    if (rhs_batch != 1 && rhs_batch != batch) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: rhs batch %d must be 1 or equal to the batch %d", rhs_batch, batch);
    const int n = ctx->tab.n;
    const long P = (long)n * n;
    const size_t B = (size_t)batch, R = (size_t)restart;
    const Range r[] = {{x, B * 2 * P * 4, "x"}, {k_sq, B * P * 4, "k_sq"}, {rhs, (size_t)rhs_batch * 2 * P * 4, "rhs"}, {basis, B * (R + 1) * 2 * P * 4, "basis"},
                       {hess, B * (R + 1) * R * 2 * 4, "hess"}, {rmse, (R + 1) * B * 4, "rmse"}, {k_used, B * 4, "k_used"}};
    for (int i = 0; i < 4; ++i)   // the fields are read and written as float4
        if (reinterpret_cast<uintptr_t>(r[i].p) % 16 != 0) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: %s is not 16-byte aligned", r[i].name);
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j) {
            const char *a = static_cast<const char*>(r[i].p), *b = static_cast<const char*>(r[j].p);
            if (a < b + r[j].bytes && b < a + r[i].bytes) return fail(ctx, HN_ERR_ARG, "hn_gmres_cycle: %s overlaps %s", r[i].name, r[j].name);
        }
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    int rc = prepare(ctx, batch, restart, s);
    if (rc != HN_OK) return rc;
    const KrylovWs& ws = *ctx->kry;
    // the partial-sum table is indexed with the CALL's restart and batch: a workspace sized for more holds it
    const int nchunk = ws.nchunk;
    const dim3 grid(nchunk, batch), blk(256);
    SmallArgs a{ws.part, ws.npart, ws.scale, ws.g, ws.cs, ws.R, ws.y, ws.stopped, hess, rmse, k_used, batch, restart, nchunk,
                (double)tol, 1.0 / sqrt(2.0 * (double)P)};
    // w = A x - rhs = -r
    if ((rc = spec_apply(ctx, x, ws.w, k_sq, rhs, rhs_batch, batch, nullptr, s)) != HN_OK) return rc;
    hipLaunchKernelGGL(k_norm_part, grid, blk, 0, s, ws.w, ws.npart, P, nchunk);
    hipLaunchKernelGGL(k_small_init, dim3(batch), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_scale, grid, blk, 0, s, ws.w, ws.scale, -1.f, ws.vin, basis, P, 0, restart);
    for (int k = 0; k < restart; ++k) {
        if ((rc = spec_apply(ctx, ws.vin, ws.w, k_sq, ws.zero, 1, batch, nullptr, s)) != HN_OK) return rc;
        hipLaunchKernelGGL(k_dots, grid, blk, 0, s, ws.w, basis, ws.part, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_sub<0>, grid, blk, 0, s, ws.w, basis, ws.part, ws.npart, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_sub<1>, grid, blk, 0, s, ws.w, basis, ws.part, ws.npart, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_small, dim3(batch), dim3(64), 0, s, a, k);
        hipLaunchKernelGGL(k_scale, grid, blk, 0, s, ws.w, ws.scale, 1.f, ws.vin, basis, P, k + 1, restart);
    }
    hipLaunchKernelGGL(k_update, grid, blk, 0, s, x, basis, ws.y, k_used, P, restart);
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}
