// One restart cycle of GMRES on the spectral Helmholtz operator, fused (hn_gmres_cycle).
//
// The method is the one helmnet_amd/gmres.py runs with torch (matlab/spectral_gmres_solver.m:86-115 is the reference's classical baseline):
// r = rhs - A x, v_0 = r / |r|; per inner step w = A v_k, two passes of classical Gram-Schmidt, H[:k+1, k] = h + h2, H[k+1, k] = |w|, v_{k+1} = w / |w|;
// progressive Givens rotations per sample with the residual estimate |g[k+1]| / sqrt(2 n^2).  A u = L(u) + k_sq * u is spec_forward, the launcher
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
//
// hn_gmres_refine_cycle (at the end of this file) wraps the same launches into one step of iterative refinement: the true residual (hn_f64.hip) and the
// update in float64, the cycle in fp32 on the scaled correction equation A d = r / s.  hn_fgmres_refine_cycle_lossy is that step for an absorbing
// medium: the float64 residual f64_apply_lossy's, the cycle and the preconditioner the lossy ones.
//
// The medium (hn_internal.h: Medium) is built by the entry point and passed down: A is spec_forward, A^H spec_backward and the learned iteration
// step_entry on it, whichever kind it is.
//
// hn_fgmres_cycle / hn_fgmres_refine_cycle are the same launches as a FLEXIBLE cycle (Saad 1993), right-preconditioned by the learned iteration: per inner
// step z_k = M(v_k) -- precond_iters iterations of hn_step on A z = alpha v_k from rest, z_k = wf / alpha --, w = A z_k, the orthogonalisation and the small
// problem on V as before, the update x += sum y_j z_j over the caller's zbasis.  The preconditioner is a parameter of launch_cycle (Precond); without one
// (zbasis nullptr) not one launch or argument of hn_gmres_cycle differs.  Three streaming kernels (k_seed, k_take, k_take_copy) move the vectors; none sums.
//
// hn_fgmres_adjoint_cycle is the flexible cycle on A^H (spec_backward): the operator is a parameter of launch_cycle (Op), and with Op::Forward not one launch
// or argument of the four entry points above differs.  spec_backward has no source operand: the start residual is its output minus rhs (k_minus_rhs, which
// also leaves the partial sums of |w|^2 that k_norm_part leaves for the forward operator).  The learned network approximates A^-1, not A^-H; the PML
// operator is complex-symmetric up to the diagonal similarity W = gamma_y[i] gamma_x[j] (A^T ~ W A W^-1), so A^-H v ~ conj(W A^-1 (conj(v) / W)): the
// preconditioner is the SAME hn_step problem between two streaming kernels (k_seed_adj, k_take_adj) that conjugate and scale by 1 / W and W.
// hn_fgmres_adjoint_cycle_medium is that cycle on A_rho^H; its similarity weight is W / rho (k_seed_adj_rho, k_take_adj_rho read the caller's rho plane).
// hn_adjoint_grad (at the end) is the pointwise product that turns the adjoint solution into the gradients with respect to k_sq and the source.
#include "hn_internal.h"

namespace hn {

constexpr int kKryMaxRestart = 64;
constexpr int kKryChunk = 1024;   // pixels per block: 256 threads x one float4 per plane

struct KrylovWs {
    int batch = 0, restart = 0, n = 0, nchunk = 0;
    DeviceBlock block;        // one allocation; the pointers below lead into it
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

// what hn_gmres_refine_cycle needs beyond the cycle's workspace and the float64 operator's tables
struct RefineWs {
    int batch = 0, n = 0;
    DeviceBlock block;        // one allocation; the pointers below lead into it
    double* ksq64 = nullptr;  // [B][n^2]    k_sq up-cast
    double* ksq_im64 = nullptr;   // [B][n^2]  k_sq_im up-cast: only once hn_fgmres_refine_cycle_lossy has asked for it
    double* rhs64 = nullptr;  // [B][2 n^2]  rhs up-cast (the first rhs_batch samples)
    double* res64 = nullptr;  // [B][2 n^2]  A x - b
    float* rhs32 = nullptr;   // [B][2 n^2]  -res / s: the cycle's right-hand side
    float* d32 = nullptr;     // [B][2 n^2]  the cycle's iterate: the correction
    double* tol = nullptr;    // [B]  max(tol / s, inner_floor)
    int* stop = nullptr;      // [B]  rmse64 < tol (or a residual of exactly zero)
};

// what the learned preconditioner of hn_fgmres_cycle works on: one hn_step problem of `batch` samples
struct PrecondWs {
    int batch = 0, n = 0;
    int64_t state_len = 0;
    DeviceBlock block;        // one allocation; the pointers below lead into it
    float* src = nullptr;     // [B][2 n^2]  alpha v_k
    float* wf = nullptr;      // [B][2 n^2]  the learned iterate, from zero
    float* res = nullptr;     // [B][2 n^2]  its residual, from 0 - src
    float* states = nullptr;  // [B][2][state_len]  the hidden states, from zero
};

// the similarity weight of the adjoint preconditioner on the current domain: gamma = 1 + i sigma / k per axis with sigma the fp32 table's value,
// W[i][j] = gamma[i] gamma[j] and 1 / W formed in double, each rounded once to fp32
struct AdjointW {
    int n = 0;
    DeviceBlock block;        // one allocation; the pointers below lead into it
    float* w = nullptr;       // [2][n^2]  W, (re | im) planes
    float* winv = nullptr;    // [2][n^2]  1 / W
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

// the adjoint cycle's start: w = A^H x comes without a source operand -- w -= rhs (w = -r, as spec_apply leaves it), then k_norm_part's partial sums
__global__ __launch_bounds__(256) void k_minus_rhs(float* __restrict__ w, const float* __restrict__ rhs, long rhs_sb, float* __restrict__ npart, long P,
                                                   int nchunk) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    const bool on = off < P;
    float* pw = w + (long)b * 2 * P + off;
    const float* pr = rhs + (long)b * rhs_sb + off;
    float4 wr = ld4(pw, on), wi = ld4(pw + P, on);
    const float4 rr = ld4(pr, on), ri = ld4(pr + P, on);
    wr.x -= rr.x; wr.y -= rr.y; wr.z -= rr.z; wr.w -= rr.w;
    wi.x -= ri.x; wi.y -= ri.y; wi.z -= ri.z; wi.w -= ri.w;
    if (on) {
        *reinterpret_cast<float4*>(pw) = wr;
        *reinterpret_cast<float4*>(pw + P) = wi;
    }
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
    // hn_gmres_refine_cycle only (both nullptr for hn_gmres_cycle): a tolerance per sample, written by k_refine_rhs, in place of `tol`; samples the float64
    // residual test has stopped already, whatever their own row 0 says
    const double* tol_dev; const int* pre_stopped;
};
__device__ __forceinline__ double sample_tol(const SmallArgs& a, int b) { return a.tol_dev != nullptr ? a.tol_dev[b] : a.tol; }

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
    a.stopped[b] = (est < sample_tol(a, b) || (a.pre_stopped != nullptr && a.pre_stopped[b] != 0)) ? 1 : 0;
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
            if (est < sample_tol(a, b)) back = k + 1;
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

// x += sum_{j < k_used} y_j v_j; a sample with k_used == 0 is not written.  `slots`: vectors per sample of `basis` (restart + 1; restart for the z_j of
// the flexible cycle)
__global__ __launch_bounds__(256) void k_update(float* __restrict__ x, const float* __restrict__ basis, const float* __restrict__ y,
                                                const int32_t* __restrict__ k_used, long P, int restart, int slots) {
    const int b = blockIdx.y;
    const int m = k_used[b];
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (m <= 0 || off >= P) return;
    const float* V = basis + (long)b * slots * 2 * P;
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

// ---- the flexible cycle's vector traffic: a thread owns four consecutive pixels of both planes, a block 1024 pixels of a sample; nothing sums ----
__device__ __forceinline__ float4 mul4(float4 v, float a) { return make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
__device__ __forceinline__ float4 zero_minus4(float4 v) { return make_float4(0.f - v.x, 0.f - v.y, 0.f - v.z, 0.f - v.w); }
__device__ __forceinline__ float4 div4(float4 v, float a) { return make_float4(v.x / a, v.y / a, v.z / a, v.w / a); }

// the learned solve of A z = alpha v from rest: src = alpha v (one multiply), res = 0 - src, wf = 0; v is the dense operator input
__global__ __launch_bounds__(256) void k_seed(const float* __restrict__ vin, float alpha, float* __restrict__ src, float* __restrict__ res,
                                              float* __restrict__ wf, long P) {
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)blockIdx.y * 2 * P + off;
    const float4 sr = mul4(*reinterpret_cast<const float4*>(vin + at), alpha), si = mul4(*reinterpret_cast<const float4*>(vin + at + P), alpha);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(src + at) = sr; *reinterpret_cast<float4*>(src + at + P) = si;
    *reinterpret_cast<float4*>(res + at) = zero_minus4(sr); *reinterpret_cast<float4*>(res + at + P) = zero_minus4(si);
    *reinterpret_cast<float4*>(wf + at) = z; *reinterpret_cast<float4*>(wf + at + P) = z;
}

// z = wf / alpha (a true division) into slot `slot` of the caller's zbasis [B][restart][2 P] and into the dense operator input
__global__ __launch_bounds__(256) void k_take(const float* __restrict__ wf, float alpha, float* __restrict__ vin, float* __restrict__ zbasis, long P,
                                              int slot, int restart) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)b * 2 * P + off;
    const float4 zr = div4(*reinterpret_cast<const float4*>(wf + at), alpha), zi = div4(*reinterpret_cast<const float4*>(wf + at + P), alpha);
    float* pz = zbasis + ((long)b * restart + slot) * 2 * P + off;
    *reinterpret_cast<float4*>(vin + at) = zr; *reinterpret_cast<float4*>(vin + at + P) = zi;
    *reinterpret_cast<float4*>(pz) = zr; *reinterpret_cast<float4*>(pz + P) = zi;
}

// no preconditioner (precond_iters 0): z = v, copied exactly; the operator input holds it already
__global__ __launch_bounds__(256) void k_take_copy(const float* __restrict__ vin, float* __restrict__ zbasis, long P, int slot, int restart) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const float* pv = vin + (long)b * 2 * P + off;
    float* pz = zbasis + ((long)b * restart + slot) * 2 * P + off;
    *reinterpret_cast<float4*>(pz) = *reinterpret_cast<const float4*>(pv);
    *reinterpret_cast<float4*>(pz + P) = *reinterpret_cast<const float4*>(pv + P);
}

// ---- the adjoint cycle's twins of k_seed / k_take: the same traffic plus the two planes of 1 / W resp. W (shared by the samples) ----
// each component is an fp32 product sum as written (a * b + c * d, contraction as the compiler has it), then ONE multiply by alpha resp. a true division

// src = alpha * (conj(v) * winv): re = vr ir + vi ii, im = vr ii - vi ir; res = 0 - src, wf = 0
__global__ __launch_bounds__(256) void k_seed_adj(const float* __restrict__ vin, const float* __restrict__ winv, float alpha, float* __restrict__ src,
                                                  float* __restrict__ res, float* __restrict__ wf, long P) {
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)blockIdx.y * 2 * P + off;
    const float4 vr = *reinterpret_cast<const float4*>(vin + at), vi = *reinterpret_cast<const float4*>(vin + at + P);
    const float4 ir = *reinterpret_cast<const float4*>(winv + off), ii = *reinterpret_cast<const float4*>(winv + P + off);
    const float4 sr = mul4(make_float4(vr.x * ir.x + vi.x * ii.x, vr.y * ir.y + vi.y * ii.y, vr.z * ir.z + vi.z * ii.z, vr.w * ir.w + vi.w * ii.w), alpha);
    const float4 si = mul4(make_float4(vr.x * ii.x - vi.x * ir.x, vr.y * ii.y - vi.y * ir.y, vr.z * ii.z - vi.z * ir.z, vr.w * ii.w - vi.w * ir.w), alpha);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(src + at) = sr; *reinterpret_cast<float4*>(src + at + P) = si;
    *reinterpret_cast<float4*>(res + at) = zero_minus4(sr); *reinterpret_cast<float4*>(res + at + P) = zero_minus4(si);
    *reinterpret_cast<float4*>(wf + at) = z; *reinterpret_cast<float4*>(wf + at + P) = z;
}

// z = conj(w * wf) / alpha: re = (wr fr - wi fi) / alpha, im = (0 - (wr fi + wi fr)) / alpha, into slot `slot` of zbasis and into the dense operator input
__global__ __launch_bounds__(256) void k_take_adj(const float* __restrict__ wf, const float* __restrict__ w, float alpha, float* __restrict__ vin,
                                                  float* __restrict__ zbasis, long P, int slot, int restart) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)b * 2 * P + off;
    const float4 fr = *reinterpret_cast<const float4*>(wf + at), fi = *reinterpret_cast<const float4*>(wf + at + P);
    const float4 wr = *reinterpret_cast<const float4*>(w + off), wi = *reinterpret_cast<const float4*>(w + P + off);
    const float4 zr = div4(make_float4(wr.x * fr.x - wi.x * fi.x, wr.y * fr.y - wi.y * fi.y, wr.z * fr.z - wi.z * fi.z, wr.w * fr.w - wi.w * fi.w), alpha);
    const float4 zi = div4(zero_minus4(make_float4(wr.x * fi.x + wi.x * fr.x, wr.y * fi.y + wi.y * fr.y, wr.z * fi.z + wi.z * fr.z, wr.w * fi.w + wi.w * fr.w)), alpha);
    float* pz = zbasis + ((long)b * restart + slot) * 2 * P + off;
    *reinterpret_cast<float4*>(vin + at) = zr; *reinterpret_cast<float4*>(vin + at + P) = zi;
    *reinterpret_cast<float4*>(pz) = zr; *reinterpret_cast<float4*>(pz + P) = zi;
}

// ---- the variable-density adjoint cycle's twins of the two above: the weight is W / rho, rho [B][n^2] per sample (A_rho = rho * a W-symmetric operator) ----
// The same expressions with ONE more operation per component, a multiply resp. a true division by rho / rho[b][0], in front of alpha's: with rho == 1
// the bits are k_seed_adj's and k_take_adj's.  Same traffic plus the one plane.  The sample's first pixel (a corner of the PML: the background) normalises
// the plane, so that only ratios of rho enter and the network's right-hand side keeps the magnitude precond_scale gives it whatever the units of rho.

// src = alpha * ((conj(v) * winv) * (rho / rho[b][0])); res = 0 - src, wf = 0
__global__ __launch_bounds__(256) void k_seed_adj_rho(const float* __restrict__ vin, const float* __restrict__ winv, const float* __restrict__ rho, float alpha,
                                                      float* __restrict__ src, float* __restrict__ res, float* __restrict__ wf, long P) {
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)blockIdx.y * 2 * P + off;
    const float4 vr = *reinterpret_cast<const float4*>(vin + at), vi = *reinterpret_cast<const float4*>(vin + at + P);
    const float4 ir = *reinterpret_cast<const float4*>(winv + off), ii = *reinterpret_cast<const float4*>(winv + P + off);
    const float r0 = rho[(long)blockIdx.y * P];
    const float4 rw = *reinterpret_cast<const float4*>(rho + (long)blockIdx.y * P + off);
    const float4 rh = make_float4(rw.x / r0, rw.y / r0, rw.z / r0, rw.w / r0);
    const float4 pr = make_float4(vr.x * ir.x + vi.x * ii.x, vr.y * ir.y + vi.y * ii.y, vr.z * ir.z + vi.z * ii.z, vr.w * ir.w + vi.w * ii.w);
    const float4 pi = make_float4(vr.x * ii.x - vi.x * ir.x, vr.y * ii.y - vi.y * ir.y, vr.z * ii.z - vi.z * ir.z, vr.w * ii.w - vi.w * ir.w);
    const float4 sr = mul4(make_float4(pr.x * rh.x, pr.y * rh.y, pr.z * rh.z, pr.w * rh.w), alpha);
    const float4 si = mul4(make_float4(pi.x * rh.x, pi.y * rh.y, pi.z * rh.z, pi.w * rh.w), alpha);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(src + at) = sr; *reinterpret_cast<float4*>(src + at + P) = si;
    *reinterpret_cast<float4*>(res + at) = zero_minus4(sr); *reinterpret_cast<float4*>(res + at + P) = zero_minus4(si);
    *reinterpret_cast<float4*>(wf + at) = z; *reinterpret_cast<float4*>(wf + at + P) = z;
}

// z = conj(w * wf) / (rho / rho[b][0]) / alpha, into slot `slot` of zbasis and into the dense operator input
__global__ __launch_bounds__(256) void k_take_adj_rho(const float* __restrict__ wf, const float* __restrict__ w, const float* __restrict__ rho, float alpha,
                                                      float* __restrict__ vin, float* __restrict__ zbasis, long P, int slot, int restart) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)b * 2 * P + off;
    const float4 fr = *reinterpret_cast<const float4*>(wf + at), fi = *reinterpret_cast<const float4*>(wf + at + P);
    const float4 wr = *reinterpret_cast<const float4*>(w + off), wi = *reinterpret_cast<const float4*>(w + P + off);
    const float r0 = rho[(long)b * P];
    const float4 rw = *reinterpret_cast<const float4*>(rho + (long)b * P + off);
    const float4 rh = make_float4(rw.x / r0, rw.y / r0, rw.z / r0, rw.w / r0);
    const float4 pr = make_float4(wr.x * fr.x - wi.x * fi.x, wr.y * fr.y - wi.y * fi.y, wr.z * fr.z - wi.z * fi.z, wr.w * fr.w - wi.w * fi.w);
    const float4 pi = zero_minus4(make_float4(wr.x * fi.x + wi.x * fr.x, wr.y * fi.y + wi.y * fr.y, wr.z * fi.z + wi.z * fr.z, wr.w * fi.w + wi.w * fr.w));
    const float4 zr = div4(make_float4(pr.x / rh.x, pr.y / rh.y, pr.z / rh.z, pr.w / rh.w), alpha);
    const float4 zi = div4(make_float4(pi.x / rh.x, pi.y / rh.y, pi.z / rh.z, pi.w / rh.w), alpha);
    float* pz = zbasis + ((long)b * restart + slot) * 2 * P + off;
    *reinterpret_cast<float4*>(vin + at) = zr; *reinterpret_cast<float4*>(vin + at + P) = zi;
    *reinterpret_cast<float4*>(pz) = zr; *reinterpret_cast<float4*>(pz + P) = zi;
}

// g_k_sq[b] = -(l_re u_re + l_im u_im); g_src (nullable): lambda per sample (per == 1), or its sum over the `per` samples of the batch in sample order
// GIm: empty (hn_adjoint_grad), or one float* (hn_adjoint_grad_lossy): g_k_sq_im[b] = l_re u_im - l_im u_re from the same loads; the pack stands last, so
// the lossless kernel keeps its arguments, and the other two outputs their expressions and bits
template <typename... GIm>
__global__ __launch_bounds__(256) void k_adjoint_grad(const float* __restrict__ lam, const float* __restrict__ u, float* __restrict__ g_ksq,
                                                      float* __restrict__ g_src, long P, int per, GIm... g_ksq_im) {
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    float4 ar = make_float4(0.f, 0.f, 0.f, 0.f), ai = ar;
    for (int i = 0; i < per; ++i) {
        const int b = blockIdx.y * per + i;
        const long at = (long)b * 2 * P + off;
        const float4 lr = *reinterpret_cast<const float4*>(lam + at), li = *reinterpret_cast<const float4*>(lam + at + P);
        const float4 ur = *reinterpret_cast<const float4*>(u + at), ui = *reinterpret_cast<const float4*>(u + at + P);
        *reinterpret_cast<float4*>(g_ksq + (long)b * P + off) =
            zero_minus4(make_float4(lr.x * ur.x + li.x * ui.x, lr.y * ur.y + li.y * ui.y, lr.z * ur.z + li.z * ui.z, lr.w * ur.w + li.w * ui.w));
        if constexpr (sizeof...(GIm) != 0) {
            float* const gim[] = {g_ksq_im...};
            *reinterpret_cast<float4*>(gim[0] + (long)b * P + off) =
                make_float4(lr.x * ui.x - li.x * ur.x, lr.y * ui.y - li.y * ur.y, lr.z * ui.z - li.z * ur.z, lr.w * ui.w - li.w * ur.w);
        }
        if (i == 0) { ar = lr; ai = li; }
        else { ar.x += lr.x; ar.y += lr.y; ar.z += lr.z; ar.w += lr.w; ai.x += li.x; ai.y += li.y; ai.z += li.z; ai.w += li.w; }
    }
    if (g_src != nullptr) {
        const long at = (long)blockIdx.y * 2 * P + off;
        *reinterpret_cast<float4*>(g_src + at) = ar; *reinterpret_cast<float4*>(g_src + at + P) = ai;
    }
}

// which operator a cycle runs on: A (spec_forward) or A^H (spec_backward)
enum class Op { Forward, Adjoint };

// The preconditioner of a flexible cycle as launch_cycle takes it; zbasis nullptr: none, the cycle is plain GMRES
struct Precond {
    float* zbasis = nullptr;   // [B][restart][2 n^2], the caller's
    int iters = 0;             // hn_step iterations per inner step; 0: z = v
    float alpha = 1.f;         // the learned solve sees alpha v
    const char* who = "";      // the entry point, for what the operator and hn_step report from inside the cycle
    const float* rho = nullptr;   // [B][n^2], the adjoint cycle of a variable-density medium: the similarity weight is W / rho (k_seed_adj_rho, k_take_adj_rho)
};

// what hn_step reported, under the name of the entry point that called it
int step_named(hn_ctx* ctx, const char* who, int rc) {
    if (rc == HN_OK) return rc;
    const std::string msg = ctx->err;
    return fail(ctx, rc, "%s: hn_step: %s", who, msg.c_str());
}

void precond_ws_free(hn_ctx* ctx) {
    if (ctx->pcw == nullptr) return;
    ctx->pcw->block.free();
    delete ctx->pcw;
    ctx->pcw = nullptr;
}

// the learned preconditioner's problem for `batch` samples on the current domain and network -- the caller has refused stream capture
int precond_prepare(hn_ctx* ctx, const char* who, const Medium& m, int batch, hipStream_t s) {
    const int n = ctx->tab.n;
    PrecondWs* ws = ctx->pcw;
    if (ws == nullptr || ws->n != n || ws->state_len != ctx->state_len || batch > ws->batch) {
        precond_ws_free(ctx);
        ws = new (std::nothrow) PrecondWs();
        if (!ws) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
        ctx->pcw = ws;
        const size_t F = (size_t)batch * 2 * n * n * 4;
        const size_t sizes[] = {F, F, F, (size_t)batch * kState * (size_t)ctx->state_len * 4};
        DeviceBlock& k = ws->block;
        if (const int rc = k.alloc(ctx, who, sizes, 4); rc != HN_OK) { precond_ws_free(ctx); return rc; }
        ws->src = (float*)k.take(); ws->wf = (float*)k.take(); ws->res = (float*)k.take(); ws->states = (float*)k.take();
        ws->batch = batch; ws->n = n; ws->state_len = ctx->state_len;
    }
    // hn_step's own refusals (a domain the network's depth does not divide) and its workspace now, with nothing enqueued: the call of the cycle with
    // zero iterations, which launches nothing
    return step_named(ctx, who, step_entry(ctx, m.step_name(), ws->wf, ws->res, ws->states, m, ws->src, batch, batch, 0, nullptr, nullptr, nullptr, nullptr, s));
}

void adjoint_w_free(hn_ctx* ctx) {
    if (ctx->adjw == nullptr) return;
    ctx->adjw->block.free();
    delete ctx->adjw;
    ctx->adjw = nullptr;
}

// W and 1 / W of the current domain -- the caller has refused stream capture; built once per domain (hn_set_domain frees it)
int adjoint_w_prepare(hn_ctx* ctx, const char* who) {
    const SpecTables& t = ctx->tab;
    const int n = t.n;
    if (ctx->adjw != nullptr && ctx->adjw->n == n) return HN_OK;
    adjoint_w_free(ctx);
    AdjointW* aw = new (std::nothrow) AdjointW();
    if (!aw) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    ctx->adjw = aw;
    const size_t P = (size_t)n * n;
    const size_t sizes[] = {2 * P * 4, 2 * P * 4};
    if (const int rc = aw->block.alloc(ctx, who, sizes, 2); rc != HN_OK) { adjoint_w_free(ctx); return rc; }
    aw->w = (float*)aw->block.take(); aw->winv = (float*)aw->block.take();
    aw->n = n;
    const AxisHost ax = spec_axis_host(n, t.pml, t.sigma_max, t.k);
    std::vector<std::complex<double>> gamma(n);
    for (int i = 0; i < n; ++i) gamma[i] = std::complex<double>(1.0, (double)(float)ax.sigma[i] / t.k);   // the sigma maps' fp32 values
    std::vector<float> hw(2 * P), hi(2 * P);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const std::complex<double> w = gamma[i] * gamma[j], iw = 1.0 / w;
            const size_t at = (size_t)i * n + j;
            hw[at] = (float)w.real(); hw[P + at] = (float)w.imag();
            hi[at] = (float)iw.real(); hi[P + at] = (float)iw.imag();
        }
    hipError_t e = hipMemcpy(aw->w, hw.data(), 2 * P * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(aw->winv, hi.data(), 2 * P * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        adjoint_w_free(ctx);
        return fail(ctx, HN_ERR_HIP, "%s: uploading the similarity weight failed: %s", who, hipGetErrorString(e));
    }
    return HN_OK;
}

void cycle_ws_free(hn_ctx* ctx) {
    if (ctx->kry == nullptr) return;
    ctx->kry->block.free();
    delete ctx->kry;
    ctx->kry = nullptr;
}

// the workspace for (batch, restart) on the current domain: built by the first call, grown by a larger batch or restart -- never under stream capture
int prepare(hn_ctx* ctx, int batch, int restart, hipStream_t s) {
    const int n = ctx->tab.n;
    KrylovWs* ws = ctx->kry;
    const bool same = ws != nullptr && ws->n == n;
    if (same && batch <= ws->batch && restart <= ws->restart) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "hn_gmres_cycle: the workspace (or a larger batch's / restart's) is built by the first call, which must not be under stream capture");
    const int cb = same && ws->batch > batch ? ws->batch : batch;         // the larger of old and new, each on its own
    const int cr = same && ws->restart > restart ? ws->restart : restart;
    cycle_ws_free(ctx);
    ws = new (std::nothrow) KrylovWs();
    if (!ws) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    ctx->kry = ws;
    const size_t P = (size_t)n * n, B = (size_t)cb, R = (size_t)cr;
    const size_t nchunk = (P + kKryChunk - 1) / kKryChunk;
    const size_t sizes[] = {B * 2 * P * 4, B * 2 * P * 4, 2 * P * 4, B * 2 * (R + 1) * nchunk * 2 * 4, B * nchunk * 4, B * 4,
                            B * (R + 1) * 2 * 8, B * R * 4 * 8, B * R * (R + 1) * 2 * 8, B * R * 2 * 4, B * 4};
    DeviceBlock& k = ws->block;
    if (const int rc = k.alloc(ctx, "hn_gmres_cycle", sizes, 11); rc != HN_OK) { cycle_ws_free(ctx); return rc; }
    ws->vin = (float*)k.take(); ws->w = (float*)k.take(); ws->zero = (float*)k.take(); ws->part = (float*)k.take(); ws->npart = (float*)k.take();
    ws->scale = (float*)k.take(); ws->g = (double*)k.take(); ws->cs = (double*)k.take(); ws->R = (double*)k.take(); ws->y = (float*)k.take();
    ws->stopped = (int*)k.take();
    ws->batch = cb; ws->restart = cr; ws->n = n; ws->nchunk = (int)nchunk;
    return HN_OK;
}

// The restart cycle's launches, the workspace prepared.  tol_dev / pre_stopped: see SmallArgs (nullptr: hn_gmres_cycle, whose bits they leave alone --
// the comparison est < tol is the same one on the same doubles); x, rhs and the outputs may lie in a workspace of the library's.  pc: the flexible
// cycle's preconditioner (its workspace prepared when pc.iters > 0); the operator input then holds z_k while A is applied and v_{k+1} after k_scale.
// op: Op::Adjoint runs the same cycle on A^H (and, with pc.iters > 0, needs ctx->adjw prepared and, for a variable-density medium, pc.rho);
// Op::Forward is every launch and argument of before.
int launch_cycle(hn_ctx* ctx, Op op, float* x, const Medium& m, const float* rhs, int rhs_batch, int batch, int restart, double tol,
                 const double* tol_dev, const int* pre_stopped, const Precond& pc, float* basis, float* hess, float* rmse, int32_t* k_used, hipStream_t s) {
    const KrylovWs& ws = *ctx->kry;
    const long P = (long)ws.n * ws.n;
    int rc;
    // the partial-sum table is indexed with the CALL's restart and batch: a workspace sized for more holds it
    const int nchunk = ws.nchunk;
    const dim3 grid(nchunk, batch), blk(256);
    SmallArgs a{ws.part, ws.npart, ws.scale, ws.g, ws.cs, ws.R, ws.y, ws.stopped, hess, rmse, k_used, batch, restart, nchunk,
                tol, 1.0 / sqrt(2.0 * (double)P), tol_dev, pre_stopped};
    const bool adj = op == Op::Adjoint;
    // w = A x - rhs = -r; A^H comes without a source operand
    if (adj) {
        if ((rc = spec_backward(ctx, pc.who, m, x, ws.w, nullptr, batch, s)) != HN_OK) return rc;
        hipLaunchKernelGGL(k_minus_rhs, grid, blk, 0, s, ws.w, rhs, rhs_batch == 1 ? 0L : 2 * P, ws.npart, P, nchunk);
    } else {
        if ((rc = spec_forward(ctx, pc.who, m, x, ws.w, rhs, rhs_batch, batch, nullptr, s)) != HN_OK) return rc;
        hipLaunchKernelGGL(k_norm_part, grid, blk, 0, s, ws.w, ws.npart, P, nchunk);
    }
    hipLaunchKernelGGL(k_small_init, dim3(batch), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_scale, grid, blk, 0, s, ws.w, ws.scale, -1.f, ws.vin, basis, P, 0, restart);
    for (int k = 0; k < restart; ++k) {
        if (pc.zbasis != nullptr && pc.iters > 0) {
            const PrecondWs& p = *ctx->pcw;
            if (adj && pc.rho != nullptr) hipLaunchKernelGGL(k_seed_adj_rho, grid, blk, 0, s, ws.vin, ctx->adjw->winv, pc.rho, pc.alpha, p.src, p.res, p.wf, P);
            else if (adj) hipLaunchKernelGGL(k_seed_adj, grid, blk, 0, s, ws.vin, ctx->adjw->winv, pc.alpha, p.src, p.res, p.wf, P);
            else hipLaunchKernelGGL(k_seed, grid, blk, 0, s, ws.vin, pc.alpha, p.src, p.res, p.wf, P);
            if ((rc = zero_async(ctx, p.states, sizeof(float) * (size_t)batch * kState * (size_t)p.state_len, s)) != HN_OK) return rc;
            rc = step_entry(ctx, m.step_name(), p.wf, p.res, p.states, m, p.src, batch, batch, pc.iters, nullptr, nullptr, nullptr, nullptr, s);
            if (rc != HN_OK) return step_named(ctx, pc.who, rc);
            if (adj && pc.rho != nullptr)
                hipLaunchKernelGGL(k_take_adj_rho, grid, blk, 0, s, p.wf, ctx->adjw->w, pc.rho, pc.alpha, ws.vin, pc.zbasis, P, k, restart);
            else if (adj) hipLaunchKernelGGL(k_take_adj, grid, blk, 0, s, p.wf, ctx->adjw->w, pc.alpha, ws.vin, pc.zbasis, P, k, restart);
            else hipLaunchKernelGGL(k_take, grid, blk, 0, s, p.wf, pc.alpha, ws.vin, pc.zbasis, P, k, restart);
        } else if (pc.zbasis != nullptr) {
            hipLaunchKernelGGL(k_take_copy, grid, blk, 0, s, ws.vin, pc.zbasis, P, k, restart);
        }
        rc = adj ? spec_backward(ctx, pc.who, m, ws.vin, ws.w, nullptr, batch, s) : spec_forward(ctx, pc.who, m, ws.vin, ws.w, ws.zero, 1, batch, nullptr, s);
        if (rc != HN_OK) return rc;
        hipLaunchKernelGGL(k_dots, grid, blk, 0, s, ws.w, basis, ws.part, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_sub<0>, grid, blk, 0, s, ws.w, basis, ws.part, ws.npart, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_sub<1>, grid, blk, 0, s, ws.w, basis, ws.part, ws.npart, P, k, restart, nchunk);
        hipLaunchKernelGGL(k_small, dim3(batch), dim3(64), 0, s, a, k);
        hipLaunchKernelGGL(k_scale, grid, blk, 0, s, ws.w, ws.scale, 1.f, ws.vin, basis, P, k + 1, restart);
    }
    if (pc.zbasis != nullptr) hipLaunchKernelGGL(k_update, grid, blk, 0, s, x, pc.zbasis, ws.y, k_used, P, restart, restart);
    else hipLaunchKernelGGL(k_update, grid, blk, 0, s, x, basis, ws.y, k_used, P, restart, restart + 1);
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

// ---- iterative refinement around the cycle (hn_gmres_refine_cycle): r = b - A x and x += s d in float64, A d = r / s by the fp32 cycle above ----
// The three kernels below stream: a thread owns four consecutive pixels of a plane, a block 1024 pixels of a sample, as the cycle's kernels do.  A float4
// of fp32 stands against TWO double2 of float64, so that every access is 16 bytes on both sides (one double2 per float2 would halve the fp32 access).
// None of them sums anything: the one sum of a refinement step, rmse64, is hn_residual_f64's own (k_helm_f64's per-tile sums, k_rmse_f64's fixed tree), launched
// as hn_residual_f64 launches it, because the caller compares it bit for bit with that entry point's -- a block-order sum of the tile table by every
// consumer block would be a second order of summation (and up to 4096 table reads per block).  s travels as rmse64[b], a device word.

// float -> double, exactly: quad i of k_sq for i < nk4, then quad i - nk4 of rhs
__global__ __launch_bounds__(256) void k_refine_upcast(const float* __restrict__ ksq, double* __restrict__ ksq64, long nk4, const float* __restrict__ rhs,
                                                       double* __restrict__ rhs64, long nr4) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const float* src = ksq;
    double* dst = ksq64;
    if (i >= nk4) {
        i -= nk4;
        if (i >= nr4) return;
        src = rhs;
        dst = rhs64;
    }
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    reinterpret_cast<double2*>(dst)[2 * i] = make_double2((double)v.x, (double)v.y);
    reinterpret_cast<double2*>(dst)[2 * i + 1] = make_double2((double)v.z, (double)v.w);
}

__device__ __forceinline__ float4 scaled_down(const double* p, double s) {   // fp32(-p / s): a true division, the value the caller can form itself
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    return make_float4((float)(-a.x / s), (float)(-a.y / s), (float)(-b.x / s), (float)(-b.y / s));
}

// rhs32 = fp32(-res / s), d32 = 0, and per sample the inner tolerance and the float64 stop; s = max(rmse64, 1e-300)
__global__ __launch_bounds__(256) void k_refine_rhs(const double* __restrict__ res, const double* __restrict__ rmse64, double tol, double inner_floor,
                                                    float* __restrict__ rhs32, float* __restrict__ d32, double* __restrict__ tol_dev,
                                                    int* __restrict__ stop, long P) {
    const int b = blockIdx.y;
    const double r = rmse64[b];
    const double s = fmax(r, 1e-300);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        tol_dev[b] = fmax(tol / s, inner_floor);
        stop[b] = (r < tol || r == 0.0) ? 1 : 0;   // a residual of exactly zero: nothing to correct, whatever the tolerance
    }
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (off >= P) return;
    const long at = (long)b * 2 * P + off;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(rhs32 + at) = scaled_down(res + at, s);
    *reinterpret_cast<float4*>(rhs32 + at + P) = scaled_down(res + at + P, s);
    *reinterpret_cast<float4*>(d32 + at) = z;
    *reinterpret_cast<float4*>(d32 + at + P) = z;
}

__device__ __forceinline__ void add_scaled(double* p, float4 d, double s) {
    double2 a = reinterpret_cast<double2*>(p)[0], b = reinterpret_cast<double2*>(p)[1];
    a.x += s * (double)d.x; a.y += s * (double)d.y; b.x += s * (double)d.z; b.y += s * (double)d.w;
    reinterpret_cast<double2*>(p)[0] = a;
    reinterpret_cast<double2*>(p)[1] = b;
}

// x += s * d in float64; a sample with k_used == 0 is not written
__global__ __launch_bounds__(256) void k_refine_update(double* __restrict__ x, const float* __restrict__ d32, const double* __restrict__ rmse64,
                                                       const int32_t* __restrict__ k_used, long P) {
    const int b = blockIdx.y;
    const long off = (long)blockIdx.x * kKryChunk + threadIdx.x * 4;
    if (k_used[b] <= 0 || off >= P) return;
    const double s = fmax(rmse64[b], 1e-300);
    const long at = (long)b * 2 * P + off;
    add_scaled(x + at, *reinterpret_cast<const float4*>(d32 + at), s);
    add_scaled(x + at + P, *reinterpret_cast<const float4*>(d32 + at + P), s);
}

void refine_ws_free(hn_ctx* ctx) {
    if (ctx->rfn == nullptr) return;
    ctx->rfn->block.free();
    delete ctx->rfn;
    ctx->rfn = nullptr;
}

// the refinement's own fields for `batch` samples on the current domain -- never built or grown under stream capture
int refine_prepare(hn_ctx* ctx, int batch, hipStream_t s, bool lossy) {
    const int n = ctx->tab.n;
    RefineWs* ws = ctx->rfn;
    if (ws != nullptr && ws->n == n && batch <= ws->batch && (!lossy || ws->ksq_im64 != nullptr)) return HN_OK;
    if (ws != nullptr && ws->n == n) {   // a rebuilt workspace keeps what the old one could do
        lossy = lossy || ws->ksq_im64 != nullptr;
        batch = batch > ws->batch ? batch : ws->batch;
    }
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "hn_gmres_refine_cycle: the workspace (or a larger batch's) is built by the first call, which must not be under stream capture");
    refine_ws_free(ctx);
    ws = new (std::nothrow) RefineWs();
    if (!ws) return fail(ctx, HN_ERR_NOMEM, "out of host memory");
    ctx->rfn = ws;
    const size_t P = (size_t)n * n, B = (size_t)batch;
    const size_t sizes[] = {B * P * 8, B * 2 * P * 8, B * 2 * P * 8, B * 2 * P * 4, B * 2 * P * 4, B * 8, B * 4, B * P * 8};
    DeviceBlock& k = ws->block;
    if (const int rc = k.alloc(ctx, "hn_gmres_refine_cycle", sizes, lossy ? 8 : 7); rc != HN_OK) { refine_ws_free(ctx); return rc; }
    ws->ksq64 = (double*)k.take(); ws->rhs64 = (double*)k.take(); ws->res64 = (double*)k.take(); ws->rhs32 = (float*)k.take(); ws->d32 = (float*)k.take();
    ws->tol = (double*)k.take(); ws->stop = (int*)k.take();
    if (lossy) ws->ksq_im64 = (double*)k.take();
    ws->batch = batch; ws->n = n;
    return HN_OK;
}

// What the cycle entry points refuse alike, under the entry point's name: x fp32 and rmse64 NULL for the plain cycles, x float64 for the refinements;
// zbasis NULL for the two without a preconditioner, required for the flexible ones; the medium's k_sq_im and rho_grad where it has them.  Any two arguments
// that overlap are refused, read against read too (every range counts as written); the medium's extra planes stand first in the table, so that they are
// the ones named first ("k_sq_im overlaps basis").  hn_gmres_cycle reports a missing domain with HN_ERR_ARG, the others with HN_ERR_STATE, and a caller may
// rely on either: a known wart.
int check_cycle_args(hn_ctx* ctx, const char* who, bool refine, bool flexible, const void* x, const Medium& m, const float* rhs, int rhs_batch, int batch,
                     int restart, const float* basis, const float* zbasis, const float* hess, const float* rmse, const int32_t* k_used, const double* rmse64,
                     const float* rho = nullptr) {
    if (!ctx || !x || !m.k_sq || !rhs || !basis || !hess || !rmse || !k_used || (refine && !rmse64) || (flexible && !zbasis))
        return fail(ctx, HN_ERR_ARG, "%s: NULL argument", who);
    if (ctx->rect) return rect_unsupported(ctx, who);
    if (ctx->tab.n == 0) return fail(ctx, refine || flexible ? HN_ERR_STATE : HN_ERR_ARG, "%s: hn_set_domain has not been called", who);
    if (batch < 1) return fail(ctx, HN_ERR_ARG, "%s: batch must be positive (got %d)", who, batch);
    if (restart < 1 || restart > kKryMaxRestart) return fail(ctx, HN_ERR_ARG, "%s: restart %d outside [1, %d]", who, restart, kKryMaxRestart);
    if (rhs_batch != 1 && rhs_batch != batch) return fail(ctx, HN_ERR_ARG, "%s: rhs batch %d must be 1 or equal to the batch %d", who, rhs_batch, batch);
    const size_t P = (size_t)ctx->tab.n * ctx->tab.n, B = (size_t)batch, R = (size_t)restart;
    const MemRange r[] = {{m.k_sq_im, B * P * 4, true, "k_sq_im"}, {m.rho_grad, B * 2 * P * 4, true, "rho_grad"}, {rho, B * P * 4, true, "rho"},
                          {x, B * 2 * P * (refine ? 8 : 4), true, "x"}, {m.k_sq, B * P * 4, true, "k_sq"}, {rhs, (size_t)rhs_batch * 2 * P * 4, true, "rhs"},
                          {basis, B * (R + 1) * 2 * P * 4, true, "basis"}, {zbasis, B * R * 2 * P * 4, true, "zbasis"},
                          {hess, B * (R + 1) * R * 2 * 4, true, "hess"}, {rmse, (R + 1) * B * 4, true, "rmse"}, {k_used, B * 4, true, "k_used"},
                          {rmse64, B * 8, true, "rmse64"}};
    for (int i = 0; i < 8; ++i)   // the fields are read and written as float4 (x of the refinement: as double2); a NULL one is aligned
        if (reinterpret_cast<uintptr_t>(r[i].p) % 16 != 0) return fail(ctx, HN_ERR_ARG, "%s: %s is not 16-byte aligned", who, r[i].name);
    if (reinterpret_cast<uintptr_t>(rmse64) % 8 != 0) return fail(ctx, HN_ERR_ARG, "%s: rmse64 is not 8-byte aligned", who);
    const char *na, *nb;
    if (first_overlap(r, 12, &na, &nb)) return fail(ctx, HN_ERR_ARG, "%s: %s overlaps %s", who, na, nb);
    return HN_OK;
}

// What the flexible entry points refuse beyond check_cycle_args, and the preconditioner's workspace: nothing is enqueued before this has passed.
// Not capturable: hn_step's first call on a new stream probes its side stream and synchronises.
int check_precond(hn_ctx* ctx, const char* who, int precond_iters, float precond_scale, const Medium& m, int batch, hipStream_t s) {
    if (precond_iters < 0) return fail(ctx, HN_ERR_ARG, "%s: precond_iters must be >= 0 (got %d)", who, precond_iters);
    if (!(precond_scale > 0.f) || !(precond_scale <= 3.402823466e38f))
        return fail(ctx, HN_ERR_ARG, "%s: precond_scale must be finite and > 0 (got %g)", who, (double)precond_scale);
    if (stream_capturing(s)) return fail(ctx, HN_ERR_STATE, "%s: not capturable (the preconditioner calls hn_step, whose first call on a stream synchronises)", who);
    if (precond_iters == 0) return HN_OK;
    if (!ctx->have_weights) return fail(ctx, HN_ERR_STATE, "%s: hn_load_weights has not been called (precond_iters %d needs the network)", who, precond_iters);
    return precond_prepare(ctx, who, m, batch, s);
}

// the plain and the flexible cycles, the arguments checked
int run_cycle(hn_ctx* ctx, Op op, float* x, const Medium& m, const float* rhs, int rhs_batch, int batch, int restart, float tol, const Precond& pc, float* basis,
              float* hess, float* rmse, int32_t* k_used, hipStream_t s) {
    if (const int rc = prepare(ctx, batch, restart, s); rc != HN_OK) return rc;
    return launch_cycle(ctx, op, x, m, rhs, rhs_batch, batch, restart, (double)tol, nullptr, nullptr, pc, basis, hess, rmse, k_used, s);
}

// the refinement steps, the arguments but tol and inner_floor checked; a lossy medium: the lossy operator in the float64 residual, the cycle and the
// preconditioner
int run_refine_cycle(hn_ctx* ctx, double* x, const Medium& m, const float* rhs, int rhs_batch, int batch, int restart, double tol,
                     float inner_floor, const Precond& pc, float* basis, float* hess, float* rmse, int32_t* k_used, double* rmse64, hipStream_t s) {
    const long P = (long)ctx->tab.n * ctx->tab.n;
    // all three workspaces before the first launch: a call that has to build one under capture leaves nothing behind
    int rc = prepare(ctx, batch, restart, s);
    const bool lossy = m.k_sq_im != nullptr;
    if (rc == HN_OK) rc = refine_prepare(ctx, batch, s, lossy);
    if (rc == HN_OK) rc = lossy ? f64_lossy_reserve(ctx, batch, true, s) : f64_reserve(ctx, batch, true, s);
    if (rc != HN_OK) return rc;
    const RefineWs& ws = *ctx->rfn;
    const long nk4 = (long)batch * P / 4, nr4 = (long)rhs_batch * 2 * P / 4;   // (n is a multiple of 16)
    const dim3 grid(ctx->kry->nchunk, batch), blk(256);
    hipLaunchKernelGGL(k_refine_upcast, dim3((unsigned)((nk4 + nr4 + 255) / 256)), blk, 0, s, m.k_sq, ws.ksq64, nk4, rhs, ws.rhs64, nr4);
    if (lossy) {
        hipLaunchKernelGGL(k_refine_upcast, dim3((unsigned)((nk4 + 255) / 256)), blk, 0, s, m.k_sq_im, ws.ksq_im64, nk4, nullptr, nullptr, 0L);
        rc = f64_apply_lossy(ctx, x, ws.res64, ws.ksq64, ws.ksq_im64, ws.rhs64, rhs_batch, rmse64, batch, s);
    } else {
        rc = f64_apply(ctx, x, ws.res64, ws.ksq64, ws.rhs64, rhs_batch, rmse64, batch, s);
    }
    if (rc != HN_OK) return rc;
    hipLaunchKernelGGL(k_refine_rhs, grid, blk, 0, s, ws.res64, rmse64, tol, (double)inner_floor, ws.rhs32, ws.d32, ws.tol, ws.stop, P);
    if ((rc = launch_cycle(ctx, Op::Forward, ws.d32, m, ws.rhs32, batch, batch, restart, 0.0, ws.tol, ws.stop, pc, basis, hess, rmse, k_used, s)) != HN_OK) return rc;
    hipLaunchKernelGGL(k_refine_update, grid, blk, 0, s, x, ws.d32, rmse64, k_used, P);
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

int check_refine_tols(hn_ctx* ctx, const char* who, double tol, float inner_floor) {
    if (!(tol >= 0.0)) return fail(ctx, HN_ERR_ARG, "%s: tol must be a number >= 0 (got %g)", who, tol);
    if (!(inner_floor >= 0.f)) return fail(ctx, HN_ERR_ARG, "%s: inner_floor must be a number >= 0 (got %g)", who, (double)inner_floor);
    return HN_OK;
}

}  // namespace

void krylov_free(hn_ctx* ctx) {
    cycle_ws_free(ctx);
    refine_ws_free(ctx);
    precond_ws_free(ctx);
    adjoint_w_free(ctx);
}
void precond_free(hn_ctx* ctx) { precond_ws_free(ctx); }

}  // namespace hn

using namespace hn;

// hn_gmres_cycle, hn_fgmres_cycle[_lossy|_medium] and hn_fgmres_adjoint_cycle[_lossy|_medium] behind their own NULL refusals; rho: the last one's
static int cycle_entry(hn_ctx* ctx, const char* who, Op op, bool flexible, float* x, const Medium& m, const float* rhs, int rhs_batch, int batch, int restart,
                       float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used, void* stream,
                       const float* rho = nullptr) {
    int rc = check_cycle_args(ctx, who, false, flexible, x, m, rhs, rhs_batch, batch, restart, basis, zbasis, hess, rmse, k_used, nullptr, rho);
    if (rc != HN_OK) return rc;
    if (op == Op::Adjoint && m.kind() == Medium::Kind::Density && precond_iters > 0 && rho == nullptr)
        return fail(ctx, HN_ERR_ARG, "%s: rho is NULL (precond_iters %d: the preconditioner's similarity weight is W / rho; only precond_iters 0 runs without)", who,
                    precond_iters);
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (!flexible) return run_cycle(ctx, op, x, m, rhs, rhs_batch, batch, restart, tol, Precond{}, basis, hess, rmse, k_used, s);
    if ((rc = check_precond(ctx, who, precond_iters, precond_scale, m, batch, s)) != HN_OK) return rc;
    // (precond_iters 0 has not asked step_entry for the tables)
    if (m.kind() != Medium::Kind::Lossless && (rc = spec_lossy_reserve(ctx, who, s)) != HN_OK) return rc;
    if (op == Op::Adjoint && precond_iters > 0 && (rc = adjoint_w_prepare(ctx, who)) != HN_OK) return rc;
    return run_cycle(ctx, op, x, m, rhs, rhs_batch, batch, restart, tol, Precond{zbasis, precond_iters, precond_scale, who, precond_iters > 0 ? rho : nullptr},
                     basis, hess, rmse, k_used, s);
}

extern "C" int hn_gmres_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                              float* basis, float* hess, float* rmse, int32_t* k_used, void* stream) {
    return cycle_entry(ctx, "hn_gmres_cycle", Op::Forward, false, x, Medium{k_sq}, rhs, rhs_batch, batch, restart, tol, 0, 1.f, basis, nullptr, hess, rmse, k_used,
                       stream);
}

extern "C" int hn_fgmres_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                               int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used,
                               void* stream) {
    return cycle_entry(ctx, "hn_fgmres_cycle", Op::Forward, true, x, Medium{k_sq}, rhs, rhs_batch, batch, restart, tol, precond_iters, precond_scale, basis, zbasis,
                       hess, rmse, k_used, stream);
}

extern "C" int hn_fgmres_cycle_lossy(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch, int restart,
                                     float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse,
                                     int32_t* k_used, void* stream) {
    if (ctx && !k_sq_im) return fail(ctx, HN_ERR_ARG, "hn_fgmres_cycle_lossy: k_sq_im is NULL (a lossless medium is hn_fgmres_cycle)");
    return cycle_entry(ctx, "hn_fgmres_cycle_lossy", Op::Forward, true, x, Medium{k_sq, k_sq_im}, rhs, rhs_batch, batch, restart, tol, precond_iters, precond_scale,
                       basis, zbasis, hess, rmse, k_used, stream);
}

extern "C" int hn_fgmres_cycle_medium(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rho_grad, const float* rhs, int rhs_batch,
                                      int batch, int restart, float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess,
                                      float* rmse, int32_t* k_used, void* stream) {
    if (ctx && !rho_grad)
        return fail(ctx, HN_ERR_ARG, "hn_fgmres_cycle_medium: rho_grad is NULL (a medium of constant density is hn_fgmres_cycle_lossy, or hn_fgmres_cycle without "
                    "absorption)");
    return cycle_entry(ctx, "hn_fgmres_cycle_medium", Op::Forward, true, x, Medium{k_sq, k_sq_im, rho_grad}, rhs, rhs_batch, batch, restart, tol, precond_iters,
                       precond_scale, basis, zbasis, hess, rmse, k_used, stream);
}

extern "C" int hn_fgmres_adjoint_cycle_lossy(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch,
                                             int restart, float tol, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess,
                                             float* rmse, int32_t* k_used, void* stream) {
    if (ctx && !k_sq_im) return fail(ctx, HN_ERR_ARG, "hn_fgmres_adjoint_cycle_lossy: k_sq_im is NULL (a lossless medium is hn_fgmres_adjoint_cycle)");
    return cycle_entry(ctx, "hn_fgmres_adjoint_cycle_lossy", Op::Adjoint, true, x, Medium{k_sq, k_sq_im}, rhs, rhs_batch, batch, restart, tol, precond_iters,
                       precond_scale, basis, zbasis, hess, rmse, k_used, stream);
}

extern "C" int hn_fgmres_adjoint_cycle_medium(hn_ctx* ctx, float* x, const float* k_sq, const float* k_sq_im, const float* rho_grad, const float* rho,
                                              const float* rhs, int rhs_batch, int batch, int restart, float tol, int precond_iters, float precond_scale,
                                              float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used, void* stream) {
    if (ctx && !rho_grad)
        return fail(ctx, HN_ERR_ARG, "hn_fgmres_adjoint_cycle_medium: rho_grad is NULL (a medium of constant density is hn_fgmres_adjoint_cycle_lossy, or "
                    "hn_fgmres_adjoint_cycle without absorption)");
    return cycle_entry(ctx, "hn_fgmres_adjoint_cycle_medium", Op::Adjoint, true, x, Medium{k_sq, k_sq_im, rho_grad}, rhs, rhs_batch, batch, restart, tol,
                       precond_iters, precond_scale, basis, zbasis, hess, rmse, k_used, stream, rho);
}

extern "C" int hn_fgmres_adjoint_cycle(hn_ctx* ctx, float* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, float tol,
                                       int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse, int32_t* k_used,
                                       void* stream) {
    return cycle_entry(ctx, "hn_fgmres_adjoint_cycle", Op::Adjoint, true, x, Medium{k_sq}, rhs, rhs_batch, batch, restart, tol, precond_iters, precond_scale, basis,
                       zbasis, hess, rmse, k_used, stream);
}

// hn_adjoint_grad (g_k_sq_im nullptr, lossy false), hn_adjoint_grad_lossy and hn_adjoint_grad_medium (medium: g_rho_grad required, lossy = g_k_sq_im given)
static int adjoint_grad_entry(hn_ctx* ctx, const char* who, bool lossy, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq,
                              float* g_k_sq_im, float* g_src, void* stream, bool medium = false, float* g_rho_grad = nullptr) {
    if (!ctx || !lambda || !u || !g_k_sq || (lossy && !g_k_sq_im) || (medium && !g_rho_grad)) return fail(ctx, HN_ERR_ARG, "%s: NULL argument", who);
    if (ctx->rect) return rect_unsupported(ctx, who);
    if (ctx->tab.n == 0) return fail(ctx, HN_ERR_STATE, "%s: hn_set_domain has not been called", who);
    if (batch < 1) return fail(ctx, HN_ERR_ARG, "%s: batch must be positive (got %d)", who, batch);
    if (src_batch != 1 && src_batch != batch) return fail(ctx, HN_ERR_ARG, "%s: src batch %d must be 1 or equal to the batch %d", who, src_batch, batch);
    const size_t P = (size_t)ctx->tab.n * ctx->tab.n, B = (size_t)batch;
    const MemRange r[] = {{lambda, B * 2 * P * 4, false, "lambda"}, {u, B * 2 * P * 4, false, "u"}, {g_k_sq, B * P * 4, true, "g_k_sq"},
                          {g_src, (size_t)src_batch * 2 * P * 4, true, "g_src"}, {g_k_sq_im, B * P * 4, true, "g_k_sq_im"},
                          {g_rho_grad, B * 2 * P * 4, true, "g_rho_grad"}};
    const int nr = medium ? 6 : lossy ? 5 : 4;   // (a NULL g_k_sq_im of the medium call is aligned and overlaps nothing)
    for (int i = 0; i < nr; ++i)   // read and written as float4; a NULL g_src is aligned
        if (reinterpret_cast<uintptr_t>(r[i].p) % 16 != 0) return fail(ctx, HN_ERR_ARG, "%s: %s is not 16-byte aligned", who, r[i].name);
    const char *na, *nb;
    if (first_overlap(r, nr, &na, &nb)) return fail(ctx, HN_ERR_ARG, "%s: %s overlaps %s", who, na, nb);
    DeviceGuard guard(ctx);
    // the line tables before the first launch: a first call under stream capture that has them to build enqueues nothing
    if (medium)
        if (const int rc = spec_lossy_reserve(ctx, who, (hipStream_t)stream); rc != HN_OK) return rc;
    const int per = (g_src != nullptr && src_batch == 1) ? batch : 1;
    const dim3 grid((unsigned)((P + kKryChunk - 1) / kKryChunk), batch / per);
    if (lossy)
        hipLaunchKernelGGL((k_adjoint_grad<float*>), grid, dim3(256), 0, (hipStream_t)stream, lambda, u, g_k_sq, g_src, (long)P, per, g_k_sq_im);
    else
        hipLaunchKernelGGL((k_adjoint_grad<>), grid, dim3(256), 0, (hipStream_t)stream, lambda, u, g_k_sq, g_src, (long)P, per);
    HN_HIP(ctx, hipGetLastError());
    if (medium) return spec_density_grad(ctx, who, lambda, u, g_rho_grad, batch, (hipStream_t)stream);
    return HN_OK;
}

extern "C" int hn_adjoint_grad_medium(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_k_sq_im,
                                      float* g_rho_grad, float* g_src, void* stream) {
    return adjoint_grad_entry(ctx, "hn_adjoint_grad_medium", g_k_sq_im != nullptr, lambda, u, src_batch, batch, g_k_sq, g_k_sq_im, g_src, stream, true,
                              g_rho_grad);
}

extern "C" int hn_adjoint_grad(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_src, void* stream) {
    return adjoint_grad_entry(ctx, "hn_adjoint_grad", false, lambda, u, src_batch, batch, g_k_sq, nullptr, g_src, stream);
}

extern "C" int hn_adjoint_grad_lossy(hn_ctx* ctx, const float* lambda, const float* u, int src_batch, int batch, float* g_k_sq, float* g_k_sq_im,
                                     float* g_src, void* stream) {
    return adjoint_grad_entry(ctx, "hn_adjoint_grad_lossy", true, lambda, u, src_batch, batch, g_k_sq, g_k_sq_im, g_src, stream);
}

// hn_gmres_refine_cycle and hn_fgmres_refine_cycle[_lossy] behind their own NULL refusals
static int refine_entry(hn_ctx* ctx, const char* who, bool flexible, double* x, const Medium& m, const float* rhs, int rhs_batch, int batch, int restart,
                        double tol, float inner_floor, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse,
                        int32_t* k_used, double* rmse64, void* stream) {
    int rc = check_cycle_args(ctx, who, true, flexible, x, m, rhs, rhs_batch, batch, restart, basis, zbasis, hess, rmse, k_used, rmse64);
    if (rc == HN_OK) rc = check_refine_tols(ctx, who, tol, inner_floor);
    if (rc != HN_OK) return rc;
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (!flexible) return run_refine_cycle(ctx, x, m, rhs, rhs_batch, batch, restart, tol, inner_floor, Precond{}, basis, hess, rmse, k_used, rmse64, s);
    if ((rc = check_precond(ctx, who, precond_iters, precond_scale, m, batch, s)) != HN_OK) return rc;
    // (precond_iters 0 has not asked step_entry for the tables)
    if (m.kind() != Medium::Kind::Lossless && (rc = spec_lossy_reserve(ctx, who, s)) != HN_OK) return rc;
    return run_refine_cycle(ctx, x, m, rhs, rhs_batch, batch, restart, tol, inner_floor, Precond{zbasis, precond_iters, precond_scale, who}, basis, hess, rmse,
                            k_used, rmse64, s);
}

extern "C" int hn_gmres_refine_cycle(hn_ctx* ctx, double* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, double tol,
                                     float inner_floor, float* basis, float* hess, float* rmse, int32_t* k_used, double* rmse64, void* stream) {
    return refine_entry(ctx, "hn_gmres_refine_cycle", false, x, Medium{k_sq}, rhs, rhs_batch, batch, restart, tol, inner_floor, 0, 1.f, basis, nullptr, hess, rmse,
                        k_used, rmse64, stream);
}

extern "C" int hn_fgmres_refine_cycle(hn_ctx* ctx, double* x, const float* k_sq, const float* rhs, int rhs_batch, int batch, int restart, double tol,
                                      float inner_floor, int precond_iters, float precond_scale, float* basis, float* zbasis, float* hess, float* rmse,
                                      int32_t* k_used, double* rmse64, void* stream) {
    return refine_entry(ctx, "hn_fgmres_refine_cycle", true, x, Medium{k_sq}, rhs, rhs_batch, batch, restart, tol, inner_floor, precond_iters, precond_scale, basis,
                        zbasis, hess, rmse, k_used, rmse64, stream);
}

extern "C" int hn_fgmres_refine_cycle_lossy(hn_ctx* ctx, double* x, const float* k_sq, const float* k_sq_im, const float* rhs, int rhs_batch, int batch,
                                            int restart, double tol, float inner_floor, int precond_iters, float precond_scale, float* basis,
                                            float* zbasis, float* hess, float* rmse, int32_t* k_used, double* rmse64, void* stream) {
    if (ctx && !k_sq_im) return fail(ctx, HN_ERR_ARG, "hn_fgmres_refine_cycle_lossy: k_sq_im is NULL (a lossless medium is hn_fgmres_refine_cycle)");
    return refine_entry(ctx, "hn_fgmres_refine_cycle_lossy", true, x, Medium{k_sq, k_sq_im}, rhs, rhs_batch, batch, restart, tol, inner_floor, precond_iters,
                        precond_scale, basis, zbasis, hess, rmse, k_used, rmse64, stream);
}
