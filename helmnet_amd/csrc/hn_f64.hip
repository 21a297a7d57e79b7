// hn_f64.hip -- the Helmholtz residual operator in float64: the check the fp32 residual (hn_spectral.hip) is measured against.
//
//   L(u) = ax . D1x u + bx . D2x u + ay . D1y u + by . D2y u        (spectral.py:31-79 under .double())
//   res  = L(u) + k_sq . u - src                                    (hybridnet.py:544-556)
//
// Absorbing media (hn_residual_f64_lossy: res = L(u) + (k_sq + i k_sq_im) . u - src, square and rectangular domains) have no dense form: f64_apply_lossy
// always runs the line transforms of hn_f64_fft.hip.
// ONE dense code path for every legal n (the default; HN_OPT_F64_FFT 1 routes f64_reserve / f64_apply to the line transforms of hn_f64_fft.hip instead).  D1 = F^-1 diag(i k) F and D2 = F^-1 diag(-k^2) F are circulant, D[j][m] = g[(j - m) mod n], so an axis'
// operator is its first column: g2 real, g1 real but for the Nyquist term (the reference keeps k = -pi there, which makes Im g1[d] = k1[n/2] (-1)^d / n).
// The kernel keeps Re g1, Im g1 and g2 in LDS (24 n bytes) and reads matrix elements from there; only the wavefield is streamed.  The values are the
// reference's: the fp32 wavenumber grid with its fp32 square and the fp32-rounded PML coefficients, carried and applied in float64.
//
// Per 32 x 32 output tile (four waves, one 16 x 16 sub-tile each; n is a multiple of 16, so a sub-tile is inside the domain or outside it as a whole):
// both axes' products on v_mfma_f64_16x16x4_f64 -- six per k-step of 4 (D1 complex x u complex: four, D2 real x u complex: two) --, the PML combine of the
// first axis between the two k loops, the second axis' combine, k_sq . u - src and the tile's sum of squares in the epilogue.  The result is written once.
// The f64 matrix instruction runs at the rate of v_fma_f64 on this chip; it is used because one operand pair read from LDS feeds 16 FMAs per lane, which a
// vector-FMA kernel only reaches with a 4 x 4 register tile per lane and the LDS traffic of one.
//
// RMSE: per-tile sums in a table, one block per sample adds them in a fixed order.  No atomics, bit-reproducible.
#include "hn_internal.h"

namespace hn {
namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int kTile = 32;          // output tile and k chunk
constexpr int kLd = kTile + 2;     // row stride of the staged wavefield tile (doubles): the 16 rows x 2 k of a half-wave's A read fall on distinct banks

inline size_t f64_lds_bytes(int n) { return sizeof(double) * ((size_t)3 * n + 2 * kTile * kLd + 4); }

__device__ __forceinline__ d4 mma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// su[p][r][c] = u[p][r0 + r][c0 + c] (zero outside the domain), p = re / im
__device__ __forceinline__ void stage_tile(double* su, const double* u, int n, int r0, int c0) {
    const long plane = (long)n * n;
    for (int e = threadIdx.x; e < 2 * kTile * kTile; e += 256) {
        const int p = e >> 10, r = (e >> 5) & 31, c = e & 31;
        const bool in = r0 + r < n && c0 + c < n;
        su[(p * kTile + r) * kLd + c] = in ? u[p * plane + (long)(r0 + r) * n + c0 + c] : 0.0;
    }
}

// tab: Re g1 [n], Im g1 [n], g2 [n], a [n] (re, im), b [n] (re, im).  out nullable; part nullable: [batch][tiles] sums of out^2 over a tile.
template <bool RESID>
__global__ __launch_bounds__(256) void k_helm_f64(const double* __restrict__ wf, double* __restrict__ out, const double* __restrict__ ksq,
                                                  const double* __restrict__ src, long src_sb, const double* __restrict__ tab, int n,
                                                  double* __restrict__ part) {
    extern __shared__ double lds[];
    double* g1r = lds;
    double* g1i = lds + n;
    double* g2 = lds + 2 * n;
    double* su = lds + 3 * n;
    double* red = su + 2 * kTile * kLd;
    const double* ca = tab + 3 * n;
    const double* cb = tab + 5 * n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int b = blockIdx.z, i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int ri = i0 + (wave >> 1) * 16, cj = j0 + (wave & 1) * 16;   // this wave's 16 x 16 sub-tile
    const bool live = ri < n && cj < n;
    const long plane = (long)n * n;
    const double* u = wf + (long)b * 2 * plane;
    for (int t = tid; t < 3 * n; t += 256) lds[t] = tab[t];

    // ---- along W: X[i][j] = sum_m u[i][m] D[j][m]; A = u (rows i, k = m), B[k][j] = g[(j - m) mod n] ----
    d4 x1r = {0, 0, 0, 0}, x1i = x1r, x2r = x1r, x2i = x1r;
    for (int m0 = 0; m0 < n; m0 += kTile) {
        __syncthreads();
        stage_tile(su, u, n, i0, m0);
        __syncthreads();
        if (!live) continue;
        const int steps = (n - m0) >> 2 < 8 ? (n - m0) >> 2 : 8;
        const double* ar_p = su + ((wave >> 1) * 16 + li) * kLd + lk;
        for (int kk = 0; kk < steps; ++kk) {
            const double ar = ar_p[kk * 4], ai = ar_p[kTile * kLd + kk * 4];
            int d = cj + li - (m0 + kk * 4 + lk);
            d += d < 0 ? n : 0;
            const double b1r = g1r[d], b1i = g1i[d], b2 = g2[d];
            x1r = mma(ar, b1r, x1r);
            x1i = mma(ai, b1r, x1i);
            x2r = mma(ar, b2, x2r);
            x2i = mma(ai, b2, x2i);
            x1r = mma(ai, -b1i, x1r);
            x1i = mma(ar, b1i, x1i);
        }
    }
    // result r of a lane: row (lane >> 4) + 4 r, column lane & 15
    const int col = cj + li;
    double acc_re[4] = {0, 0, 0, 0}, acc_im[4] = {0, 0, 0, 0};
    if (live) {
        const double ar = ca[2 * col], ai = ca[2 * col + 1], br = cb[2 * col], bi = cb[2 * col + 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc_re[r] = ar * x1r[r] - ai * x1i[r] + br * x2r[r] - bi * x2i[r];
            acc_im[r] = ar * x1i[r] + ai * x1r[r] + br * x2i[r] + bi * x2r[r];
        }
    }

    // ---- along H: Y[i][j] = sum_m D[i][m] u[m][j]; A[i][k] = g[(i - m) mod n], B = u (k = m, columns j) ----
    d4 y1r = {0, 0, 0, 0}, y1i = y1r, y2r = y1r, y2i = y1r;
    for (int m0 = 0; m0 < n; m0 += kTile) {
        __syncthreads();
        stage_tile(su, u, n, m0, j0);
        __syncthreads();
        if (!live) continue;
        const int steps = (n - m0) >> 2 < 8 ? (n - m0) >> 2 : 8;
        const double* br_p = su + lk * kLd + (wave & 1) * 16 + li;
        for (int kk = 0; kk < steps; ++kk) {
            const double br = br_p[kk * 4 * kLd], bi = br_p[kTile * kLd + kk * 4 * kLd];
            int d = ri + li - (m0 + kk * 4 + lk);
            d += d < 0 ? n : 0;
            const double a1r = g1r[d], a1i = g1i[d], a2 = g2[d];
            y1r = mma(a1r, br, y1r);
            y1i = mma(a1r, bi, y1i);
            y2r = mma(a2, br, y2r);
            y2i = mma(a2, bi, y2i);
            y1r = mma(-a1i, bi, y1r);
            y1i = mma(a1i, br, y1i);
        }
    }
    double sq = 0.0;
    if (live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ri + lk + 4 * r;
            const double ar = ca[2 * row], ai = ca[2 * row + 1], br = cb[2 * row], bi = cb[2 * row + 1];
            double re = acc_re[r] + (ar * y1r[r] - ai * y1i[r] + br * y2r[r] - bi * y2i[r]);
            double im = acc_im[r] + (ar * y1i[r] + ai * y1r[r] + br * y2i[r] + bi * y2r[r]);
            const long idx = (long)row * n + col;
            if (RESID) {
                const double kq = ksq[(long)b * plane + idx];
                const double* sp = src + (long)b * src_sb + idx;
                re += kq * u[idx] - sp[0];
                im += kq * u[plane + idx] - sp[plane];
            }
            if (out != nullptr) {
                out[(long)b * 2 * plane + idx] = re;
                out[(long)b * 2 * plane + plane + idx] = im;
            }
            sq += re * re + im * im;
        }
    }
    if (part != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        if (lane == 0) red[wave] = sq;
        __syncthreads();
        if (tid == 0) part[((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// rmse[b] = sqrt(sum over the sample's tiles / count): each thread adds its tiles in order, then a fixed tree
__global__ __launch_bounds__(256) void k_rmse_f64(const double* __restrict__ part, int tiles, double inv_count, double* __restrict__ rmse) {
    __shared__ double red[256];
    const double* p = part + (long)blockIdx.x * tiles;
    double s = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) s += p[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) rmse[blockIdx.x] = sqrt(red[0] * inv_count);
}

}  // namespace

bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return s != nullptr && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int DeviceBlock::alloc(hn_ctx* ctx, const char* who, const size_t* sizes, int count) {
    free();
    size_t total = 0;
    for (int i = 0; i < count; ++i) { offs.push_back(total); total += (sizes[i] + 255) & ~(size_t)255; }
    hipError_t e = hipMalloc((void**)&base, total);
    if (e == hipSuccess) e = hipMemset(base, 0, total);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) return HN_OK;
    free();
    return fail(ctx, e == hipErrorOutOfMemory ? HN_ERR_NOMEM : HN_ERR_HIP, "%s: workspace of %zu bytes: %s", who, total, hipGetErrorString(e));
}
void DeviceBlock::free() {
    (void)hipFree(base);
    base = nullptr;
    offs.clear();
    taken = 0;
}

bool first_overlap(const MemRange* r, int count, const char** a_name, const char** b_name) {
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j) {
            if (r[i].p == nullptr || r[j].p == nullptr || !(r[i].written || r[j].written)) continue;
            const char *a = static_cast<const char*>(r[i].p), *b = static_cast<const char*>(r[j].p);
            if (a < b + r[j].bytes && b < a + r[i].bytes) { *a_name = r[i].name; *b_name = r[j].name; return true; }
        }
    return false;
}

// the first float64 call on a domain builds and uploads the tables; a larger batch with an rmse grows the table of partial sums (one per tile and sample)
int f64_reserve(hn_ctx* ctx, int batch, bool want_rmse, hipStream_t s, bool want_out) {
    SpecTables& t = ctx->tab;
    if (t.n == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    if (ctx->opt_f64_fft) return f64_fft_reserve(ctx, batch, want_rmse, want_out, s);   // (its tables live beside the dense ones: flipping back finds them)
    const int tiles_1d = (t.n + kTile - 1) / kTile;
    const long part_needed = want_rmse ? (long)batch * tiles_1d * tiles_1d : 0;
    if (t.f64_tab != nullptr && part_needed <= t.f64_part_cap) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "the float64 tables of this domain (or a larger batch's partial sums) are built by the first call, which must not be under stream capture");
    if (t.f64_tab == nullptr) {
        const int n = t.n;
        const AxisHost ax = spec_axis_host(n, t.pml, t.sigma_max, t.k);
        std::vector<std::complex<double>> g1, g2;
        spec_circulant_host(ax, g1, g2);
        std::vector<double> h((size_t)7 * n);
        for (int i = 0; i < n; ++i) {
            h[i] = g1[i].real();
            h[n + i] = g1[i].imag();
            h[2 * n + i] = g2[i].real();
            h[3 * n + 2 * i] = (double)ax.fa[i].x;
            h[3 * n + 2 * i + 1] = (double)ax.fa[i].y;
            h[5 * n + 2 * i] = (double)ax.fb[i].x;
            h[5 * n + 2 * i + 1] = (double)ax.fb[i].y;
        }
        const int lds = (int)f64_lds_bytes(2048);   // the largest domain's: the attribute belongs to the kernel, not to this context
        HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_helm_f64<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_helm_f64<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        double* dev = nullptr;
        HN_HIP(ctx, hipMalloc((void**)&dev, h.size() * sizeof(double)));
        if (hipError_t e = hipMemcpy(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice); e != hipSuccess) {
            (void)hipFree(dev);
            return fail(ctx, HN_ERR_HIP, "upload of the float64 tables failed: %s", hipGetErrorString(e));
        }
        t.f64_tab = dev;
    }
    if (part_needed > t.f64_part_cap) {
        (void)hipFree(t.f64_part);   // (waits for the launches that still read it)
        t.f64_part = nullptr;
        t.f64_part_cap = 0;
        HN_HIP(ctx, hipMalloc((void**)&t.f64_part, (size_t)part_needed * sizeof(double)));
        t.f64_part_cap = part_needed;
    }
    return HN_OK;
}

int f64_apply(hn_ctx* ctx, const double* wf, double* out, const double* ksq, const double* src, int src_batch, double* rmse, int batch, hipStream_t s) {
    SpecTables& t = ctx->tab;
    if (t.n == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    const int n = t.n, tiles_1d = (n + kTile - 1) / kTile, tiles = tiles_1d * tiles_1d;
    const long plane = (long)n * n;
    const size_t bytes = (size_t)batch * 2 * plane * sizeof(double);
    const MemRange r[] = {{wf, bytes, false, "wf"}, {out, bytes, true, "out"}};
    const char *na, *nb;
    if (first_overlap(r, 2, &na, &nb)) return fail(ctx, HN_ERR_ARG, "float64 residual: the wavefield must not alias the output");
    if (int rc = f64_reserve(ctx, batch, rmse != nullptr, s, out != nullptr); rc != HN_OK) return rc;
    if (ctx->opt_f64_fft) {
        double* lines = nullptr;   // one partial sum per line: k_rmse_f64 adds a sample's n of them
        if (int rc = f64_fft_launch(ctx, wf, out, ksq, nullptr, src, src_batch == 1 ? 0L : 2 * plane, rmse != nullptr, batch, s, &lines); rc != HN_OK) return rc;
        if (rmse != nullptr) hipLaunchKernelGGL(k_rmse_f64, dim3(batch), dim3(256), 0, s, lines, n, 1.0 / (2.0 * (double)plane), rmse);
        HN_HIP(ctx, hipGetLastError());
        ctx->f64_route = 2;
        return HN_OK;
    }
    double* part = rmse != nullptr ? t.f64_part : nullptr;
    const dim3 grid(tiles_1d, tiles_1d, batch);
    const size_t lds = f64_lds_bytes(n);
    if (ksq != nullptr)
        hipLaunchKernelGGL(k_helm_f64<true>, grid, dim3(256), lds, s, wf, out, ksq, src, src_batch == 1 ? 0L : 2 * plane, t.f64_tab, n, part);
    else
        hipLaunchKernelGGL(k_helm_f64<false>, grid, dim3(256), lds, s, wf, out, ksq, src, 0L, t.f64_tab, n, part);
    if (rmse != nullptr) hipLaunchKernelGGL(k_rmse_f64, dim3(batch), dim3(256), 0, s, part, tiles, 1.0 / (2.0 * (double)plane), rmse);
    HN_HIP(ctx, hipGetLastError());
    ctx->f64_route = 1;
    return HN_OK;
}

int f64_lossy_reserve(hn_ctx* ctx, int batch, bool want_rmse, hipStream_t s, bool want_out) {
    if (ctx->geo.h == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    return f64_fft_reserve(ctx, batch, want_rmse, want_out, s);
}

// the lossy operator has no dense form: the two line passes whatever HN_OPT_F64_FFT says, on ctx->geo (a square domain's dense tables are not touched)
int f64_apply_lossy(hn_ctx* ctx, const double* wf, double* out, const double* ksq, const double* ksq_im, const double* src, int src_batch, double* rmse,
                    int batch, hipStream_t s) {
    if (ctx->geo.h == 0) return fail(ctx, HN_ERR_STATE, "hn_set_domain has not been called");
    const int h = ctx->geo.h;
    const long plane = ctx->geo.plane();
    const size_t bytes = (size_t)batch * 2 * plane * sizeof(double);
    const MemRange r[] = {{out, bytes, true, "res"}, {wf, bytes, false, "wf"}, {ksq_im, bytes / 2, false, "k_sq_im"}};
    const char *na, *nb;
    if (first_overlap(r, 3, &na, &nb)) return fail(ctx, HN_ERR_ARG, "float64 lossy residual: %s must not alias the output", nb);
    if (int rc = f64_lossy_reserve(ctx, batch, rmse != nullptr, s, out != nullptr); rc != HN_OK) return rc;
    double* lines = nullptr;   // one partial sum per row: k_rmse_f64 adds a sample's h of them
    if (int rc = f64_fft_launch(ctx, wf, out, ksq, ksq_im, src, src_batch == 1 ? 0L : 2 * plane, rmse != nullptr, batch, s, &lines); rc != HN_OK) return rc;
    if (rmse != nullptr) hipLaunchKernelGGL(k_rmse_f64, dim3(batch), dim3(256), 0, s, lines, h, 1.0 / (2.0 * (double)plane), rmse);
    HN_HIP(ctx, hipGetLastError());
    ctx->f64_route = 2;
    return HN_OK;
}

}  // namespace hn

extern "C" {

int hn_laplacian_f64(hn_ctx* ctx, const double* wf, double* out, int batch, void* stream) {
    if (!ctx || !wf || !out) return hn::fail(ctx, HN_ERR_ARG, "hn_laplacian_f64: NULL argument");
    if (ctx->rect) return hn::rect_unsupported(ctx, "hn_laplacian_f64");
    if (batch <= 0) return hn::fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    hn::DeviceGuard guard(ctx);
    return hn::f64_apply(ctx, wf, out, nullptr, nullptr, 1, nullptr, batch, (hipStream_t)stream);
}

int hn_residual_f64(hn_ctx* ctx, const double* wf, const double* k_sq, const double* src, int src_batch, double* res, double* rmse, int batch,
                    void* stream) {
    if (!ctx || !wf || !k_sq || !src) return hn::fail(ctx, HN_ERR_ARG, "hn_residual_f64: NULL argument");
    if (ctx->rect) return hn::rect_unsupported(ctx, "hn_residual_f64");
    if (!res && !rmse) return hn::fail(ctx, HN_ERR_ARG, "hn_residual_f64: res and rmse are both NULL");
    if (batch <= 0) return hn::fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    if (src_batch != 1 && src_batch != batch)
        return hn::fail(ctx, HN_ERR_ARG, "source batch %d must be 1 or equal to the batch %d", src_batch, batch);
    hn::DeviceGuard guard(ctx);
    return hn::f64_apply(ctx, wf, res, k_sq, src, src_batch, rmse, batch, (hipStream_t)stream);
}

int hn_residual_f64_lossy(hn_ctx* ctx, const double* wf, const double* k_sq, const double* k_sq_im, const double* src, int src_batch, double* res,
                          double* rmse, int batch, void* stream) {
    if (ctx && !k_sq_im) return hn::fail(ctx, HN_ERR_ARG, "hn_residual_f64_lossy: k_sq_im is NULL (a lossless medium is hn_residual_f64)");
    if (!ctx || !wf || !k_sq || !src) return hn::fail(ctx, HN_ERR_ARG, "hn_residual_f64_lossy: NULL argument");
    if (!res && !rmse) return hn::fail(ctx, HN_ERR_ARG, "hn_residual_f64_lossy: res and rmse are both NULL");
    if (batch <= 0) return hn::fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    if (src_batch != 1 && src_batch != batch)
        return hn::fail(ctx, HN_ERR_ARG, "source batch %d must be 1 or equal to the batch %d", src_batch, batch);
    hn::DeviceGuard guard(ctx);
    return hn::f64_apply_lossy(ctx, wf, res, k_sq, k_sq_im, src, src_batch, rmse, batch, (hipStream_t)stream);
}

// test aid (not part of the ABI, needs no device): the dense n x n operators the kernel's circulant columns stand for, row-major, D1 = d1_re + i d1_im
int hn_debug_f64_operators(int n, double* d1_re, double* d1_im, double* d2) {
    if (n < 16 || n > 2048 || n % 16 != 0 || !d1_re || !d1_im || !d2) return HN_ERR_ARG;
    const hn::AxisHost ax = hn::spec_axis_host(n, 1, 0.0, 1.0);
    std::vector<std::complex<double>> g1, g2;
    hn::spec_circulant_host(ax, g1, g2);
    for (int j = 0; j < n; ++j)
        for (int m = 0; m < n; ++m) {
            const int d = ((j - m) % n + n) % n;
            d1_re[(size_t)j * n + m] = g1[d].real();
            d1_im[(size_t)j * n + m] = g1[d].imag();
            d2[(size_t)j * n + m] = g2[d].real();
        }
    return HN_OK;
}

}  // extern "C"
