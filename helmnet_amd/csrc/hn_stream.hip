// hn_stream.hip -- a stream of maps solved to a tolerance: the two launches a scheduler puts between chunks of hn_step iterations so that every map
// stops on its own and its slot of the batch goes to the next map (helmnet_amd.IterativeSolver.solve_many).  The reference runs its test set batch by
// batch for a fixed iteration count (evaluate.py); solve_to_tolerance stops a batch with its WORST map.  Samples never interact and their bits do not
// depend on slot or batch, so slots can be retired and refilled freely.
//   k_stream_verdict  reads the per-iteration per-sample RMSE rows a chunk wrote and leaves one record per slot in a host-mapped table;
//   k_stream_swap     retires finished slots into the job's output rows, compacts the tail and refills slots with the next maps' start values.
// Both are byte movement: the swap moves at most (6 planes + 2 L) x 4 B x 2 per turned-over slot -- ~62 MB for all 32 slots of 256^2 --, the verdict
// n_rows x batch floats.  Neither touches UNet arithmetic, so they serve every hn_precision mode.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <limits>

#include "hn_internal.h"

namespace hn {
namespace {

constexpr int kMaxOps = 192;          // 16 B each: 3 KB of the 4 KB kernel-argument segment (the budget of hn_rows.hip); longer lists go in several launches

struct SwapArgs {
    float *wf, *res, *states, *k_sq, *src;      // the slot arrays
    const float *sos_in, *src_in;               // the job's maps [n_maps, 1, n, n] / sources [n_maps, 2, n, n]
    float *out_wf, *out_res;                    // the job's outputs [n_maps, 2, n, n]
    long plane4, state4;                        // float4s per n x n plane / per flat hidden-state row [2, L]
    int src_per_slot;                           // 1: src holds one row per slot (src_batch == batch); 0: one broadcast row
    float omega;
    hn_stream_op op[kMaxOps];
};

// k_sq of get_initials, `(omega / sos) ** 2` on a tensor: torch evaluates scalar / tensor as reciprocal(tensor) * scalar and ** 2 as x * x, all in fp32
// (correctly rounded divide: the compiler's default for HIP)
__device__ __forceinline__ float ksq_of(float sos, float omega) {
    const float q = (1.0f / sos) * omega;
    return q * q;
}
__device__ __forceinline__ float4 ksq_of(float4 c, float omega) { return make_float4(ksq_of(c.x, omega), ksq_of(c.y, omega), ksq_of(c.z, omega), ksq_of(c.w, omega)); }

// One block range per (operation, field): blockIdx.y the operation, blockIdx.z the field (0 wf, 1 res, 2 states, 3 k_sq, 4 src), float4 grid-stride over
// the field's row.  A thread retires element i of its slot BEFORE it overwrites it, and no operation of a call reads a slot another one writes (checked
// on the host), so the actions of a record happen in the documented order without any synchronisation.
// Refill: forward() starts from wf = 0, zero hidden states and res = L(0) + k_sq * 0 - src.  L is linear and every one of its terms is a product with a
// zero of the wavefield, so L(0) is +-0 and the spectral kernels' `L + k_sq * u - src` is (+0) - src exactly -- or NaN where k_sq is not finite, which
// `k_sq * 0 - src` keeps: the refilled slot holds the bits forward() starts from, with no spectral launch.
__global__ __launch_bounds__(256) void k_stream_swap(const SwapArgs a) {
    const int f = blockIdx.z;
    const hn_stream_op op = a.op[blockIdx.y];
    const long slot = op.slot, from = op.move_from, fill = op.refill_map, ret = op.retire_map;
    const long step = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    const long wf4 = 2 * a.plane4;
    if (f == 0) {          // wavefield: retire, then zero / move
        float4* d = reinterpret_cast<float4*>(a.wf) + slot * wf4;
        if (ret >= 0) {
            float4* o = reinterpret_cast<float4*>(a.out_wf) + ret * wf4;
            for (long i = i0; i < wf4; i += step) o[i] = d[i];
        }
        if (fill >= 0) {
            for (long i = i0; i < wf4; i += step) d[i] = z;
        } else if (from >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.wf) + from * wf4;
            for (long i = i0; i < wf4; i += step) d[i] = s[i];
        }
    } else if (f == 1) {   // residual: retire, then k_sq * 0 - src / move
        float4* d = reinterpret_cast<float4*>(a.res) + slot * wf4;
        if (ret >= 0 && a.out_res != nullptr) {
            float4* o = reinterpret_cast<float4*>(a.out_res) + ret * wf4;
            for (long i = i0; i < wf4; i += step) o[i] = d[i];
        }
        if (fill >= 0) {
            const float4* c = reinterpret_cast<const float4*>(a.sos_in) + fill * a.plane4;
            const float4* s = a.src_per_slot ? reinterpret_cast<const float4*>(a.src_in) + fill * wf4 : reinterpret_cast<const float4*>(a.src);
            for (long i = i0; i < wf4; i += step) {
                const float4 k = ksq_of(c[i < a.plane4 ? i : i - a.plane4], a.omega), v = s[i];
                d[i] = make_float4(k.x * 0.f - v.x, k.y * 0.f - v.y, k.z * 0.f - v.z, k.w * 0.f - v.w);
            }
        } else if (from >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.res) + from * wf4;
            for (long i = i0; i < wf4; i += step) d[i] = s[i];
        }
    } else if (f == 2) {   // hidden state, the whole flat row
        float4* d = reinterpret_cast<float4*>(a.states) + slot * a.state4;
        if (fill >= 0) {
            for (long i = i0; i < a.state4; i += step) d[i] = z;
        } else if (from >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.states) + from * a.state4;
            for (long i = i0; i < a.state4; i += step) d[i] = s[i];
        }
    } else if (f == 3) {   // k_sq
        float4* d = reinterpret_cast<float4*>(a.k_sq) + slot * a.plane4;
        if (fill >= 0) {
            const float4* c = reinterpret_cast<const float4*>(a.sos_in) + fill * a.plane4;
            for (long i = i0; i < a.plane4; i += step) d[i] = ksq_of(c[i], a.omega);
        } else if (from >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.k_sq) + from * a.plane4;
            for (long i = i0; i < a.plane4; i += step) d[i] = s[i];
        }
    } else {               // the slot's own source row (launched with src_batch == batch only)
        float4* d = reinterpret_cast<float4*>(a.src) + slot * wf4;
        if (fill >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.src_in) + fill * wf4;
            for (long i = i0; i < wf4; i += step) d[i] = s[i];
        } else if (from >= 0) {
            const float4* s = reinterpret_cast<const float4*>(a.src) + from * wf4;
            for (long i = i0; i < wf4; i += step) d[i] = s[i];
        }
    }
}

// One thread per slot walks its column of the [n_rows, batch] RMSE table in row order.
__global__ __launch_bounds__(64) void k_stream_verdict(const float* __restrict__ rmse, int n_rows, int batch, float tol, float diverge, hn_stream_verdict_rec* __restrict__ tab) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    int first = -1, bad = 0;
    float last = 0.f;
    for (int r = 0; r < n_rows; ++r) {
        last = rmse[(long)r * batch + b];
        if (!(fabsf(last) <= std::numeric_limits<float>::max()) || last > diverge) bad = 1;   // NaN fails every comparison
        if (first < 0 && last < tol) first = r;
    }
    hn_stream_verdict_rec rec;
    rec.first_below = first; rec.bad = bad; rec.last_rmse = last;
    tab[b] = rec;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int refuse_capture(hn_ctx* ctx, const char* who, hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap != hipStreamCaptureStatusNone)
        return fail(ctx, HN_ERR_STATE, "%s cannot be captured into a HIP graph (it reads host lists and hands out a host table)", who);
    return HN_OK;
}

}  // namespace

int stream_table_reserve(hn_ctx* ctx, int slots) {
    if (slots <= ctx->stream_tab_cap) return HN_OK;
    HN_HIP(ctx, hipDeviceSynchronize());   // a verdict launch may still be writing the old table
    stream_table_free(ctx);
    HN_HIP(ctx, hipHostMalloc((void**)&ctx->stream_tab, sizeof(hn_stream_verdict_rec) * (size_t)slots, hipHostMallocMapped));
    std::memset(ctx->stream_tab, 0, sizeof(hn_stream_verdict_rec) * (size_t)slots);
    HN_HIP(ctx, hipHostGetDevicePointer((void**)&ctx->stream_tab_dev, ctx->stream_tab, 0));
    ctx->stream_tab_cap = slots;
    return HN_OK;
}

void stream_table_free(hn_ctx* ctx) {
    if (ctx->stream_tab) (void)hipHostFree(ctx->stream_tab);
    ctx->stream_tab = nullptr; ctx->stream_tab_dev = nullptr; ctx->stream_tab_cap = 0;
}

}  // namespace hn

using namespace hn;

extern "C" {

int hn_stream_verdict(hn_ctx* ctx, const float* rmse_hist, int n_rows, int batch, float tol, float diverge_rmse,
                      const hn_stream_verdict_rec** host_table, void* stream) {
    if (!ctx) return HN_ERR_ARG;
    if (!rmse_hist || !host_table) return fail(ctx, HN_ERR_ARG, "hn_stream_verdict: NULL argument");
    if (n_rows < 1 || batch < 1) return fail(ctx, HN_ERR_ARG, "hn_stream_verdict: %d rows x %d slots", n_rows, batch);
    if (std::isnan(tol) || std::isnan(diverge_rmse)) return fail(ctx, HN_ERR_ARG, "hn_stream_verdict: tol / diverge_rmse is NaN");
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(ctx, "hn_stream_verdict", s); rc != HN_OK) return rc;
    if (int rc = stream_table_reserve(ctx, batch > ctx->cap_batch ? batch : ctx->cap_batch); rc != HN_OK) return rc;
    hipLaunchKernelGGL(k_stream_verdict, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, rmse_hist, n_rows, batch, tol, diverge_rmse, ctx->stream_tab_dev);
    HN_HIP(ctx, hipGetLastError());
    *host_table = ctx->stream_tab;
    return HN_OK;
}

int hn_stream_swap(hn_ctx* ctx, float* wf, float* res, float* states, float* k_sq, float* src, int src_batch, int batch,
                   int count, const hn_stream_op* ops, const float* sos_in, const float* src_in, int64_t n_maps, float omega,
                   float* out_wf, float* out_res, void* stream) {
    const char* who = "hn_stream_swap";
    if (!ctx) return HN_ERR_ARG;
    if (ctx->rect) return rect_unsupported(ctx, who);
    if (ctx->tab.n == 0 || ctx->state_len == 0) return fail(ctx, HN_ERR_STATE, "%s: hn_set_domain / hn_load_weights have not been called", who);
    if (!wf || !res || !states || !k_sq || !src || (count > 0 && !ops)) return fail(ctx, HN_ERR_ARG, "%s: NULL argument", who);
    if (batch < 1 || count < 0 || n_maps < 0) return fail(ctx, HN_ERR_ARG, "%s: batch %d, count %d, n_maps %lld", who, batch, count, (long long)n_maps);
    if (src_batch != 1 && src_batch != batch) return fail(ctx, HN_ERR_ARG, "%s: src_batch must be 1 or batch (%d), got %d", who, batch, src_batch);
    const bool per_slot = src_batch == batch && (batch > 1 || src_in != nullptr);   // one slot: a given src_in means "one source per map"
    const long plane = (long)ctx->tab.n * ctx->tab.n, L2 = 2 * (long)ctx->state_len;
    if (plane % 4 != 0 || L2 % 4 != 0) return fail(ctx, HN_ERR_ARG, "%s: rows of %ld / %ld floats are not 16-byte multiples", who, plane, L2);
    for (const void* p : {(const void*)wf, (const void*)res, (const void*)states, (const void*)k_sq, (const void*)src, (const void*)sos_in, (const void*)src_in,
                          (const void*)out_wf, (const void*)out_res})
        if (!aligned16(p)) return fail(ctx, HN_ERR_ARG, "%s: every array must be 16-byte aligned", who);
    // the whole list is checked before anything is enqueued: launches of one call run in stream order, so the rules hold across the split too
    std::vector<unsigned char> writes(batch, 0), named(batch, 0);
    std::vector<int64_t> retired;
    for (int j = 0; j < count; ++j) {
        const hn_stream_op& o = ops[j];
        if (o.slot < 0 || o.slot >= batch) return fail(ctx, HN_ERR_ARG, "%s: operation %d: slot %d outside [0, %d)", who, j, o.slot, batch);
        if (named[o.slot]) return fail(ctx, HN_ERR_ARG, "%s: operation %d: slot %d is named twice", who, j, o.slot);
        named[o.slot] = 1;
        if (o.retire_map < -1 || o.retire_map >= n_maps || o.refill_map < -1 || o.refill_map >= n_maps)
            return fail(ctx, HN_ERR_ARG, "%s: operation %d: map index outside [0, %lld)", who, j, (long long)n_maps);
        if (o.move_from < -1 || o.move_from >= batch || o.move_from == o.slot)
            return fail(ctx, HN_ERR_ARG, "%s: operation %d: move_from %d (slot %d of %d)", who, j, o.move_from, o.slot, batch);
        if (o.retire_map >= 0) {
            if (!out_wf) return fail(ctx, HN_ERR_ARG, "%s: operation %d retires a map but out_wf is NULL", who, j);
            retired.push_back(o.retire_map);
        }
        if (o.refill_map >= 0 && (!sos_in || (per_slot && !src_in))) return fail(ctx, HN_ERR_ARG, "%s: operation %d refills a slot but sos_in / src_in is NULL", who, j);
        if (o.refill_map >= 0 || o.move_from >= 0) writes[o.slot] = 1;
    }
    for (int j = 0; j < count; ++j)
        if (ops[j].move_from >= 0 && writes[ops[j].move_from])
            return fail(ctx, HN_ERR_ARG, "%s: operation %d moves slot %d, which another operation of the call writes", who, j, ops[j].move_from);
    std::sort(retired.begin(), retired.end());
    if (std::adjacent_find(retired.begin(), retired.end()) != retired.end()) return fail(ctx, HN_ERR_ARG, "%s: a map is retired twice", who);
    DeviceGuard guard(ctx);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = refuse_capture(ctx, who, s); rc != HN_OK) return rc;
    if (count == 0) return HN_OK;
    SwapArgs a{};
    a.wf = wf; a.res = res; a.states = states; a.k_sq = k_sq; a.src = src;
    a.sos_in = sos_in; a.src_in = src_in; a.out_wf = out_wf; a.out_res = out_res;
    a.plane4 = plane / 4; a.state4 = L2 / 4; a.src_per_slot = per_slot ? 1 : 0; a.omega = omega;
    long gx = (2 * a.plane4 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int c0 = 0; c0 < count; c0 += kMaxOps) {
        const int nc = count - c0 < kMaxOps ? count - c0 : kMaxOps;
        for (int j = 0; j < nc; ++j) a.op[j] = ops[c0 + j];
        hipLaunchKernelGGL(k_stream_swap, dim3((unsigned)gx, (unsigned)nc, per_slot ? 5u : 4u), dim3(256), 0, s, a);
        HN_HIP(ctx, hipGetLastError());
    }
    return HN_OK;
}

}  // extern "C"
