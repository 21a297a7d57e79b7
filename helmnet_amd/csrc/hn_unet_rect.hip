// The UNet and the solver loop on a rectangular h x w domain (hn_set_domain_rect, h != w): the rectangular branch of hn_reserve, hn_unet and hn_step.
// One stream, layer by layer, through the launchers the square path uses with (h >> d, w >> d): every one of them takes H and W apart, tiles rows by H and
// columns by W, and picks its kernel by W alone (the rectangular driver).  Never taken here: the merged level-0 launch, the deep-level kernels,
// the side stream and its device words, pipeline lanes, captured iterations, the per-domain sigma map of the input layer (it is built for n x n and does
// not exist while the domain is rectangular).  No kernel of this path waits on another workgroup.
#include "hn_internal.h"

namespace hn {
namespace {

int rect_ready(hn_ctx* ctx, int batch) {   // check_ready of hn_api.hip
    if (!ctx->have_weights) return fail(ctx, HN_ERR_STATE, "hn_load_weights has not been called");
    if (batch <= 0) return fail(ctx, HN_ERR_ARG, "batch must be positive (got %d)", batch);
    const int m = 1 << ctx->depth;
    if (ctx->rect->h % m != 0 || ctx->rect->w % m != 0)
        return fail(ctx, HN_ERR_ARG, "domain size %d x %d is not divisible by 2^depth = %d", ctx->rect->h, ctx->rect->w, m);
    return HN_OK;
}
int rect_ready_unet(hn_ctx* ctx, const char* who, int batch) {
    if (const int rc = rect_ready(ctx, batch); rc != HN_OK) return rc;
    if (ctx->precision != HN_PREC_FP32 && ctx->precision != HN_PREC_FP32_VALU) return rect_unsupported(ctx, who);   // (the 16-bit modes)
    return HN_OK;
}

}  // namespace

void rect_state_layout(hn_ctx* ctx) {
    const int depth = ctx->have_weights ? ctx->depth : 4;
    ctx->state_len = 0;
    for (int d = 0; d < depth; ++d) {
        ctx->state_off[d] = ctx->state_len;
        ctx->state_len += (int64_t)(ctx->rect->h >> d) * (ctx->rect->w >> d);
    }
}

int rect_reserve(hn_ctx* ctx, int max_batch, hipStream_t s) {
    if (const int rc = rect_ready(ctx, max_batch); rc != HN_OK) return rc;
    if (max_batch <= ctx->cap_batch && ctx->it_counter != nullptr) return HN_OK;
    if (stream_capturing(s))
        return fail(ctx, HN_ERR_STATE, "the workspace of the rectangular domain must be built or grown (batch %d) outside stream capture: call hn_reserve first", max_batch);
    HN_HIP(ctx, hipDeviceSynchronize());  // nothing may still be using the old workspace
    free_workspace(ctx);
    const int h = ctx->rect->h, w = ctx->rect->w, depth = ctx->depth;
    for (int d = 0; d <= depth; ++d) {
        const size_t bytes = sizeof(float) * (size_t)max_batch * kFeat * (h >> d) * (w >> d);
        HN_HIP(ctx, hipMalloc((void**)&ctx->buf_a[d], bytes));
        if (d < depth) HN_HIP(ctx, hipMalloc((void**)&ctx->buf_o[d], bytes));
        if (d > 0) HN_HIP(ctx, hipMalloc((void**)&ctx->buf_y[d], bytes));
    }
    HN_HIP(ctx, hipMalloc((void**)&ctx->st_tmp, sizeof(float) * (size_t)max_batch * kState * ctx->state_len));
    if (!ctx->it_counter) HN_HIP(ctx, hipMalloc((void**)&ctx->it_counter, 8 * sizeof(int)));
    if (int rc = stream_table_reserve(ctx, max_batch); rc != HN_OK) return rc;
    ctx->cap_batch = max_batch;
    return HN_OK;
}

int unet_forward_rect(hn_ctx* ctx, const UnetCall& c) {
    const int H = ctx->rect->h, W = ctx->rect->w, depth = ctx->depth, batch = c.batch, ws_off = c.ws_off;
    const hipStream_t s = c.stream;
    const long L = ctx->state_len;
    const Src none{nullptr, 0, 0, 1.f};
    const bool mfma = ctx->precision != HN_PREC_FP32_VALU;
    auto plane = [&](int d) { return (long)(H >> d) * (W >> d); };
    auto feat = [&](float* p, int d) { return Dst{p + (long)ws_off * kFeat * plane(d), kFeat * plane(d), plane(d)}; };
    auto featsrc = [&](const float* p, int d) { return Src{p + (long)ws_off * kFeat * plane(d), kFeat * plane(d), plane(d), 1.f}; };
    auto st_old = [&](int d) { return Src{c.states_in + ctx->state_off[d], 2 * L, L, 1.f}; };
    // One DoubleConv of level d: launch_dc8 (the hand-scheduled or packed-FMA kernel from W >= 256, else the matrix-core kernels) or, in HN_PREC_FP32_VALU,
    // the direct kernel.  fin (decode_0 only): + outc 1x1 and wf <- d / 1e3 + wf
    auto dc = [&](DcKind kind, int d, Src a, Src b, Src c3, Dst out, const FinalEpi* fin) {
        const DcLayer& l = kind == DcKind::Inc ? ctx->inc : kind == DcKind::Signal ? ctx->sig[d] : ctx->dec[d];
        if (mfma) launch_dc8(ctx, kind, a, b, c3, out, l, fin, H >> d, W >> d, batch, s);
        else launch_dc_direct(ctx, kind, a, b, c3, out, l.w, fin, H >> d, W >> d, batch, s);
    };
    {
        ProfScope ps(ctx, KID_INC, s);
        dc(DcKind::Inc, 0, c.wf, c.res, c.sig, feat(ctx->buf_a[0], 0), nullptr);
    }
    for (int d = 0; d < depth; ++d) {
        {   // out = conv_signal(cat[x, state])
            ProfScope ps(ctx, KID_SIG0 + 3 * d, s);
            dc(DcKind::Signal, d, featsrc(ctx->buf_a[d], d), st_old(d), none, feat(ctx->buf_o[d], d), nullptr);
        }
        {   // state = conv_state(cat[out, state_old]): the streaming kernel where it applies (W >= 64), else the direct kernel
            ProfScope ps(ctx, KID_STATE0 + 3 * d, s);
            const StateLevel v{featsrc(ctx->buf_o[d], d), st_old(d), Dst{c.states_out + ctx->state_off[d], 2 * L, L}, ctx->st[d].w, H >> d, W >> d};
            if (conv_state_applies(ctx, v)) launch_conv_state(ctx, 1, &v, batch, s);
            else launch_state_direct(v, batch, s);
        }
        {   // x = down(out)
            ProfScope ps(ctx, KID_DOWN0 + 3 * d, s);
            if (mfma) launch_down(ctx, featsrc(ctx->buf_o[d], d), feat(ctx->buf_a[d + 1], d + 1), ctx->down[d].f, H >> d, W >> d, batch, s);
            else launch_down_direct(featsrc(ctx->buf_o[d], d), feat(ctx->buf_a[d + 1], d + 1), ctx->down[d].w, H >> d, W >> d, batch, s);
        }
    }
    {
        ProfScope ps(ctx, KID_BOTTLENECK, s);
        dc(DcKind::Bottleneck, depth, featsrc(ctx->buf_a[depth], depth), none, none, feat(ctx->buf_y[depth], depth), nullptr);
    }
    const FinalEpi fin{c.d_out, c.wf_out, c.wf_in, 0};
    for (int d = depth - 1; d >= 0; --d) {
        {   // x = up[d](x)
            ProfScope ps(ctx, KID_UP0 + 2 * d, s);
            if (mfma) launch_up(ctx, featsrc(ctx->buf_y[d + 1], d + 1), feat(ctx->buf_a[d], d), ctx->up[d].f, H >> (d + 1), W >> (d + 1), batch, s);
            else launch_up_direct(featsrc(ctx->buf_y[d + 1], d + 1), feat(ctx->buf_a[d], d), ctx->up[d].w, H >> (d + 1), W >> (d + 1), batch, s);
        }
        // x = decode[d](cat[x, skip_d]); decode_0 + outc + the wavefield update
        ProfScope ps(ctx, KID_DEC0 + 2 * d, s);
        dc(DcKind::Decoder, d, featsrc(ctx->buf_a[d], d), featsrc(ctx->buf_o[d], d), none, d > 0 ? feat(ctx->buf_y[d], d) : Dst{nullptr, 0, 0}, d == 0 ? &fin : nullptr);
    }
    HN_HIP(ctx, hipGetLastError());
    return HN_OK;
}

int rect_unet(hn_ctx* ctx, const float* in6, const float* states_in, float* states_out, float* d_out, int batch, hipStream_t s) {
    int rc = rect_ready_unet(ctx, "hn_unet", batch);
    if (rc != HN_OK) return rc;
    const long plane = (long)ctx->rect->h * ctx->rect->w;
    {
        const size_t sl = sizeof(float) * (size_t)batch * kState * ctx->state_len;
        const MemRange r[] = {{in6, sizeof(float) * (size_t)batch * kInCh * plane, false, "in6"}, {states_in, sl, false, "states_in"},
                              {states_out, sl, true, "states_out"}, {d_out, sizeof(float) * (size_t)batch * 2 * plane, true, "d_out"}};
        const char *who, *other;
        if (first_overlap(r, 4, &who, &other)) return fail(ctx, HN_ERR_ARG, "hn_unet: %s overlaps %s", who, other);
    }
    if ((rc = rect_reserve(ctx, batch, s)) != HN_OK) return rc;
    UnetCall c;
    c.wf = Src{in6, kInCh * plane, plane, 1.f};
    c.res = Src{in6 + 2 * plane, kInCh * plane, plane, 1.f};
    c.sig = Src{in6 + 4 * plane, kInCh * plane, plane, 1.f};
    c.states_in = states_in; c.states_out = states_out; c.d_out = d_out;
    c.batch = batch; c.stream = s;
    return unet_forward_rect(ctx, c);
}

// hn_step's contract in the copying form: every iteration in place in the caller's wf / res, the hidden states ping-pong between the caller's buffer and the
// library's, one device-to-device copy per history and iteration.  The same launches whatever n_iter is, so n_iter in one call equals the same iterations
// in several calls bit for bit.
int rect_step(hn_ctx* ctx, float* wf, float* res, float* states, const float* k_sq, const float* src, int src_batch, int batch, int n_iter, float* res_hist,
              float* wf_hist, float* st_hist, float* rmse_hist, hipStream_t s) {
    int rc = rect_ready_unet(ctx, "hn_step", batch);
    if (rc != HN_OK) return rc;
    if (ctx->opt_lanes > 1) return fail(ctx, HN_ERR_UNSUPPORTED, "hn_step: HN_OPT_LANES %d is not implemented on a rectangular domain (one lane only)", ctx->opt_lanes);
    const long plane = (long)ctx->rect->h * ctx->rect->w, L = ctx->state_len;
    const size_t fc = sizeof(float) * (size_t)batch * 2 * plane, sc = sizeof(float) * (size_t)batch * kState * L, it_n = (size_t)n_iter;
    {   // (as hn_step: res_hist == res / wf_hist == wf, the live buffer being slot 0 of its history, is the one tolerated overlap)
        const MemRange r[] = {{wf_hist != nullptr && wf_hist == wf ? nullptr : wf, fc, true, "wf"}, {res_hist != nullptr && res_hist == res ? nullptr : res, fc, true, "res"},
                              {states, sc, true, "states"}, {k_sq, sizeof(float) * (size_t)batch * plane, false, "k_sq"},
                              {src, sizeof(float) * (size_t)src_batch * 2 * plane, false, "src"}, {res_hist, it_n * fc, true, "res_hist"},
                              {wf_hist, it_n * fc, true, "wf_hist"}, {st_hist, it_n * sc, true, "st_hist"},
                              {rmse_hist, sizeof(float) * it_n * batch, true, "rmse_hist"}};
        const char *who, *other;
        if (first_overlap(r, 9, &who, &other)) return fail(ctx, HN_ERR_ARG, "hn_step: %s overlaps %s", who, other);
    }
    if ((rc = rect_reserve(ctx, batch, s)) != HN_OK) return rc;
    if (n_iter == 0) return HN_OK;
    if (rmse_hist) {
        if ((rc = zero_async(ctx, rmse_hist, sizeof(float) * it_n * batch, s)) != HN_OK) return rc;
        if ((rc = zero_async(ctx, ctx->it_counter, 8 * sizeof(int), s)) != HN_OK) return rc;
    }
    for (int it = 0; it < n_iter; ++it) {
        UnetCall c;
        c.wf = Src{wf, 2 * plane, plane, 1.f};
        c.res = Src{res, 2 * plane, plane, 1e3f};          // 1e3 * residual (hybridnet.py:566)
        c.sig = Src{ctx->rect->sigmas, 0, plane, 1.f};     // sigmas.repeat(B) without the copy
        c.states_in = (it & 1) ? ctx->st_tmp : states; c.states_out = (it & 1) ? states : ctx->st_tmp;
        c.wf_in = wf; c.wf_out = wf;
        c.batch = batch; c.stream = s;
        if ((rc = unet_forward_rect(ctx, c)) != HN_OK) return rc;
        if ((rc = spec_rect_apply(ctx, wf, res, k_sq, src, src_batch, batch, rmse_hist, s, rmse_hist ? ctx->it_counter : nullptr, batch)) != HN_OK) return rc;
        ++ctx->eager_iterations;
        if (res_hist) HN_HIP(ctx, hipMemcpyAsync(res_hist + (size_t)it * batch * 2 * plane, res, fc, hipMemcpyDeviceToDevice, s));
        if (wf_hist) HN_HIP(ctx, hipMemcpyAsync(wf_hist + (size_t)it * batch * 2 * plane, wf, fc, hipMemcpyDeviceToDevice, s));
        if (st_hist) HN_HIP(ctx, hipMemcpyAsync(st_hist + (size_t)it * batch * kState * L, (it & 1) ? states : ctx->st_tmp, sc, hipMemcpyDeviceToDevice, s));
    }
    if (n_iter & 1) HN_HIP(ctx, hipMemcpyAsync(states, ctx->st_tmp, sc, hipMemcpyDeviceToDevice, s));
    if (rmse_hist) {
        launch_rmse_finalize(rmse_hist, n_iter * batch, 1.0f / (float)(2 * plane), s);
        HN_HIP(ctx, hipGetLastError());
    }
    return HN_OK;
}

}  // namespace hn
