// testhooks.cpp — the vdt_* entries: stages of the pipeline exposed to the tests.

#include "../../include/vdmi.h"
#include "vd_common.h"
#include "vd_math.h"
#include "nets.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

extern "C" {

int vdt_set_debug(vd_ctx* h, const char* name, int value) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!name) return vd_set_error(VD_ERR_ARG, "null debug switch name");
    ctx->bands.forget();   // letterbox bands: tiles written under a debug switch are not kept
    // timing-only stage skips: results are WRONG while set (tools/x6bench, tools/runs)
    if (!strcmp(name, "x6_dbg")) { ctx->tune.x6_dbg = value; return VD_OK; }
    if (!strcmp(name, "block32_dbg")) { ctx->tune.block32_dbg = value; return VD_OK; }
    return vd_set_error(VD_ERR_ARG, "unknown debug switch '%s'", name);
}

int vdt_blur_weights(int ksize, float sigma, uint32_t* q) {
    if (!q) return vd_set_error(VD_ERR_ARG, "vdt_blur_weights: null q");
    if (vd_blur_weights(ksize, sigma, q))
        return vd_set_error(VD_ERR_ARG, "vdt_blur_weights: ksize must be odd in [3, %d] (got %d) and sigma finite",
                            VD_BLUR_KSIZE_MAX, ksize);
    return VD_OK;
}

// ---- test hooks ----
static int letterbox_readback(Ctx* ctx, int n, float* out, int cpad);

int vdt_letterbox_tiles(vd_ctx* h, const uint8_t* frames, int n, int fh, int fw, size_t pitch, int where, float* out,
                        int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (!ctx->tiles_on()) return vd_set_error(VD_ERR_STATE, "vdt_letterbox_tiles: tiling is off (vd_tiles)");
    int rc = ctx->check_frames(n, fh, fw, pitch);
    if (rc) return rc;
    TileGrid g;
    if ((rc = ctx->tiles_check(n, fh, fw, &g))) return rc;
    const uint8_t* d = ctx->frames_to_device(frames, n, fh, pitch, where, &rc);
    if (rc) return rc;
    if ((rc = ctx->face_letterbox_tiles(d, n, fh, fw, pitch, g))) return rc;
    return letterbox_readback(ctx, n * g.T, out, cpad);
}

int vdt_letterbox(vd_ctx* h, const uint8_t* frames, int n, int fh, int fw, size_t pitch, int where, float* out,
                  int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    int rc = ctx->check_frames(n, fh, fw, pitch);
    if (rc) return rc;
    const uint8_t* d = ctx->frames_to_device(frames, n, fh, pitch, where, &rc);
    if (rc) return rc;
    if ((rc = ctx->face_letterbox(d, n, fh, fw, pitch))) return rc;
    return letterbox_readback(ctx, n, out, cpad);
}

int vdt_letterbox_nv12(vd_ctx* h, const vd_nv12* frames, int n, int fh, int fw, int where, float* out, int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "vdt_letterbox_nv12: bad where");
    int rc = vd_nv12_check("vdt_letterbox_nv12", frames, n, fh, fw, true);
    if (rc) return rc;
    if ((rc = ctx->check_frames(n, fh, fw, (size_t)fw * 3))) return rc;   // n within max_batch
    Ctx::Nv12Dev d{};
    if ((rc = ctx->nv12_in(vd_yuv420_dev(vd_yuv420_of_nv12(*frames)), n, fh, fw, where, &d))) return rc;
    const Nv12Scope scope(ctx, d, frames->matrix, frames->range);
    if ((rc = ctx->face_letterbox(d.base, n, fh, fw, d.pitch))) return rc;
    return letterbox_readback(ctx, n, out, cpad);
}

int vdt_letterbox_yuv420(vd_ctx* h, const vd_yuv420* frames, int n, int fh, int fw, int where, float* out, int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "vdt_letterbox_yuv420: bad where");
    int rc = vd_yuv420_check("vdt_letterbox_yuv420", frames, n, fh, fw, true);
    if (rc) return rc;
    if ((rc = ctx->check_frames(n, fh, fw, (size_t)fw * 3))) return rc;   // n within max_batch
    Ctx::Nv12Dev d{};
    if ((rc = ctx->nv12_in(vd_yuv420_dev(*frames), n, fh, fw, where, &d))) return rc;
    const Nv12Scope scope(ctx, d, frames->matrix, frames->range);
    if ((rc = ctx->face_letterbox(d.base, n, fh, fw, d.pitch))) return rc;
    return letterbox_readback(ctx, n, out, cpad);
}

int vdt_letterbox_yuv420_16(vd_ctx* h, const vd_yuv420_16* frames, int n, int fh, int fw, int where, float* out, int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "vdt_letterbox_yuv420_16: bad where");
    int rc = vd_yuv420_16_check("vdt_letterbox_yuv420_16", frames, n, fh, fw, true);
    if (rc) return rc;
    if ((rc = ctx->check_frames(n, fh, fw, (size_t)fw * 3))) return rc;   // n within max_batch
    Ctx::Nv12Dev d{};
    if ((rc = ctx->nv12_in(vd_yuv420_dev(*frames), n, fh, fw, where, &d))) return rc;
    const Nv12Scope scope(ctx, d, frames->matrix, frames->range);
    if ((rc = ctx->face_letterbox(d.base, n, fh, fw, d.pitch))) return rc;
    return letterbox_readback(ctx, n, out, cpad);
}

// vdt_letterbox_tiles on surfaces: the tile letterbox of the product path with the surfaces' pixel source
// (the switch vd_tiles_surfaces is not read, as no hook reads a blur setting)
static int letterbox_tiles_420(Ctx* ctx, const char* who, const Yuv420Dev& frames, int matrix, int range, int n, int fh, int fw,
                               int where, float* out, int cpad) {
    if (!ctx->tiles_on()) return vd_set_error(VD_ERR_STATE, "%s: tiling is off (vd_tiles)", who);
    int rc = ctx->check_frames(n, fh, fw, (size_t)fw * 3);   // n within max_batch
    if (rc) return rc;
    TileGrid g;
    if ((rc = ctx->tiles_check(n, fh, fw, &g))) return rc;
    Ctx::Nv12Dev d{};
    if ((rc = ctx->nv12_in(frames, n, fh, fw, where, &d))) return rc;
    const Nv12Scope scope(ctx, d, matrix, range);
    if ((rc = ctx->face_letterbox_tiles(d.base, n, fh, fw, d.pitch, g))) return rc;
    return letterbox_readback(ctx, n * g.T, out, cpad);
}

int vdt_letterbox_tiles_nv12(vd_ctx* h, const vd_nv12* frames, int n, int fh, int fw, int where, float* out, int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vdt_letterbox_tiles_nv12";
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    int rc = vd_nv12_check(who, frames, n, fh, fw, true);
    if (rc) return rc;
    return letterbox_tiles_420(ctx, who, vd_yuv420_dev(vd_yuv420_of_nv12(*frames)), frames->matrix, frames->range, n, fh, fw,
                               where, out, cpad);
}

int vdt_letterbox_tiles_yuv420(vd_ctx* h, const vd_yuv420* frames, int n, int fh, int fw, int where, float* out, int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vdt_letterbox_tiles_yuv420";
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    int rc = vd_yuv420_check(who, frames, n, fh, fw, true);
    if (rc) return rc;
    return letterbox_tiles_420(ctx, who, vd_yuv420_dev(*frames), frames->matrix, frames->range, n, fh, fw, where, out, cpad);
}

int vdt_letterbox_tiles_yuv420_16(vd_ctx* h, const vd_yuv420_16* frames, int n, int fh, int fw, int where, float* out,
                                  int cpad) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vdt_letterbox_tiles_yuv420_16";
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    int rc = vd_yuv420_16_check(who, frames, n, fh, fw, true);
    if (rc) return rc;
    return letterbox_tiles_420(ctx, who, vd_yuv420_dev(*frames), frames->matrix, frames->range, n, fh, fw, where, out, cpad);
}

// the merge step of vd_tiles_merge / vd_tiles_merge_plates with low_on = 1: the strong prefix into
// out_strong as the merge itself writes it, then the whole merged rows (count = m_all) into out_all
int vdt_tiles_merge_low(vd_ctx* h, const vd_boxes* lists, int n, int fh, int fw, int plates, float thr, vd_boxes* out_strong,
                        vd_boxes* out_all) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (out_all && (!out_all->count || !out_all->xyxy || out_all->cap <= 0))
        return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    int rc = vd_tiles_merge_lists(ctx, "vdt_tiles_merge_low", plates != 0, lists, n, fh, fw, out_strong, true, thr);
    if (rc || !out_all) return rc;
    const TileMergeArgs& tm = plates ? ctx->ptiles_last : ctx->tiles_last;
    const hipMemcpyKind kind = out_all->where == VD_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const int w = std::min(out_all->cap, tm.mcap);
    const size_t dp = (size_t)out_all->cap, sp = (size_t)tm.mcap;
    VD_CHECK_HIP(hipMemcpyAsync(out_all->count, tm.m_all, (size_t)n * 4, kind, ctx->stream));
    VD_CHECK_HIP(hipMemcpy2DAsync(out_all->xyxy, dp * 16, tm.m_xyxy, sp * 16, (size_t)w * 16, n, kind, ctx->stream));
    if (out_all->xyxy_f)
        VD_CHECK_HIP(hipMemcpy2DAsync(out_all->xyxy_f, dp * 16, tm.m_xyxy_f, sp * 16, (size_t)w * 16, n, kind, ctx->stream));
    if (out_all->score)
        VD_CHECK_HIP(hipMemcpy2DAsync(out_all->score, dp * 4, tm.m_score, sp * 4, (size_t)w * 4, n, kind, ctx->stream));
    if (out_all->label)
        VD_CHECK_HIP(hipMemcpy2DAsync(out_all->label, dp * 4, tm.m_label, sp * 4, (size_t)w * 4, n, kind, ctx->stream));
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VD_OK;
}

// the first n face canvases as host f32 [n][H][W][cpad], whatever form the plan keeps them in
static int letterbox_readback(Ctx* ctx, int n, float* out, int cpad) {
    const Act& in = ctx->face.input;
    size_t px = (size_t)n * in.h * in.w;
    std::vector<uint16_t> hb;
    std::vector<float> hf;
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (in.f32) {
        hf.resize(px * in.c);
        VD_CHECK_HIP(hipMemcpy(hf.data(), in.p, hf.size() * 4, hipMemcpyDeviceToHost));
    } else {
        hb.resize(px * in.c);
        VD_CHECK_HIP(hipMemcpy(hb.data(), in.p, hb.size() * 2, hipMemcpyDeviceToHost));
    }
    if (ctx->face.s2d) {   // unpack the space-to-depth canvas back to [n][H][W][cpad]
        const int H = ctx->face.in_h, W = ctx->face.in_w;
        for (int f = 0; f < n; ++f)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    for (int c = 0; c < cpad; ++c) {
                        float v = 0.f;
                        if (c < 3) {
                            const int Y = (y + 1) >> 1, X = (x + 1) >> 1, s = ((y + 1) & 1) * 2 + ((x + 1) & 1);
                            const size_t i = (((size_t)f * in.h + Y) * in.w + X) * in.c + s * 4 + c;
                            if (ctx->f32) {                 // fused fp32 stem: fp16 canvas
                                v = from_half(true, hb[i]);
                            } else {
                                uint32_t u = (uint32_t)hb[i] << 16;
                                memcpy(&v, &u, 4);
                            }
                        }
                        out[(((size_t)f * H + y) * W + x) * cpad + c] = v;
                    }
        return VD_OK;
    }
    for (size_t i = 0; i < px; ++i)
        for (int c = 0; c < cpad; ++c) {
            float v = 0.f;
            if (c < in.c) {
                if (in.f32) v = hf[i * in.c + c];
                else v = from_half(ctx->f16, hb[i * in.c + c]);
            }
            out[i * cpad + c] = v;
        }
    return VD_OK;
}

int vdt_forward_heads(vd_ctx* h, const uint8_t* frames, int n, int fh, int fw, size_t pitch, int where, float* loc,
                      float* conf, float* landm) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    int rc = ctx->check_frames(n, fh, fw, pitch);
    if (rc) return rc;
    const uint8_t* d = ctx->frames_to_device(frames, n, fh, pitch, where, &rc);
    if (rc) return rc;
    if ((rc = ctx->face_letterbox(d, n, fh, fw, pitch))) return rc;
    if ((rc = ctx->face_forward(n))) return rc;
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const int A = ctx->face.A;
    for (int l = 0; l < 3; ++l) {
        const Act& hd = ctx->face.heads[l];
        std::vector<float> buf((size_t)n * hd.h * hd.w * 32);
        VD_CHECK_HIP(hipMemcpy(buf.data(), hd.p, buf.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < n; ++b)
            for (int px = 0; px < hd.h * hd.w; ++px)
                for (int k = 0; k < 2; ++k) {
                    const float* src = &buf[((size_t)b * hd.h * hd.w + px) * 32];
                    size_t a = (size_t)b * A + ctx->face.loff[l] + px * 2 + k;
                    if (loc) for (int j = 0; j < 4; ++j) loc[a * 4 + j] = src[4 * k + j];
                    if (conf) for (int j = 0; j < 2; ++j) conf[a * 2 + j] = src[8 + 2 * k + j];
                    if (landm) for (int j = 0; j < 10; ++j) landm[a * 10 + j] = src[12 + 10 * k + j];
                }
    }
    return VD_OK;
}

int vdt_face_band_rows(int canvas_h, int top, int nh, int left, int32_t out[4][5]) {
    if (!out || canvas_h <= 0 || canvas_h % 4) return vd_set_error(VD_ERR_ARG, "vdt_face_band_rows: canvas rows % 4, out");
    const FaceBandPlan P = vd_face_band_plan(canvas_h, top, nh, left);
    for (int k = 0; k < VD_BAND_OPS; ++k) {
        out[k][0] = P.rows[k].top_end; out[k][1] = P.rows[k].bot_begin;
        out[k][2] = P.tile_rows[k]; out[k][3] = P.lo[k]; out[k][4] = P.hi[k];
    }
    return VD_OK;
}

int vdt_face_band_stats(vd_ctx* h, int32_t out[4][5]) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!out) return vd_set_error(VD_ERR_ARG, "vdt_face_band_stats: null out");
    memset(out, 0, sizeof(int32_t) * VD_BAND_OPS * 5);
    const FaceBands& B = ctx->bands;
    if (!B.plan || !B.ran) return VD_OK;
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    unsigned st[VD_BAND_OPS][2];
    VD_CHECK_HIP(hipMemcpy(st, B.stats, sizeof st, hipMemcpyDeviceToHost));
    for (int k = 0; k < VD_BAND_OPS; ++k) {
        out[k][0] = B.cur.lo[k]; out[k][1] = B.cur.hi[k]; out[k][2] = B.cur.tile_rows[k];
        out[k][3] = (int32_t)st[k][0]; out[k][4] = (int32_t)st[k][1];
    }
    return VD_OK;
}

int vdt_postprocess(vd_ctx* h, const float* loc, const float* conf, int n, const int32_t* img_hw, vd_boxes* faces) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (n <= 0 || n > ctx->cfg.max_batch || !loc || !conf || !img_hw) return vd_set_error(VD_ERR_ARG, "vdt_postprocess args");
    for (int i = 1; i < n; ++i)
        if (img_hw[2 * i] != img_hw[0] || img_hw[2 * i + 1] != img_hw[1])
            return vd_set_error(VD_ERR_ARG, "vdt_postprocess: frames of one call share a size");
    const int A = ctx->face.A;
    for (int l = 0; l < 3; ++l) {
        const Act& hd = ctx->face.heads[l];
        std::vector<float> buf((size_t)n * hd.h * hd.w * 32, 0.f);
        for (int b = 0; b < n; ++b)
            for (int px = 0; px < hd.h * hd.w; ++px)
                for (int k = 0; k < 2; ++k) {
                    float* dst = &buf[((size_t)b * hd.h * hd.w + px) * 32];
                    size_t a = (size_t)b * A + ctx->face.loff[l] + px * 2 + k;
                    for (int j = 0; j < 4; ++j) dst[4 * k + j] = loc[a * 4 + j];
                    for (int j = 0; j < 2; ++j) dst[8 + 2 * k + j] = conf[a * 2 + j];
                }
        VD_CHECK_HIP(hipMemcpy(hd.p, buf.data(), buf.size() * 4, hipMemcpyHostToDevice));
    }
    BoxTargets t;
    int rc = ctx->box_targets(faces, n, t);
    if (rc) return rc;
    if ((rc = ctx->face_post(n, img_hw[0], img_hw[1], t))) return rc;
    rc = ctx->box_finish(faces, n, t);
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

int vdt_conv2d(vd_ctx* h, const float* x, int n, int xh, int xw, int cin, const float* wgt, int cout, int kh, int kw,
               int stride, int pad, const float* scale, const float* shift, int act, float slope, const float* res,
               int res_mode, float* y, int* oh_out, int* ow_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (n <= 0 || xh <= 0 || xw <= 0 || cin <= 0 || cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0)
        return vd_set_error(VD_ERR_ARG, "vdt_conv2d: bad shape");
    Conv cv{};
    cv.cin = cin; cv.cout = cout; cv.kh = kh; cv.kw = kw; cv.stride = stride; cv.pad = pad; cv.act = act;
    cv.slope = slope;
    std::vector<float> w(wgt, wgt + (size_t)cout * cin * kh * kw);
    std::vector<float> sc(scale, scale + cout), sh(shift, shift + cout);
    const size_t nalloc = ctx->allocs.size();
    int rc = ctx->upload_conv(cv, w, sc, sh);
    if (rc) return rc;
    const int oh = (xh + 2 * pad - kh) / stride + 1, ow = (xw + 2 * pad - kw) / stride + 1;
    const int es = ctx->f32 ? 4 : 2;
    const int ldx = cv.cin_pad;
    const int ldy = (cout + 7) / 8 * 8;
    std::vector<char> xb((size_t)n * xh * xw * ldx * es, 0), rb;
    for (size_t p = 0; p < (size_t)n * xh * xw; ++p)
        for (int c = 0; c < cin; ++c) {
            float v = x[p * cin + c];
            if (ctx->f32) memcpy(&xb[(p * ldx + c) * 4], &v, 4);
            else { uint16_t b = to_half(ctx->f16, v); memcpy(&xb[(p * ldx + c) * 2], &b, 2); }
        }
    void *dx = nullptr, *dy = nullptr, *dr = nullptr;
    if ((rc = ctx->dalloc(&dx, xb.size()))) return rc;
    if ((rc = ctx->dalloc(&dy, (size_t)n * oh * ow * ldy * 4))) return rc;   // f32 output
    VD_CHECK_HIP(hipMemcpy(dx, xb.data(), xb.size(), hipMemcpyHostToDevice));
    if (res && res_mode) {
        rb.assign((size_t)n * oh * ow * ldy * es, 0);
        for (size_t p = 0; p < (size_t)n * oh * ow; ++p)
            for (int c = 0; c < cout; ++c) {
                float v = res[p * cout + c];
                if (ctx->f32) memcpy(&rb[(p * ldy + c) * 4], &v, 4);
                else { uint16_t b = to_half(ctx->f16, v); memcpy(&rb[(p * ldy + c) * 2], &b, 2); }
            }
        if ((rc = ctx->dalloc(&dr, rb.size()))) return rc;
        VD_CHECK_HIP(hipMemcpy(dr, rb.data(), rb.size(), hipMemcpyHostToDevice));
    }
    ConvArgs a{};
    a.x = dx; a.xh = xh; a.xw = xw; a.ldx = ldx; a.xcoff = 0;
    a.w = cv.w; a.scale = cv.scale; a.shift = cv.shift;
    a.res = dr; a.res_ld = ldy; a.res_coff = 0; a.res_up = 0; a.rh = oh; a.rw = ow;
    a.res_mode = dr ? res_mode : VD_RES_NONE;
    a.y = dy; a.yh = oh; a.yw = ow; a.ldy = ldy; a.ycoff = 0;
    a.B = n; a.cin_pad = cv.cin_pad; a.cout = cout; a.kpad = cv.kpad;
    a.kh = kh; a.kw = kw; a.stride = stride; a.pad = pad; a.M = n * oh * ow;
    a.act = act; a.slope = slope; a.out_f32 = 1; a.f16 = ctx->f16 ? 1 : 0;
    a.tune = &ctx->tune;
    a.wx3 = cv.wx3;
    a.scale_x = cv.scale_x;
    a.f32_split = cv.split;
    // fp16-pair plan: the input's per-frame max |x| as a producer would have left it,
    // and the output's slots, checked below against the host max of the result
    unsigned* dm = nullptr;
    const bool ranged = cv.split == 2;
    if (ranged) {
        std::vector<unsigned> xm(2 * n, 0u);
        for (int b = 0; b < n; ++b) {
            float m = 0.f;
            for (size_t i = (size_t)b * xh * xw * cin; i < (size_t)(b + 1) * xh * xw * cin; ++i) m = std::max(m, std::fabs(x[i]));
            memcpy(&xm[b], &m, 4);
        }
        if ((rc = ctx->dalloc((void**)&dm, xm.size() * 4))) return rc;
        VD_CHECK_HIP(hipMemcpy(dm, xm.data(), xm.size() * 4, hipMemcpyHostToDevice));
        a.xmax = dm;
        a.ymax = dm + n;
    }
    hipError_t e = vd_launch_conv(a, ctx->f32, ctx->stream);
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "conv launch: %s", hipGetErrorString(e));
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<float> yb((size_t)n * oh * ow * ldy);
    VD_CHECK_HIP(hipMemcpy(yb.data(), dy, yb.size() * 4, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < (size_t)n * oh * ow; ++p)
        for (int c = 0; c < cout; ++c) y[p * cout + c] = yb[p * ldy + c];
    if (ranged && cv.wx3) {
        std::vector<float> ym(n);
        VD_CHECK_HIP(hipMemcpy(ym.data(), dm + n, n * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < n; ++b) {
            float m = 0.f;
            for (size_t i = (size_t)b * oh * ow * cout; i < (size_t)(b + 1) * oh * ow * cout; ++i) m = std::max(m, std::fabs(y[i]));
            if (m != ym[b]) {
                for (size_t i = nalloc; i < ctx->allocs.size(); ++i) hipFree(ctx->allocs[i]);
                ctx->allocs.resize(nalloc);
                return vd_set_error(VD_ERR_HIP, "frame %d: output max slot %g, host max %g", b, ym[b], m);
            }
        }
    }
    if (oh_out) *oh_out = oh;
    if (ow_out) *ow_out = ow;
    // release this call's temporaries
    for (size_t i = nalloc; i < ctx->allocs.size(); ++i) hipFree(ctx->allocs[i]);
    ctx->allocs.resize(nalloc);
    return VD_OK;
}

// ---- vdt_run_op: one op of a plan on whole buffers, through Ctx::run_ops ----
// a host f32 image [frames][a.h][a.w][a.c] as a device buffer of the Act's element type
static int op_upload(Ctx* ctx, Act& a, const float* host, int frames, bool f32) {
    const size_t elems = (size_t)frames * a.h * a.w * a.c;
    a.f32 = f32;
    int rc = ctx->dalloc(&a.p, elems * (f32 ? 4 : 2));
    if (rc) return rc;
    if (f32) {
        VD_CHECK_HIP(hipMemcpy(a.p, host, elems * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> hb(elems);
        for (size_t i = 0; i < elems; ++i) hb[i] = to_half(ctx->f16, host[i]);
        VD_CHECK_HIP(hipMemcpy(a.p, hb.data(), elems * 2, hipMemcpyHostToDevice));
    }
    return VD_OK;
}

static int op_download(Ctx* ctx, const Act& a, float* host, int frames) {
    const size_t elems = (size_t)frames * a.h * a.w * a.c;
    if (a.f32) {
        VD_CHECK_HIP(hipMemcpy(host, a.p, elems * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> hb(elems);
        VD_CHECK_HIP(hipMemcpy(hb.data(), a.p, elems * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < elems; ++i) host[i] = from_half(ctx->f16, hb[i]);
    }
    return VD_OK;
}

// per-frame range slots [frames] holding `init` (f32 bit patterns; NULL: zeros)
static int op_slots(Ctx* ctx, Act& a, const float* init, int frames) {
    std::vector<float> z(frames, 0.f);
    int rc = ctx->dalloc((void**)&a.amax, (size_t)frames * 4);
    if (rc) return rc;
    VD_CHECK_HIP(hipMemcpy(a.amax, init ? init : z.data(), (size_t)frames * 4, hipMemcpyHostToDevice));
    return VD_OK;
}

static int op_conv(Ctx* ctx, const float* w, const float* scale, const float* shift, int cin, int cout, int kh, int kw,
                   int stride, int pad, int act, float slope, int* idx) {
    Conv cv{};
    cv.cin = cin; cv.cout = cout; cv.kh = kh; cv.kw = kw; cv.stride = stride; cv.pad = pad; cv.act = act;
    cv.slope = slope;
    std::vector<float> wv(w, w + (size_t)cout * cin * kh * kw), sc(scale, scale + cout), sh(shift, shift + cout);
    int rc = ctx->upload_conv(cv, wv, sc, sh);
    if (rc) return rc;
    ctx->convs.push_back(cv);
    *idx = (int)ctx->convs.size() - 1;
    return VD_OK;
}

static int run_op_impl(Ctx* ctx, vdt_op* o) {
    const bool f32 = ctx->f32;
    const bool ranged = f32 && ctx->tune.f32_split == 2;
    const int vec = f32 ? 4 : 8;
    o->ranged = ranged ? 1 : 0;
    o->family[0] = 0;
    if (!o->x || !o->y || o->frames <= 0 || o->frames > ctx->cfg.max_batch || o->f0 < 0 || o->n <= 0 ||
        o->f0 + o->n > o->frames)
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: buffers / frames [f0, f0 + n) within frames <= max_batch");
    if (o->xh <= 0 || o->xw <= 0 || o->ldx <= 0 || o->yh <= 0 || o->yw <= 0 || o->ldy <= 0 || o->xcoff < 0 || o->ycoff < 0)
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: bad buffer shape");
    if (o->y_is_x && (o->xh != o->yh || o->xw != o->yw || o->ldx != o->ldy))
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: y_is_x needs one buffer shape");
    if (!f32 && !o->out16 && (o->y_is_x || o->r_is_y))
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: an f32 output cannot share a 16-bit buffer (out16 = 0)");
    const bool conv = o->kind == VDT_OP_CONV;
    if (!f32 && !o->out16 && !conv)
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: only convs write f32 outputs in a 16-bit context (out16 = 0)");
    const bool has_res = conv && o->res_mode != VD_RES_NONE && (o->r_is_y || o->res);
    if (!conv && (o->res || o->r_is_y || o->x2)) return vd_set_error(VD_ERR_ARG, "vdt_run_op: residual / x2 on a conv only");
    if (ranged && (!o->xslots || !o->yslots)) return vd_set_error(VD_ERR_ARG, "vdt_run_op: range slot arrays");

    Act ax{}, ay{}, ar{}, ax2{};
    int rc;
    ax.h = o->xh; ax.w = o->xw; ax.c = o->ldx;
    if ((rc = op_upload(ctx, ax, o->x, o->frames, f32))) return rc;
    if (ranged) {   // what the producers of the whole buffer would have left: max |x| of each frame
        const size_t fe = (size_t)o->xh * o->xw * o->ldx;
        std::vector<float> mx(o->frames, 0.f);
        for (int b = 0; b < o->frames; ++b)
            for (size_t i = 0; i < fe; ++i) mx[b] = std::max(mx[b], std::fabs(o->x[b * fe + i]));
        if ((rc = op_slots(ctx, ax, mx.data(), o->frames))) return rc;
    }
    if (o->y_is_x) {
        ay = ax;
    } else {
        ay.h = o->yh; ay.w = o->yw; ay.c = o->ldy;
        if ((rc = op_upload(ctx, ay, o->y, o->frames, f32 || !o->out16))) return rc;
        if (ranged && (rc = op_slots(ctx, ay, o->yslots, o->frames))) return rc;
    }
    if (has_res) {
        if (o->r_is_y) {
            if (o->res_up) return vd_set_error(VD_ERR_ARG, "vdt_run_op: r_is_y with res_up");
            ar = ay;
        } else {
            ar.h = o->rh; ar.w = o->rw; ar.c = o->res_ld;
            if (ar.h <= 0 || ar.w <= 0 || ar.c <= 0) return vd_set_error(VD_ERR_ARG, "vdt_run_op: bad residual shape");
            if ((rc = op_upload(ctx, ar, o->res, o->frames, f32))) return rc;
        }
        const bool fits = o->res_up ? (ar.h >= (o->yh + 1) / 2 && ar.w >= (o->yw + 1) / 2) : (ar.h == o->yh && ar.w == o->yw);
        if (!fits || o->res_coff < 0 || o->res_coff + o->cout > ar.c)
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: residual slice outside its buffer");
    }

    Net net;
    if (conv) {
        if (!o->w || !o->scale || !o->shift || o->cin <= 0 || o->cout <= 0 || o->kh <= 0 || o->kw <= 0 || o->stride <= 0 ||
            o->pad < 0)
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: bad conv");
        if (o->grp_co && (!f32 || o->grp_co < 0 || o->grp_ci <= 0 || o->cout % o->grp_co))
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: grouped convs are an fp32-plan form");
        int ci = -1, c2 = -1;
        if ((rc = op_conv(ctx, o->w, o->scale, o->shift, o->cin, o->cout, o->kh, o->kw, o->stride, o->pad, o->act,
                          o->slope, &ci)))
            return rc;
        ctx->convs[ci].grp_co = o->grp_co;   // after the upload, as the plate net's yconv_group sets them
        ctx->convs[ci].grp_ci = o->grp_co ? o->grp_ci : 0;
        if (o->x2) {
            if (!o->w2 || !o->scale2 || !o->shift2 || o->cin2 <= 0 || o->stride2 <= 0 || o->xh2 <= 0 || o->xw2 <= 0 ||
                o->ldx2 <= 0 || o->xcoff || o->ycoff || has_res || o->grp_co)
                return vd_set_error(VD_ERR_ARG, "vdt_run_op: bad second conv (plan form: no offsets, no residual)");
            if ((rc = op_conv(ctx, o->w2, o->scale2, o->shift2, o->cin2, o->cout, 1, 1, o->stride2, 0, VD_ACT_NONE, 0.f, &c2)))
                return rc;
            ax2.h = o->xh2; ax2.w = o->xw2; ax2.c = o->ldx2;
            if ((rc = op_upload(ctx, ax2, o->x2, o->frames, f32))) return rc;
            if (ranged) {
                const size_t fe = (size_t)o->xh2 * o->xw2 * o->ldx2;
                std::vector<float> mx(o->frames, 0.f);
                for (int b = 0; b < o->frames; ++b)
                    for (size_t i = 0; i < fe; ++i) mx[b] = std::max(mx[b], std::fabs(o->x2[b * fe + i]));
                if ((rc = op_slots(ctx, ax2, mx.data(), o->frames))) return rc;
            }
            rc = ctx->add_conv_dual(net, ci, ax, c2, ax2, ay);
        } else {
            rc = ctx->add_conv(net, ci, ax, o->xcoff, ay, o->ycoff, has_res ? &ar : nullptr, o->res_coff, o->res_mode,
                               o->res_up);
        }
        if (rc) return rc;
    } else if (o->kind == VDT_OP_MAXPOOL || o->kind == VDT_OP_UPSAMPLE) {
        const bool pool = o->kind == VDT_OP_MAXPOOL;
        if (o->ch <= 0 || (o->ch | o->ldx | o->xcoff | o->ldy | o->ycoff) % vec || o->xcoff + o->ch > o->ldx ||
            o->ycoff + o->ch > o->ldy)
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: channel slices of whole %d-element vectors inside the buffers", vec);
        if (pool ? (o->k <= 0 || o->s <= 0 || o->p < 0 || o->p >= o->k || o->xh + 2 * o->p < o->k ||
                    o->xw + 2 * o->p < o->k || o->yh != (o->xh + 2 * o->p - o->k) / o->s + 1 ||
                    o->yw != (o->xw + 2 * o->p - o->k) / o->s + 1)
                 : (o->yh != 2 * o->xh || o->yw != 2 * o->xw))
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: pool / upsample output shape");
        Op op{};
        op.kind = pool ? OP_MAXPOOL : OP_UPSAMPLE;
        op.x = ax; op.xcoff = o->xcoff;
        op.y = ay; op.ycoff = o->ycoff;
        op.ch = o->ch; op.k = o->k; op.s = o->s; op.p = o->p;
        net.ops.push_back(op);
    } else if (o->kind == VDT_OP_DWCONV) {
        if (!o->w || !o->scale || !o->shift || o->cout <= 0 || o->cout % vec || o->ldx % vec || o->ldy % vec ||
            (o->stride != 1 && o->stride != 2) || o->xcoff || o->ycoff || o->y_is_x)
            return vd_set_error(VD_ERR_ARG, "vdt_run_op: bad depthwise conv (plan form: offsets 0, whole vectors)");
        DwConv d;
        d.c = o->cout; d.stride = o->stride; d.act = o->act; d.slope = o->slope;
        std::vector<float> wt((size_t)9 * d.c);
        for (int c = 0; c < d.c; ++c)
            for (int t = 0; t < 9; ++t) wt[(size_t)t * d.c + c] = o->w[(size_t)c * 9 + t];
        if (f32) {
            if ((rc = ctx->dalloc(&d.w, wt.size() * 4))) return rc;
            VD_CHECK_HIP(hipMemcpy(d.w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
        } else {
            std::vector<uint16_t> hw(wt.size());
            for (size_t i = 0; i < wt.size(); ++i) hw[i] = to_half(ctx->f16, wt[i]);
            if ((rc = ctx->dalloc(&d.w, hw.size() * 2))) return rc;
            VD_CHECK_HIP(hipMemcpy(d.w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
        }
        if ((rc = ctx->dalloc((void**)&d.scale, d.c * 4)) || (rc = ctx->dalloc((void**)&d.shift, d.c * 4))) return rc;
        VD_CHECK_HIP(hipMemcpy(d.scale, o->scale, d.c * 4, hipMemcpyHostToDevice));
        VD_CHECK_HIP(hipMemcpy(d.shift, o->shift, d.c * 4, hipMemcpyHostToDevice));
        ctx->dwconvs.push_back(d);
        if ((rc = ctx->add_dwconv(net, (int)ctx->dwconvs.size() - 1, ax, ay))) return rc;
    } else {
        return vd_set_error(VD_ERR_ARG, "vdt_run_op: unknown op kind %d", o->kind);
    }

    vd_conv_fam_set(VD_FAM_NONE);
    if ((rc = ctx->run_ops(net, 0, 1, o->f0, o->n))) return rc;
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (conv) snprintf(o->family, sizeof o->family, "%s", vd_conv_fam_name(vd_conv_fam_get()));
    if ((rc = op_download(ctx, ay, o->y, o->frames))) return rc;
    if (ranged) {
        VD_CHECK_HIP(hipMemcpy(o->xslots, ax.amax, (size_t)o->frames * 4, hipMemcpyDeviceToHost));
        VD_CHECK_HIP(hipMemcpy(o->yslots, ay.amax, (size_t)o->frames * 4, hipMemcpyDeviceToHost));
    }
    return VD_OK;
}

int vdt_run_op(vd_ctx* h, vdt_op* o) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!o) return vd_set_error(VD_ERR_ARG, "vdt_run_op: null op");
    const size_t nalloc = ctx->allocs.size(), nconv = ctx->convs.size(), ndw = ctx->dwconvs.size();
    const int rc = run_op_impl(ctx, o);
    // release this call's temporaries; amax_snaps is keyed by conv index and its arrays are among the
    // allocations freed here, so the temporary convs' entries go first
    (void)hipStreamSynchronize(ctx->stream);
    ctx->amax_snaps.erase(ctx->amax_snaps.lower_bound((int)nconv), ctx->amax_snaps.end());
    for (size_t i = nalloc; i < ctx->allocs.size(); ++i) hipFree(ctx->allocs[i]);
    ctx->allocs.resize(nalloc);
    ctx->convs.resize(nconv);
    ctx->dwconvs.resize(ndw);
    return rc;
}

}  // extern "C"
