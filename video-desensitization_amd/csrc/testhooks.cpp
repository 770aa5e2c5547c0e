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
    if ((rc = ctx->nv12_in(*frames, n, fh, fw, where, &d))) return rc;
    const Nv12Scope scope(ctx, d, frames->matrix, frames->range);
    if ((rc = ctx->face_letterbox(d.base, n, fh, fw, d.pitch))) return rc;
    return letterbox_readback(ctx, n, out, cpad);
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

}  // extern "C"
