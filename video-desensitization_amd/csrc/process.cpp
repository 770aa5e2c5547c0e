// process.cpp — detection and blurring: the blur passes behind the mask setting, the stand-alone
// blur entries, vd_detect*, vd_read_boxes and vd_process / vd_process_lead and their 4:2:0 forms.

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

int Ctx::launch_mosaic(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                       const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int level, int cells) {
    const int tcap = (cnt0 ? cap0 : 0) + (cnt1 ? cap1 : 0);
    int rc = ensure_staging(&mosaic_table, &mosaic_table_bytes, vd_mosaic_table_bytes(n, tcap) + 64);
    if (rc) return rc;
    const int map_on = tune.mosaic_map | (tune.mosaic_nt << 1) | (tune.mosaic_gather ? 16 : 0) | ((tune.mosaic_rows & 63) << 8);
    auto launch = [&](int stages) {
        return vd_launch_mosaic(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, level, mosaic_table, stages,
                                map_on, tune.mosaic_cells, stream, cells);
    };
    hipError_t e = hipSuccess;
    if (tune.mosaic_fused) {
        // one launch: the output pass walks and gathers its bands' cells itself (family 1)
        t_begin(1, 2.0 * n * (double)h * w * 3);
        e = launch(8);
        t_end();
    } else {
        t_begin(6, 0);
        e = launch(1);
        t_end();
        if (e == hipSuccess) {
            t_begin(1, 2.0 * n * (double)h * w * 3);
            e = launch(2);
            t_end();
        }
    }
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "mosaic: %s", hipGetErrorString(e));
    return VD_OK;
}

// The scaled smooth blur (vd_cells in a Gaussian-mode context, vd_smooth): the copy in -> out,
// then the box pass; no scratch (the cell sums live in LDS). Two family-1 intervals: the copy
// carries the frames' bytes, the box pass's bytes follow from the boxes.
int Ctx::launch_smooth(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                       const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int level, int cells) {
    if (h > 32768 || w > 32768 || level < 1 || level > 32768)
        return vd_set_error(VD_ERR_ARG, "smooth blur: h, w <= 32768 and level in [1, 32768] required (got %d x %d, "
                            "level %d)", w, h, level);
    if (cells < VD_CELLS_MIN || cells > VD_CELLS_MAX)
        return vd_set_error(VD_ERR_ARG, "smooth blur: cells %d outside [%d, %d]", cells, VD_CELLS_MIN, VD_CELLS_MAX);
    hipError_t e = hipSuccess;
    for (int stage = 0; stage < 2 && e == hipSuccess; ++stage) {
        t_begin(1, stage == 0 ? 2.0 * n * (double)h * w * 3 : 0);
        e = vd_launch_smooth(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, level, cells, stage, stream);
        t_end();
    }
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "smooth: %s", hipGetErrorString(e));
    return VD_OK;
}

// Gaussian mode: plan kernel, band pass (copy + independent boxes), dependent-box pass,
// bracketed as one family-1 interval with the mosaic's algorithmic bytes.
int Ctx::launch_blur(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                     const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int ksize, float sigma) {
    uint32_t q[VD_BLUR_KSIZE_MAX];
    if (vd_blur_weights(ksize, sigma, q))
        return vd_set_error(VD_ERR_ARG, "blur: ksize must be odd in [3, %d] (got %d) and sigma finite",
                            VD_BLUR_KSIZE_MAX, ksize);
    const int tcap = (cnt0 ? cap0 : 0) + (cnt1 ? cap1 : 0);
    int rc = ensure_staging(&blur_table, &blur_table_bytes, vd_blur_table_bytes(n, h, pitch, tcap));
    if (rc) return rc;
    t_begin(1, 2.0 * n * (double)h * w * 3);
    hipError_t e = vd_launch_blur(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, ksize, q, blur_table,
                                  stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "blur: %s", hipGetErrorString(e));
    return VD_OK;
}

// ---- mask shaping (mask.hip) ----
// Merged rows of the lists grown by mask_grow; the row capacity is the lists' capacity, so the
// scratch and the grid depend on n and the capacities only (the counts stay on the device).
int Ctx::launch_mask_grow(int n, const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1,
                          int zero_tail) {
    const size_t mcap = std::max<size_t>((size_t)(cnt0 ? cap0 : 0) + (size_t)(cnt1 ? cap1 : 0), 1);
    if (mcap > 0x7fffffffu) return vd_set_error(VD_ERR_ARG, "mask: list capacity too large");
    const size_t nb = (size_t)n * mcap;
    int rc = ensure_staging(&mask_rows, &mask_rows_bytes, nb * 16 + (size_t)n * 4 + 64);
    if (rc) return rc;
    MaskArgs a{};
    a.n = n;
    a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cap0;
    a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cap1;
    a.g = mask_grow; a.zero_tail = zero_tail;
    a.m_xy = (int*)mask_rows; a.m_cnt = a.m_xy + nb * 4; a.mcap = (int)mcap;
    t_begin(3, (double)nb * 16);                  // the rows' bytes: the counts are known to the device only
    hipError_t e = vd_launch_mask_grow(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "mask grow: %s", hipGetErrorString(e));
    mask_last = a;
    return VD_OK;
}

int Ctx::launch_mask_restore(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch) {
    MaskArgs a = mask_last;
    a.in = in; a.out = out; a.n = n; a.h = h; a.w = w; a.pitch = pitch;
    // the bytes moved follow from the boxes (6 B per pixel of a clipped box outside every
    // ellipse), which the host does not see: time and launches only
    t_begin(1, 0);
    hipError_t e = vd_launch_mask_restore(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "mask restore: %s", hipGetErrorString(e));
    return VD_OK;
}

// What the three blurring calls launch. Default mask: the rectangular pass alone, exactly as
// before. Otherwise the lists are grown into one merged row per frame, the rectangular pass
// runs on that row (its second list null), and the ellipse composite follows it.
int Ctx::launch_shaped(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                       const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int pass, int level,
                       int ksize, float sigma, int cells) {
    const bool shaped = mask_on() && (cnt0 || cnt1);
    if (shaped) {
        int rc = launch_mask_grow(n, cnt0, xy0, cap0, cnt1, xy1, cap1);
        if (rc) return rc;
        cnt0 = mask_last.m_cnt; xy0 = mask_last.m_xy; cap0 = mask_last.mcap;
        cnt1 = xy1 = nullptr; cap1 = 0;
    }
    // the cell levels come from the boxes as this pass receives them: grown, when a mask is set
    int rc = pass == RECT_GAUSSIAN ? launch_blur(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, ksize, sigma)
             : pass == RECT_SMOOTH ? launch_smooth(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, level, cells)
                                   : launch_mosaic(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, level, cells);
    if (rc) return rc;
    if (shaped && mask_shape == VD_MASK_ELLIPSE) return launch_mask_restore(in, out, n, h, w, pitch);
    return VD_OK;
}

// box-scaled strength (vd_cells): pixelation takes its level per box, the Gaussian mode becomes
// the scaled smooth blur
int Ctx::launch_cfg_pass(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                         const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1) {
    const bool gaussian = cfg.blur_mode == VD_BLUR_GAUSSIAN;
    const int pass = !gaussian ? RECT_MOSAIC : (cells ? RECT_SMOOTH : RECT_GAUSSIAN);
    return launch_shaped(in, out, n, h, w, pitch, cnt0, xy0, cap0, cnt1, xy1, cap1, pass, cfg.mosaic_level,
                         cfg.blur_ksize, cfg.blur_sigma, cells);
}

// The NV12 output pass: what launch_shaped is to RGB frames. Pixelation (nv12.hip) or the scaled
// smooth blur (smooth.hip) of both planes on the grown lists, then the ellipse composite of both
// planes (mask.hip). The cell levels come from the grown boxes.
int Ctx::launch_nv12_pass(const Nv12Dev& in, const Nv12Dev& out, int n, int h, int w, const int* cnt0, const int* xy0,
                          int cap0, const int* cnt1, const int* xy1, int cap1, int pass, int level, int ncells) {
    if (pass == RECT_SMOOTH) {
        if (h > 32768 || w > 32768 || level < 1 || level > 32768)
            return vd_set_error(VD_ERR_ARG, "smooth blur: h, w <= 32768 and level in [1, 32768] required (got %d x %d, "
                                "level %d)", w, h, level);
        if (ncells < VD_CELLS_MIN || ncells > VD_CELLS_MAX)
            return vd_set_error(VD_ERR_ARG, "smooth blur: cells %d outside [%d, %d]", ncells, VD_CELLS_MIN, VD_CELLS_MAX);
    }
    const bool shaped = mask_on() && (cnt0 || cnt1);
    if (shaped) {
        int rc = launch_mask_grow(n, cnt0, xy0, cap0, cnt1, xy1, cap1);
        if (rc) return rc;
        cnt0 = mask_last.m_cnt; xy0 = mask_last.m_xy; cap0 = mask_last.mcap;
        cnt1 = xy1 = nullptr; cap1 = 0;
    }
    Nv12MosaicArgs a{};
    a.set(in, out);
    a.n = n; a.h = h; a.w = w;
    a.cnt0 = cnt0; a.xy0 = xy0; a.cap0 = cap0;
    a.cnt1 = cnt1; a.xy1 = xy1; a.cap1 = cap1;
    a.level = level; a.cells = ncells;
    hipError_t e = hipSuccess;
    if (pass == RECT_SMOOTH) {   // the copy carries the frames' bytes, the box pass's follow from the boxes
        for (int stage = 0; stage < 2 && e == hipSuccess; ++stage) {
            t_begin(1, stage == 0 ? 2.0 * 1.5 * in.es() * n * (double)h * w : 0);
            e = vd_launch_smooth_nv12(a, stage, stream, in.depth, in.shift);
            t_end();
        }
        if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "nv12 smooth: %s", hipGetErrorString(e));
    } else {
        t_begin(1, 2.0 * 1.5 * in.es() * n * (double)h * w);
        e = vd_launch_mosaic_nv12(a, stream, in.depth);
        t_end();
        if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "nv12 mosaic: %s", hipGetErrorString(e));
    }
    if (!(shaped && mask_shape == VD_MASK_ELLIPSE)) return VD_OK;
    MaskNv12Args m{};
    m.in = in.base; m.in_pitch = in.pitch; m.in_uv = in.u; m.in_v = in.v; m.in_cp = in.cpitch; m.in_stride = in.stride;
    m.out = out.base; m.out_pitch = out.pitch; m.out_uv = out.u; m.out_v = out.v; m.out_cp = out.cpitch; m.out_stride = out.stride;
    m.in_step = in.step; m.out_step = out.step;
    m.n = n; m.h = h; m.w = w;
    m.m_cnt = mask_last.m_cnt; m.m_xy = mask_last.m_xy; m.mcap = mask_last.mcap;
    t_begin(1, 0);               // as the RGB restore: its bytes follow from the boxes
    e = vd_launch_mask_restore_nv12(m, stream, in.es());
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "nv12 mask restore: %s", hipGetErrorString(e));
    return VD_OK;
}

extern "C" {

int vd_detect(vd_ctx* h, const uint8_t* frames, int n, int fh, int fw, size_t pitch, int where, vd_boxes* faces) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    int rc = ctx->check_frames(n, fh, fw, pitch);
    if (rc) return rc;
    const bool tiled = ctx->faces_tiled();
    TileGrid g;
    if (tiled && (rc = ctx->tiles_check(n, fh, fw, &g))) return rc;
    BoxTargets t;
    rc = ctx->box_targets(faces, n, t);
    if (rc) return rc;
    const uint8_t* d = ctx->frames_to_device(frames, n, fh, pitch, where, &rc);
    if (rc) return rc;
    if (tiled) {   // T net inputs per frame, merged into one list (tiles.hip)
        if ((rc = ctx->face_letterbox_tiles(d, n, fh, fw, pitch, g))) return rc;
        if ((rc = ctx->face_forward(n * g.T, false))) return rc;
        if ((rc = ctx->face_post_tiled(n, fh, fw, g, t))) return rc;
        return ctx->box_finish(faces, n, t);
    }
    if ((rc = ctx->face_letterbox(d, n, fh, fw, pitch))) return rc;
    if ((rc = ctx->face_forward(n))) return rc;
    if ((rc = ctx->face_post(n, fh, fw, t))) return rc;
    return ctx->box_finish(faces, n, t);
}

int vd_detect_plates(vd_ctx* h, const uint8_t* frames, int n, int fh, int fw, size_t pitch, int where,
                     vd_boxes* plates) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!ctx->plate.loaded) return vd_set_error(VD_ERR_STATE, "plate weights not loaded");
    int rc = ctx->check_frames(n, fh, fw, pitch);
    if (rc) return rc;
    const bool tiled = ctx->plates_tiled();   // T net inputs per frame, merged into one list (tiles.hip)
    TileGrid g;
    if (tiled && (rc = ctx->tiles_check(n, fh, fw, &g))) return rc;
    BoxTargets t;
    rc = ctx->box_targets(plates, n, t);
    if (rc) return rc;
    const uint8_t* d = ctx->frames_to_device(frames, n, fh, pitch, where, &rc);
    if (rc) return rc;
    if ((rc = vd_plate_detect(*ctx, d, n, fh, fw, pitch, false, tiled ? &g : nullptr, t))) return rc;
    return ctx->box_finish(plates, n, t);
}

// The stand-alone blurring calls: out-of-place pass `pass` over the caller's frames and one box list
// (host frames and lists are staged; the last five arguments are launch_shaped's).
static int blur_entry(Ctx* ctx, const char* who, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch,
                      int where, const vd_boxes* boxes, int pass, int level, int ksize, float sigma, int cells) {
    if (!in || !out || !boxes) return vd_set_error(VD_ERR_ARG, "%s: null argument", who);
    if (n <= 0 || fh <= 0 || fw <= 0 || pitch < (size_t)fw * 3) return vd_set_error(VD_ERR_ARG, "%s: bad geometry", who);
    const size_t bytes = (size_t)n * fh * pitch;
    if ((const void*)in == (const void*)out || (where == VD_DEVICE && vd_ranges_overlap(in, out, bytes)))
        return vd_set_error(VD_ERR_ARG, "%s: out-of-place only (out must not overlap in)", who);
    int rc = VD_OK;
    const uint8_t* din = in;
    uint8_t* dout = out;
    if (where == VD_HOST) {
        if ((rc = ctx->ensure_staging(&ctx->stage_in, &ctx->stage_in_bytes, bytes))) return rc;
        if ((rc = ctx->ensure_staging(&ctx->stage_out, &ctx->stage_out_bytes, bytes))) return rc;
        VD_CHECK_HIP(hipMemcpyAsync(ctx->stage_in, in, bytes, hipMemcpyHostToDevice, ctx->stream));
        din = (const uint8_t*)ctx->stage_in;
        dout = (uint8_t*)ctx->stage_out;
    }
    BoxListIn b;
    if ((rc = ctx->box_list_in(who, boxes, n, false, 0, &b))) return rc;
    if ((rc = ctx->launch_shaped(din, dout, n, fh, fw, pitch, b.cnt, b.xy, boxes->cap, nullptr, nullptr, 0, pass, level,
                                 ksize, sigma, cells)))
        return rc;
    if (where == VD_HOST) {
        VD_CHECK_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    } else if (b.staged) {
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused by the next call
    }
    return VD_OK;
}

int vd_mosaic(vd_ctx* h, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch, int where,
              const vd_boxes* boxes, int level, int mode) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (mode != VD_MOSAIC_OUT_OF_PLACE) return vd_set_error(VD_ERR_ARG, "unsupported mosaic mode %d", mode);
    if (level <= 0) return vd_set_error(VD_ERR_ARG, "vd_mosaic: bad geometry");
    return blur_entry(ctx, "vd_mosaic", in, out, n, fh, fw, pitch, where, boxes, Ctx::RECT_MOSAIC, level, 0, 0.f,
                      ctx->cells);
}

int vd_blur(vd_ctx* h, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch, int where,
            const vd_boxes* boxes, int ksize, float sigma) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    uint32_t q[VD_BLUR_KSIZE_MAX];
    if (vd_blur_weights(ksize, sigma, q))
        return vd_set_error(VD_ERR_ARG, "vd_blur: ksize must be odd in [3, %d] (got %d) and sigma finite",
                            VD_BLUR_KSIZE_MAX, ksize);
    return blur_entry(ctx, "vd_blur", in, out, n, fh, fw, pitch, where, boxes, Ctx::RECT_GAUSSIAN, 0, ksize, sigma, 0);
}

int vd_smooth(vd_ctx* h, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch, int where,
              const vd_boxes* boxes, int level, int cells) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (cells < VD_CELLS_MIN || cells > VD_CELLS_MAX)
        return vd_set_error(VD_ERR_ARG, "vd_smooth: cells %d outside [%d, %d]", cells, VD_CELLS_MIN, VD_CELLS_MAX);
    if (level < 1 || level > 32768) return vd_set_error(VD_ERR_ARG, "vd_smooth: level %d outside [1, 32768]", level);
    if (fh > 32768 || fw > 32768) return vd_set_error(VD_ERR_ARG, "vd_smooth: bad geometry (h, w in [1, 32768])");
    return blur_entry(ctx, "vd_smooth", in, out, n, fh, fw, pitch, where, boxes, Ctx::RECT_SMOOTH, level, 0, 0.f, cells);
}

// A vd_process_lead call's part in the body it shares with vd_process: the blur step becomes
// the lead step (lists, blur of the m emitted frames, ring update).
struct LeadCall {
    int flush, m;
};

// A vd_process_nv12 call's part in that body: the frames are NV12 surfaces (checked by the entry
// point), so the letterbox and the output launches differ; `in` / `out` / `pitch` are not used. Together
// with a LeadCall (vd_process_lead_nv12) `out` describes the m emitted surfaces, NULL when m == 0.
struct Nv12Call {
    const Yuv420Dev* in; const Yuv420Dev* out;   // any layout of vd_yuv420 (the *_nv12 entries: the NV12 one) or vd_yuv420_16
    int matrix, range;                           // of `in`
};

static int process_impl(Ctx* ctx, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch, int where,
                        int flags, vd_boxes* faces, vd_boxes* plates, const LeadCall* lc,
                        const Nv12Call* nv = nullptr) {
    const bool do_faces = flags & VD_PROC_FACES, do_plates = flags & VD_PROC_PLATES;
    const bool do_mosaic = flags & VD_PROC_MOSAIC, mosaic_plates = flags & VD_PROC_MOSAIC_PLATES;
    if (do_faces && !ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights not loaded");
    if (do_plates && !ctx->plate.loaded) return vd_set_error(VD_ERR_STATE, "plate weights not loaded");
    if (mosaic_plates && !do_plates) return vd_set_error(VD_ERR_ARG, "MOSAIC_PLATES needs PLATES");
    if (!lc && !nv && do_mosaic && !out) return vd_set_error(VD_ERR_ARG, "MOSAIC needs an output buffer");
    if (do_mosaic && ctx->cells && ctx->cfg.blur_mode == VD_BLUR_GAUSSIAN &&
        (fh > 32768 || fw > 32768 || ctx->cfg.mosaic_level < 1 || ctx->cfg.mosaic_level > 32768))
        return vd_set_error(VD_ERR_ARG, "vd_process: the smooth blur (vd_cells) needs h, w <= 32768 and mosaic_level "
                            "in [1, 32768]");
    int rc = nv ? ctx->check_frames(n, fh, fw, (size_t)fw * 3) : ctx->check_frames(n, fh, fw, pitch);   // NV12: n alone
    if (rc) return rc;
    // tiled detection: T net inputs per frame through the tiled nets (vd_tiles_nets), merged before
    // anything reads them
    const bool tiled = do_faces && ctx->faces_tiled();
    const bool ptiled = do_plates && ctx->plates_tiled();
    TileGrid tg;
    if ((tiled || ptiled) && (rc = ctx->tiles_check(n, fh, fw, &tg))) return rc;
    // the mosaic is out of place (combine_detect.py:142 blurs a copy; each box reads the
    // previous box's output, :247-249): its one-launch output pass gathers cell colours
    // from `in` anywhere in the frame while other workgroups write `out`, so device
    // frames that overlap would race (host frames are staged in separate buffers)
    if (!lc && !nv && do_mosaic && where == VD_DEVICE && vd_ranges_overlap(in, out, (size_t)n * fh * pitch))
        return vd_set_error(VD_ERR_ARG, "vd_process: MOSAIC is out-of-place (out must not overlap in)");
    BoxTargets tf{}, tp{};
    if (do_faces && (rc = ctx->box_targets(faces, n, tf))) return rc;
    if (do_plates && plates) {   // plate box staging must not alias the face staging
        if (!plates->count || !plates->xyxy || plates->cap <= 0)
            return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
        if (plates->where == VD_DEVICE) {
            tp.cap = plates->cap; tp.count = plates->count; tp.xyxy = plates->xyxy; tp.xyxy_f = plates->xyxy_f;
            tp.score = plates->score; tp.label = plates->label;
        } else if ((rc = ctx->host_box_staging(&ctx->stage_box2, &ctx->stage_box2_bytes, plates->cap, n, tp))) {
            return rc;
        }
    }
    const uint8_t* d = nullptr;
    Ctx::Nv12Dev nin{}, nout{};
    if (nv) {   // host surfaces are staged packed; from here d / pitch are the first luma byte and the planes' pitch
        if ((rc = ctx->nv12_in(*nv->in, n, fh, fw, where, &nin))) return rc;
        d = nin.base; pitch = nin.pitch;
    } else {
        d = ctx->frames_to_device(in, n, fh, pitch, where, &rc);
        if (rc) return rc;
    }
    const Nv12Scope nv_scope(ctx, nin, nv ? nv->matrix : 0, nv ? nv->range : 0, nv != nullptr);
    // Face and plate branches run concurrently (the reference submits them to two
    // threads, combine_detect.py:214-217): plates on stream2, forked/joined by events.
    const bool fork = do_faces && do_plates;
    hipStream_t plate_stream = ctx->stream2;
    // Both canvases from one read of the frames where the geometry allows (pre.hip
    // letterbox_s2d_pair_kernel); the plate branch then forks after it.
    bool paired = false;
    if (fork && !tiled) {   // tiling: the tile letterbox fills the face canvases, the plate branch its own
        LetterboxArgs fa, pa;
        ctx->face_letterbox_args(d, n, fh, fw, pitch, &fa);
        if (ctx->tune.lb_pair && vd_plate_letterbox_args(*ctx, d, n, fh, fw, pitch, &pa) == VD_OK &&
            vd_letterbox_pair_ok(fa, pa)) {
            ctx->t_begin(2, (double)n * (fa.nh * (double)fw * vd_src_bpp(fa.nv) + (double)(fa.oh / 2 + 1) * (fa.ow / 2 + 1) * (fa.out_f32 ? 64 : 32) +
                                         (double)(pa.oh / 2 + 1) * (pa.ow / 2 + 1) * (pa.out_f32 ? 64 : 32)));
            hipError_t e = vd_launch_letterbox_pair(fa, pa, ctx->stream);
            ctx->t_end();
            if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "letterbox pair: %s", hipGetErrorString(e));
            paired = true;
        }
    }
    // The plate branch may be held back until face stage `plate_stage` has been issued
    // (its HBM-bound convs then overlap the MFMA-bound late face layers).
    const int ps = ctx->tune.plate_stage;
    ctx->fork_at = -1;
    if (fork && ps > 0) {
        ctx->fork_at = ps >= 5 ? (int)ctx->face.net.ops.size() : ctx->face.net.stage_end[std::min(ps, 4)];
        if (ctx->fork_at <= 0) ctx->fork_at = -1;
    }
    if (fork && ctx->fork_at < 0) {
        VD_CHECK_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
        VD_CHECK_HIP(hipStreamWaitEvent(plate_stream, ctx->ev_fork, 0));
    }
    if (do_faces) {
        if (tiled) {
            if ((rc = ctx->face_letterbox_tiles(d, n, fh, fw, pitch, tg))) return rc;
        } else if (!paired && (rc = ctx->face_letterbox(d, n, fh, fw, pitch))) {
            return rc;
        }
        if ((rc = ctx->face_forward(tiled ? n * tg.T : n, !tiled))) return rc;
        if (ctx->fork_at > 0) {
            ctx->fork_at = -1;
            VD_CHECK_HIP(hipStreamWaitEvent(plate_stream, ctx->ev_fork, 0));
        }
        if ((rc = tiled ? ctx->face_post_tiled(n, fh, fw, tg, tf) : ctx->face_post(n, fh, fw, tf))) return rc;
    }
    if (do_plates) {
        hipStream_t main = ctx->stream;
        if (fork) ctx->stream = plate_stream;
        rc = vd_plate_detect(*ctx, d, n, fh, fw, pitch, paired, ptiled ? &tg : nullptr, tp);
        ctx->stream = main;
        if (rc) return rc;
    }
    // the mosaic reads plate boxes only with MOSAIC_PLATES (the reference discards them,
    // combine_detect.py:239): otherwise it runs on the face stream before the plate branch
    // joins, beside the branch's last launches (option mosaic_early)
    const bool mosaic_first = do_mosaic && fork && !mosaic_plates && ctx->tune.mosaic_early;
    // every kept box, from the library's complete keep lists (the caller's arrays
    // may hold fewer: cap), faces in NMS order then plates (combine_detect.py:241-249)
    const PostScratch& fp = ctx->face.post;
    const PostScratch& pp = ctx->plate.post;
    const TileMergeArgs& tm = ctx->tiles_last;   // tiling: the merged rows are the face list
    const int* c0 = do_faces ? (tiled ? tm.m_count : fp.kcount) : nullptr;
    const int* x0 = do_faces ? (tiled ? tm.m_xyxy : fp.kxyxy) : nullptr;
    const TileMergeArgs& pm = ctx->ptiles_last;  //   ... and the plate list, where the plate net is tiled
    const int* c1 = mosaic_plates ? (ptiled ? pm.m_count : pp.kcount) : nullptr;
    const int* x1 = mosaic_plates ? (ptiled ? pm.m_xyxy : pp.kxyxy) : nullptr;
    int k0 = do_faces ? (tiled ? tm.mcap : fp.kcap) : 0, k1 = mosaic_plates ? (ptiled ? pm.mcap : pp.kcap) : 0;
    const int* dc0 = c0; const int* dx0 = x0; const int* dc1 = c1; const int* dx1 = x1;
    int dk0 = k0, dk1 = k1;                        // D as detected (rescue: E): what the lead step matches on
    // weak-detection rescue: the lists become E = D ++ R in merged rows (one step, before the hold);
    // the rescue history is updated whether or not anything is blurred
    auto rescue = [&]() -> int {
        if (!ctx->rescue_on() || (!c0 && !c1)) return VD_OK;
        RescueArgs a{};
        // a tiled net (vd_rescue_tiles): the merged rows hold the merged list at `low`, m_all its count
        a.cnt0 = c0; a.xy0 = x0; a.cap0 = k0; a.all0 = c0 && ctx->rescue_low[0] > 0.f ? (tiled ? tm.m_all : fp.kall) : nullptr;
        a.cnt1 = c1; a.xy1 = x1; a.cap1 = k1; a.all1 = c1 && ctx->rescue_low[1] > 0.f ? (ptiled ? pm.m_all : pp.kall) : nullptr;
        int r = ctx->launch_rescue(n, fh, fw, a);
        if (r) return r;
        dc0 = c0 = ctx->rescue_last.e_count; dx0 = x0 = ctx->rescue_last.e_xy; dk0 = k0 = ctx->rescue_last.ecap;
        dc1 = dx1 = c1 = x1 = nullptr; dk1 = k1 = 0;
        return VD_OK;
    };
    // box hold: the blur list becomes B = D ++ H in merged rows (one launch, after the lists
    // it reads are complete); the history is updated whether or not anything is blurred
    auto hold = [&]() -> int {
        if (!ctx->hold.K || (!c0 && !c1)) return VD_OK;
        int r = ctx->launch_hold(n, fh, fw, c0, x0, k0, c1, x1, k1);
        if (r) return r;
        c0 = ctx->hold_last.m_count; x0 = ctx->hold_last.m_xy; k0 = ctx->hold_last.mcap;
        c1 = x1 = nullptr; k1 = 0;
        return VD_OK;
    };
    auto mosaic = [&]() -> int {
        if (nv && lc) {   // look-ahead hold on surfaces: the m emitted ones leave through the output side
            int r = lc->m ? ctx->nv12_out_begin(*nv->out, lc->m, fh, fw, where, &nout) : VD_OK;
            if (r) return r;
            if ((r = ctx->lead_step(nin.depth ? VD_LEAD_MODE_YUV16 : VD_LEAD_MODE_NV12, nullptr, nullptr, n, fh, fw, 0, lc->flush,
                                    dc0, dx0, dk0, dc1, dx1, dk1, &nin, &nout)))
                return r;
            return lc->m ? ctx->nv12_out_finish(*nv->out, nout, lc->m, fh, fw, where) : VD_OK;
        }
        if (nv) {   // both planes, by the pass the context's blur mode asks for; host surfaces come back plane by plane
            int r = ctx->nv12_out_begin(*nv->out, n, fh, fw, where, &nout);
            if (r) return r;
            if ((r = ctx->launch_nv12_pass(nin, nout, n, fh, fw, c0, x0, k0, c1, x1, k1, ctx->nv12_cfg_pass(),
                                           ctx->cfg.mosaic_level, ctx->cells)))
                return r;
            return ctx->nv12_out_finish(*nv->out, nout, n, fh, fw, where);
        }
        uint8_t* dout = out;
        size_t bytes = (size_t)(lc ? lc->m : n) * fh * pitch;
        if (where == VD_HOST) {
            int r = ctx->ensure_staging(&ctx->stage_out, &ctx->stage_out_bytes, std::max(bytes, (size_t)1));
            if (r) return r;
            dout = (uint8_t*)ctx->stage_out;
        }
        if (lc) {   // look-ahead hold: B = D ++ H ++ A of the frames whose look-ahead is complete
            int r = ctx->lead_step(VD_LEAD_MODE_PIXELS, d, dout, n, fh, fw, pitch, lc->flush, dc0, dx0, dk0, dc1, dx1, dk1);
            if (r) return r;
            if (where == VD_HOST && bytes)
                VD_CHECK_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
            return VD_OK;
        }
        // mask shaping (vd_mask) acts here, after the hold merge, on the list being blurred only
        int r = ctx->launch_cfg_pass(d, dout, n, fh, fw, pitch, c0, x0, k0, c1, x1, k1);
        if (r) return r;
        if (where == VD_HOST) VD_CHECK_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return VD_OK;
    };
    if (mosaic_first && ((rc = rescue()) || (rc = hold()) || (rc = mosaic()))) return rc;
    if (fork) {
        VD_CHECK_HIP(hipEventRecord(ctx->ev_join, plate_stream));
        VD_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    }
    if (!mosaic_first && ((rc = rescue()) || (rc = hold()) || (do_mosaic && (rc = mosaic())))) return rc;
    int rc2 = VD_OK;
    if (do_faces) rc2 = ctx->box_finish(faces, n, tf);
    if (do_plates) {
        int rc3 = ctx->box_finish(plates, n, tp);
        if (!rc2) rc2 = rc3;
    }
    if (where == VD_HOST) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return rc2;
}

int vd_process(vd_ctx* h, const uint8_t* in, uint8_t* out, int n, int fh, int fw, size_t pitch, int where,
               int flags, vd_boxes* faces, vd_boxes* plates) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (ctx->lead.J && (flags & VD_PROC_MOSAIC))
        return vd_set_error(VD_ERR_STATE, "vd_process: MOSAIC in a look-ahead context would skip the led boxes "
                            "(use vd_process_lead)");
    if (ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_process: %d frames are pending in the look-ahead ring (flush first)",
                            ctx->lead.pend);
    return process_impl(ctx, in, out, n, fh, fw, pitch, where, flags, faces, plates, nullptr);
}

// ---- 4:2:0 frames (include/vdmi.h at vd_nv12 and vd_yuv420) ----
// One path serves both families of entries. A *_nv12 entry checks the vd_nv12 it was given (its own
// rules and messages) and goes on with the NV12 descriptor of the general form; a *_yuv420 entry
// checks the vd_yuv420. extent: the bytes the n frames span, for the overlap rule.
// A *_yuv420_16 entry checks the vd_yuv420_16 and goes on with its surfaces of 16-bit words (d.depth != 0).
struct YuvDesc { Yuv420Dev d; int matrix, range; size_t extent; };
// the descriptors a 4:2:0 entry was given: the one of its family is set
struct YuvIn { const vd_nv12* nv; const vd_yuv420* yu; const vd_yuv420_16* y16; };
static int yuv_desc(const char* who, const YuvIn& g, bool nv_entry, int n, int fh, int fw, bool colour, YuvDesc* o) {
    int rc;
    if (nv_entry) {
        if ((rc = vd_nv12_check(who, g.nv, n, fh, fw, colour))) return rc;
        o->d = vd_yuv420_dev(vd_yuv420_of_nv12(*g.nv));
        o->matrix = g.nv->matrix; o->range = g.nv->range;
        o->extent = (size_t)n * g.nv->frame_stride;
        return VD_OK;
    }
    if (g.y16) {
        if ((rc = vd_yuv420_16_check(who, g.y16, n, fh, fw, colour, &o->extent))) return rc;
        o->d = vd_yuv420_dev(*g.y16);
        o->matrix = g.y16->matrix; o->range = g.y16->range;
        return VD_OK;
    }
    if ((rc = vd_yuv420_check(who, g.yu, n, fh, fw, colour, &o->extent))) return rc;
    o->d = vd_yuv420_dev(*g.yu);
    o->matrix = g.yu ? g.yu->matrix : 0; o->range = g.yu ? g.yu->range : 0;
    return VD_OK;
}
// a 16-bit call keeps its format: no depth or shift conversion between in and out
static int yuv_same_format(const char* who, const YuvDesc& in, const YuvDesc& out) {
    if (in.d.depth != out.d.depth || in.d.shift != out.d.shift)
        return vd_set_error(VD_ERR_ARG, "%s: depth and shift of out (%d, %d) must equal in's (%d, %d): no depth conversion",
                            who, out.d.depth, out.d.shift, in.d.depth, in.d.shift);
    return VD_OK;
}

// what every blurring call checks before anything changes, after the descriptors: the one blur mode
// without a 4:2:0 pass (`pass` < 0: Ctx::nv12_cfg_pass), and (device) that the frames' whole extents
// do not overlap
static int nv12_blur_check(const char* who, const YuvDesc& in, const YuvDesc& out, int where, bool host_in_place, int pass) {
    if (pass < 0)
        return vd_set_error(VD_ERR_STATE, "%s: the fixed-kernel Gaussian (blur_mode VD_BLUR_GAUSSIAN with cells off) has "
                            "no NV12 pass: set cells (vd_cells) for the scaled smooth blur", who);
    if (in.d.base == out.d.base && !(host_in_place && where == VD_HOST))   // host frames are staged in separate buffers
        return vd_set_error(VD_ERR_ARG, "%s: out-of-place only (out must not overlap in)", who);
    if (where == VD_DEVICE) {
        const uintptr_t a = (uintptr_t)in.d.base, b = (uintptr_t)out.d.base;
        if (a < b + out.extent && b < a + in.extent)
            return vd_set_error(VD_ERR_ARG, "%s: out-of-place only (out must not overlap in)", who);
    }
    return VD_OK;
}

static int process_420(Ctx* ctx, const char* who, bool nv_entry, const YuvIn& gin, const YuvIn& gout, int n, int fh, int fw,
                       int where, int flags, vd_boxes* faces, vd_boxes* plates) {
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    YuvDesc in{}, out{};
    int rc = yuv_desc(who, gin, nv_entry, n, fh, fw, true, &in);
    if (rc) return rc;
    const bool blur = flags & VD_PROC_MOSAIC;
    if (blur) {
        if (!gout.nv && !gout.yu && !gout.y16)
            return vd_set_error(VD_ERR_ARG, "%s: MOSAIC needs an output descriptor", who);
        if ((rc = yuv_desc(who, gout, nv_entry, n, fh, fw, false, &out))) return rc;
        if ((rc = yuv_same_format(who, in, out))) return rc;
        if ((rc = nv12_blur_check(who, in, out, where, true, ctx->nv12_cfg_pass()))) return rc;
    }
    if ((rc = ctx->tiles_surfaces_check(who, flags))) return rc;
    if (ctx->lead.J && (flags & VD_PROC_MOSAIC))
        return vd_set_error(VD_ERR_STATE, "%s: MOSAIC in a look-ahead context would skip the led boxes (use "
                            "vd_process_lead_nv12)", who);
    if (ctx->lead.pend)
        return vd_set_error(VD_ERR_STATE, "%s: %d frames are pending in the look-ahead ring (flush first)", who,
                            ctx->lead.pend);
    const Nv12Call nv{&in.d, blur ? &out.d : nullptr, in.matrix, in.range};
    return process_impl(ctx, nullptr, nullptr, n, fh, fw, 0, where, flags, faces, plates, nullptr, &nv);
}

int vd_process_nv12(vd_ctx* h, const vd_nv12* in, const vd_nv12* out, int n, int fh, int fw, int where, int flags,
                    vd_boxes* faces, vd_boxes* plates) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return process_420(ctx, "vd_process_nv12", true, YuvIn{in}, YuvIn{out}, n, fh, fw, where, flags, faces, plates);
}

int vd_process_yuv420(vd_ctx* h, const vd_yuv420* in, const vd_yuv420* out, int n, int fh, int fw, int where, int flags,
                      vd_boxes* faces, vd_boxes* plates) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return process_420(ctx, "vd_process_yuv420", false, YuvIn{nullptr, in}, YuvIn{nullptr, out}, n, fh, fw, where, flags, faces,
                       plates);
}

int vd_process_yuv420_16(vd_ctx* h, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int fh, int fw, int where,
                         int flags, vd_boxes* faces, vd_boxes* plates) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!in) return vd_set_error(VD_ERR_ARG, "vd_process_yuv420_16: 16-bit 4:2:0 frames: null descriptor or base");
    return process_420(ctx, "vd_process_yuv420_16", false, YuvIn{nullptr, nullptr, in}, YuvIn{nullptr, nullptr, out}, n, fh, fw,
                       where, flags, faces, plates);
}

// The stand-alone blurring calls: pass `pass` over the caller's surfaces and one box list, with
// blur_entry's staging, capacity and overlap rules.
static int nv12_blur_entry(Ctx* ctx, const char* who, bool nv_entry, const YuvIn& gin, const YuvIn& gout, int n, int fh, int fw,
                           int where, const vd_boxes* boxes, int pass, int level, int cells) {
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    if (!boxes) return vd_set_error(VD_ERR_ARG, "%s: null argument", who);
    if (level <= 0) return vd_set_error(VD_ERR_ARG, "%s: bad geometry", who);
    YuvDesc in{}, out{};
    int rc = yuv_desc(who, gin, nv_entry, n, fh, fw, false, &in);
    if (rc) return rc;
    if ((rc = yuv_desc(who, gout, nv_entry, n, fh, fw, false, &out))) return rc;
    if ((rc = yuv_same_format(who, in, out))) return rc;
    if ((rc = nv12_blur_check(who, in, out, where, false, pass))) return rc;
    if (pass == Ctx::RECT_SMOOTH && (fh > 32768 || fw > 32768 || level > 32768))
        return vd_set_error(VD_ERR_ARG, "%s: the smooth blur needs h, w <= 32768 and level in [1, 32768] (got %d x %d, "
                            "level %d)", who, fw, fh, level);
    BoxListIn b;
    if ((rc = ctx->box_list_in(who, boxes, n, false, 0, &b))) return rc;
    Ctx::Nv12Dev din{}, dout{};
    if ((rc = ctx->nv12_in(in.d, n, fh, fw, where, &din))) return rc;
    if ((rc = ctx->nv12_out_begin(out.d, n, fh, fw, where, &dout))) return rc;
    if ((rc = ctx->launch_nv12_pass(din, dout, n, fh, fw, b.cnt, b.xy, boxes->cap, nullptr, nullptr, 0, pass, level, cells)))
        return rc;
    if ((rc = ctx->nv12_out_finish(out.d, dout, n, fh, fw, where))) return rc;
    if (where == VD_HOST || b.staged) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // host results; staging reused
    return VD_OK;
}

int vd_mosaic_nv12(vd_ctx* h, const vd_nv12* in, const vd_nv12* out, int n, int fh, int fw, int where,
                   const vd_boxes* boxes, int level) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    // the context's blur mode chooses the pass, as it does for vd_process_nv12
    return nv12_blur_entry(ctx, "vd_mosaic_nv12", true, YuvIn{in}, YuvIn{out}, n, fh, fw, where, boxes,
                           ctx->nv12_cfg_pass(), level, ctx->cells);
}

int vd_mosaic_yuv420(vd_ctx* h, const vd_yuv420* in, const vd_yuv420* out, int n, int fh, int fw, int where,
                     const vd_boxes* boxes, int level) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return nv12_blur_entry(ctx, "vd_mosaic_yuv420", false, YuvIn{nullptr, in}, YuvIn{nullptr, out}, n, fh, fw, where, boxes,
                           ctx->nv12_cfg_pass(), level, ctx->cells);
}

// a NULL vd_yuv420_16 would read as "no descriptor of this family": refuse it here
static int y16_null(const char* who, const vd_yuv420_16* in, const vd_yuv420_16* out) {
    if (!in || !out) return vd_set_error(VD_ERR_ARG, "%s: 16-bit 4:2:0 frames: null descriptor or base", who);
    return VD_OK;
}

int vd_mosaic_yuv420_16(vd_ctx* h, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int fh, int fw, int where,
                        const vd_boxes* boxes, int level) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    int rc = y16_null("vd_mosaic_yuv420_16", in, out);
    if (rc) return rc;
    return nv12_blur_entry(ctx, "vd_mosaic_yuv420_16", false, YuvIn{nullptr, nullptr, in}, YuvIn{nullptr, nullptr, out}, n, fh,
                           fw, where, boxes, ctx->nv12_cfg_pass(), level, ctx->cells);
}

static int smooth_420_args(const char* who, int level, int cells) {
    if (cells < VD_CELLS_MIN || cells > VD_CELLS_MAX)
        return vd_set_error(VD_ERR_ARG, "%s: cells %d outside [%d, %d]", who, cells, VD_CELLS_MIN, VD_CELLS_MAX);
    if (level < 1 || level > 32768) return vd_set_error(VD_ERR_ARG, "%s: level %d outside [1, 32768]", who, level);
    return VD_OK;
}

int vd_smooth_nv12(vd_ctx* h, const vd_nv12* in, const vd_nv12* out, int n, int fh, int fw, int where,
                   const vd_boxes* boxes, int level, int cells) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    int rc = smooth_420_args("vd_smooth_nv12", level, cells);
    if (rc) return rc;
    return nv12_blur_entry(ctx, "vd_smooth_nv12", true, YuvIn{in}, YuvIn{out}, n, fh, fw, where, boxes,
                           Ctx::RECT_SMOOTH, level, cells);
}

int vd_smooth_yuv420(vd_ctx* h, const vd_yuv420* in, const vd_yuv420* out, int n, int fh, int fw, int where,
                     const vd_boxes* boxes, int level, int cells) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    int rc = smooth_420_args("vd_smooth_yuv420", level, cells);
    if (rc) return rc;
    return nv12_blur_entry(ctx, "vd_smooth_yuv420", false, YuvIn{nullptr, in}, YuvIn{nullptr, out}, n, fh, fw, where, boxes,
                           Ctx::RECT_SMOOTH, level, cells);
}

int vd_smooth_yuv420_16(vd_ctx* h, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int fh, int fw, int where,
                        const vd_boxes* boxes, int level, int cells) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    int rc = smooth_420_args("vd_smooth_yuv420_16", level, cells);
    if (rc) return rc;
    if ((rc = y16_null("vd_smooth_yuv420_16", in, out))) return rc;
    return nv12_blur_entry(ctx, "vd_smooth_yuv420_16", false, YuvIn{nullptr, nullptr, in}, YuvIn{nullptr, nullptr, out}, n, fh,
                           fw, where, boxes, Ctx::RECT_SMOOTH, level, cells);
}

int vd_process_lead(vd_ctx* h, const uint8_t* in, int n, int fh, int fw, size_t pitch, int where, int flags,
                    vd_boxes* faces, vd_boxes* plates, uint8_t* out, int out_cap, int flush, int* n_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vd_process_lead";
    if (!ctx->lead.J) return vd_set_error(VD_ERR_STATE, "%s: look-ahead hold is off (vd_lead)", who);
    if (!(flags & VD_PROC_MOSAIC)) return vd_set_error(VD_ERR_ARG, "%s: flags must include VD_PROC_MOSAIC", who);
    if (!(flags & VD_PROC_FACES) && !(flags & VD_PROC_MOSAIC_PLATES))
        return vd_set_error(VD_ERR_ARG, "%s: nothing to blur (FACES or MOSAIC_PLATES needed)", who);
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    if (out_cap < 0 || (n > 0 && !in)) return vd_set_error(VD_ERR_ARG, "%s: null input / negative out_cap", who);
    if (pitch < (size_t)(fw > 0 ? fw : 0) * 3) return vd_set_error(VD_ERR_ARG, "%s: bad pitch", who);
    if (n == 0 && flush && !ctx->lead.pend) {      // the end of an empty stream
        if (n_out) *n_out = 0;
        return VD_OK;
    }
    int rc = ctx->lead_check(who, VD_LEAD_MODE_PIXELS, n, fh, fw, pitch, flush);
    if (rc) return rc;
    const int m = ctx->lead.emit(n, flush);
    if (m > out_cap)
        return vd_set_error(VD_ERR_CAPACITY, "%s: %d frames to emit, out holds %d", who, m, out_cap);
    if (m > 0 && !out) return vd_set_error(VD_ERR_ARG, "%s: MOSAIC needs an output buffer", who);
    const size_t fb = (size_t)fh * pitch;
    if (where == VD_DEVICE && n > 0 && m > 0) {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        if (a < b + (size_t)m * fb && b < a + (size_t)n * fb)
            return vd_set_error(VD_ERR_ARG, "%s: out must not overlap in", who);
    }
    const LeadCall lc{flush, m};
    if (n > 0) {
        rc = process_impl(ctx, in, out, n, fh, fw, pitch, where, flags, faces, plates, &lc);
    } else {      // flush alone: the pending frames leave, no detection
        uint8_t* dout = out;
        const size_t bytes = (size_t)m * fb;
        if (where == VD_HOST) {
            if ((rc = ctx->ensure_staging(&ctx->stage_out, &ctx->stage_out_bytes, bytes))) return rc;
            dout = (uint8_t*)ctx->stage_out;
        }
        rc = ctx->lead_step(VD_LEAD_MODE_PIXELS, nullptr, dout, 0, fh, fw, pitch, 1, nullptr, nullptr, 0, nullptr, nullptr, 0);
        if (!rc && where == VD_HOST) {
            VD_CHECK_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
            VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    if (rc) return rc;
    if (n_out) *n_out = m;
    return VD_OK;
}

// vd_process_lead on NV12 surfaces: vd_process_lead's rules with vd_process_nv12's descriptors. Every
// refusal comes before anything changes; `out` describes out_cap surfaces, of which m are written.
int vd_process_lead_nv12(vd_ctx* h, const vd_nv12* in, const vd_nv12* out, int n, int fh, int fw, int where, int flags,
                         vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const char* who = "vd_process_lead_nv12";
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    if (n < 0 || out_cap < 0) return vd_set_error(VD_ERR_ARG, "%s: negative n / out_cap", who);
    int rc;
    if (n > 0) {
        if ((rc = vd_nv12_check(who, in, n, fh, fw, true))) return rc;
    } else if (fh <= 0 || fw <= 0 || (fh & 1) || (fw & 1)) {
        return vd_set_error(VD_ERR_ARG, "%s: NV12 frames: even, positive h and w required (got %d x %d)", who, fw, fh);
    }
    if (!ctx->lead.J) return vd_set_error(VD_ERR_STATE, "%s: look-ahead hold is off (vd_lead)", who);
    if (!(flags & VD_PROC_MOSAIC)) return vd_set_error(VD_ERR_ARG, "%s: flags must include VD_PROC_MOSAIC", who);
    if (!(flags & VD_PROC_FACES) && !(flags & VD_PROC_MOSAIC_PLATES))
        return vd_set_error(VD_ERR_ARG, "%s: nothing to blur (FACES or MOSAIC_PLATES needed)", who);
    if (n == 0 && flush && !ctx->lead.pend) {      // the end of an empty stream
        if (n_out) *n_out = 0;
        return VD_OK;
    }
    if (ctx->nv12_cfg_pass() < 0)
        return vd_set_error(VD_ERR_STATE, "%s: the fixed-kernel Gaussian (blur_mode VD_BLUR_GAUSSIAN with cells off) has "
                            "no NV12 pass: set cells (vd_cells) for the scaled smooth blur", who);
    if (n > 0 && (rc = ctx->tiles_surfaces_check(who, flags))) return rc;
    if ((rc = ctx->lead_check(who, VD_LEAD_MODE_NV12, n, fh, fw, 0, flush))) return rc;
    const int m = ctx->lead.emit(n, flush);
    if (m > out_cap) return vd_set_error(VD_ERR_CAPACITY, "%s: %d frames to emit, out holds %d", who, m, out_cap);
    if (m > 0) {
        if (!out) return vd_set_error(VD_ERR_ARG, "%s: MOSAIC needs an output descriptor", who);
        if ((rc = vd_nv12_check(who, out, m, fh, fw, false))) return rc;
        if (where == VD_DEVICE && n > 0) {
            const uintptr_t a = (uintptr_t)in->base, b = (uintptr_t)out->base;
            if (a < b + (size_t)m * out->frame_stride && b < a + (size_t)n * in->frame_stride)
                return vd_set_error(VD_ERR_ARG, "%s: out must not overlap in", who);
        }
    }
    const LeadCall lc{flush, m};
    if (n > 0) {
        const Yuv420Dev yin = vd_yuv420_dev(vd_yuv420_of_nv12(*in)), yout = out ? vd_yuv420_dev(vd_yuv420_of_nv12(*out)) : Yuv420Dev{};
        const Nv12Call nv{&yin, out ? &yout : nullptr, in->matrix, in->range};
        rc = process_impl(ctx, nullptr, nullptr, n, fh, fw, 0, where, flags, faces, plates, &lc, &nv);
    } else {      // flush alone: the pending surfaces leave, no detection
        Ctx::Nv12Dev nin{}, nout{};
        const Yuv420Dev yout = vd_yuv420_dev(vd_yuv420_of_nv12(*out));
        if ((rc = ctx->nv12_out_begin(yout, m, fh, fw, where, &nout))) return rc;
        if ((rc = ctx->lead_step(VD_LEAD_MODE_NV12, nullptr, nullptr, 0, fh, fw, 0, 1, nullptr, nullptr, 0, nullptr, nullptr,
                                 0, &nin, &nout)))
            return rc;
        if ((rc = ctx->nv12_out_finish(yout, nout, m, fh, fw, where))) return rc;
        if (where == VD_HOST) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (rc) return rc;
    if (n_out) *n_out = m;
    return VD_OK;
}

// vd_process_lead_nv12 on any layout of vd_yuv420, or on the 16-bit words of vd_yuv420_16: the same rules
// with the descriptor checks of vd_process_yuv420 / vd_process_yuv420_16. The 8-bit family shares the NV12
// entry's ring and pending mode; 16-bit words have a ring form and a mode of their own, with depth and
// shift part of the pending geometry.
static int process_lead_420(Ctx* ctx, const char* who, const YuvIn& gin, const YuvIn& gout, bool words, int n, int fh, int fw,
                            int where, int flags, vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out) {
    if (where != VD_HOST && where != VD_DEVICE) return vd_set_error(VD_ERR_ARG, "%s: bad where", who);
    if (n < 0 || out_cap < 0) return vd_set_error(VD_ERR_ARG, "%s: negative n / out_cap", who);
    int rc;
    YuvDesc in{}, out{};
    if (n > 0) {
        if (words && !gin.y16) return vd_set_error(VD_ERR_ARG, "%s: 16-bit 4:2:0 frames: null descriptor or base", who);
        if ((rc = yuv_desc(who, gin, false, n, fh, fw, true, &in))) return rc;
    } else if (fh <= 0 || fw <= 0 || (fh & 1) || (fw & 1)) {
        return vd_set_error(VD_ERR_ARG, "%s: 4:2:0 frames: even, positive h and w required (got %d x %d)", who, fw, fh);
    }
    if (!ctx->lead.J) return vd_set_error(VD_ERR_STATE, "%s: look-ahead hold is off (vd_lead)", who);
    if (!(flags & VD_PROC_MOSAIC)) return vd_set_error(VD_ERR_ARG, "%s: flags must include VD_PROC_MOSAIC", who);
    if (!(flags & VD_PROC_FACES) && !(flags & VD_PROC_MOSAIC_PLATES))
        return vd_set_error(VD_ERR_ARG, "%s: nothing to blur (FACES or MOSAIC_PLATES needed)", who);
    if (n == 0 && flush && !ctx->lead.pend) {      // the end of an empty stream
        if (n_out) *n_out = 0;
        return VD_OK;
    }
    if (ctx->nv12_cfg_pass() < 0)
        return vd_set_error(VD_ERR_STATE, "%s: the fixed-kernel Gaussian (blur_mode VD_BLUR_GAUSSIAN with cells off) has "
                            "no NV12 pass: set cells (vd_cells) for the scaled smooth blur", who);
    if (n > 0 && (rc = ctx->tiles_surfaces_check(who, flags))) return rc;
    // the words' format: the input's, or for a flush alone the output's (none given: nothing to compare)
    int depth = 0, shift = 0;
    if (words) {
        depth = n > 0 ? in.d.depth : gout.y16 ? gout.y16->depth : ctx->lead.depth;
        shift = n > 0 ? in.d.shift : gout.y16 ? gout.y16->shift : ctx->lead.shift;
    }
    const int mode = words ? VD_LEAD_MODE_YUV16 : VD_LEAD_MODE_NV12;
    if ((rc = ctx->lead_check(who, mode, n, fh, fw, 0, flush, depth, shift))) return rc;
    const int m = ctx->lead.emit(n, flush);
    if (m > out_cap) return vd_set_error(VD_ERR_CAPACITY, "%s: %d frames to emit, out holds %d", who, m, out_cap);
    if (m > 0) {
        if (!gout.yu && !gout.y16) return vd_set_error(VD_ERR_ARG, "%s: MOSAIC needs an output descriptor", who);
        if ((rc = yuv_desc(who, gout, false, m, fh, fw, false, &out))) return rc;
        if (n > 0 && (rc = yuv_same_format(who, in, out))) return rc;
        if (where == VD_DEVICE && n > 0) {
            const uintptr_t a = (uintptr_t)in.d.base, b = (uintptr_t)out.d.base;
            if (a < b + out.extent && b < a + in.extent) return vd_set_error(VD_ERR_ARG, "%s: out must not overlap in", who);
        }
    }
    const LeadCall lc{flush, m};
    if (n > 0) {
        const Nv12Call nv{&in.d, m > 0 ? &out.d : nullptr, in.matrix, in.range};
        rc = process_impl(ctx, nullptr, nullptr, n, fh, fw, 0, where, flags, faces, plates, &lc, &nv);
    } else {      // flush alone: the pending surfaces leave, no detection
        Ctx::Nv12Dev nin{}, nout{};
        if ((rc = ctx->nv12_out_begin(out.d, m, fh, fw, where, &nout))) return rc;
        if ((rc = ctx->lead_step(mode, nullptr, nullptr, 0, fh, fw, 0, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, &nin, &nout)))
            return rc;
        if ((rc = ctx->nv12_out_finish(out.d, nout, m, fh, fw, where))) return rc;
        if (where == VD_HOST) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (rc) return rc;
    if (n_out) *n_out = m;
    return VD_OK;
}

int vd_process_lead_yuv420(vd_ctx* h, const vd_yuv420* in, const vd_yuv420* out, int n, int fh, int fw, int where, int flags,
                           vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return process_lead_420(ctx, "vd_process_lead_yuv420", YuvIn{nullptr, in}, YuvIn{nullptr, out}, false, n, fh, fw, where,
                            flags, faces, plates, out_cap, flush, n_out);
}

int vd_process_lead_yuv420_16(vd_ctx* h, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int fh, int fw, int where,
                              int flags, vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return process_lead_420(ctx, "vd_process_lead_yuv420_16", YuvIn{nullptr, nullptr, in}, YuvIn{nullptr, nullptr, out}, true, n,
                            fh, fw, where, flags, faces, plates, out_cap, flush, n_out);
}

int vd_read_boxes(vd_ctx* h, int net, int n, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    const PostScratch* ps = net == VD_NET_RETINAFACE ? &ctx->face.post : (net == VD_NET_YOLOV8N ? &ctx->plate.post : nullptr);
    if (!ps) return vd_set_error(VD_ERR_ARG, "unknown net %d", net);
    if (!ps->kcount) return vd_set_error(VD_ERR_STATE, "net %d not loaded", net);
    if (!out || !out->count || !out->xyxy || out->cap <= 0) return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    // tiled detection: the lists of a tiled net's last call are the merged rows (tiles.hip)
    const bool face = net == VD_NET_RETINAFACE;
    const bool mg = face ? ctx->face_rows_merged : ctx->plate_rows_merged;
    const TileMergeArgs& tm = face ? ctx->tiles_last : ctx->ptiles_last;
    const int kn = mg ? (face ? ctx->tiles_kn : ctx->ptiles_kn) : ps->kn, kcap = mg ? tm.mcap : ps->kcap;
    const int* kcount = mg ? tm.m_count : ps->kcount;
    const int* kxyxy = mg ? tm.m_xyxy : ps->kxyxy;
    const float* kxyxy_f = mg ? tm.m_xyxy_f : ps->kxyxy_f;
    const float* kscore = mg ? tm.m_score : ps->kscore;
    const int* klabel = mg ? tm.m_label : ps->klabel;
    if (n <= 0 || n > kn) return vd_set_error(VD_ERR_ARG, "n=%d outside [1, %d frames of the last call]", n, kn);
    const hipMemcpyKind kind = out->where == VD_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const int w = std::min(out->cap, kcap);   // boxes per frame copied (beyond kcap nothing is ever kept)
    const size_t dp = (size_t)out->cap, sp = (size_t)kcap;
    VD_CHECK_HIP(hipMemcpyAsync(out->count, kcount, (size_t)n * 4, kind, ctx->stream));
    VD_CHECK_HIP(hipMemcpy2DAsync(out->xyxy, dp * 16, kxyxy, sp * 16, (size_t)w * 16, n, kind, ctx->stream));
    if (out->xyxy_f)
        VD_CHECK_HIP(hipMemcpy2DAsync(out->xyxy_f, dp * 16, kxyxy_f, sp * 16, (size_t)w * 16, n, kind, ctx->stream));
    if (out->score)
        VD_CHECK_HIP(hipMemcpy2DAsync(out->score, dp * 4, kscore, sp * 4, (size_t)w * 4, n, kind, ctx->stream));
    if (out->label)
        VD_CHECK_HIP(hipMemcpy2DAsync(out->label, dp * 4, klabel, sp * 4, (size_t)w * 4, n, kind, ctx->stream));
    if (out->where == VD_HOST) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VD_OK;
}

int vd_mask(vd_ctx* h, int shape, int grow_pct) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (shape != VD_MASK_RECT && shape != VD_MASK_ELLIPSE)
        return vd_set_error(VD_ERR_ARG, "vd_mask: shape %d (expected 0 = rect or 1 = ellipse)", shape);
    if (grow_pct < 0 || grow_pct > VD_MASK_GROW_MAX)
        return vd_set_error(VD_ERR_ARG, "vd_mask: grow_pct %d outside [0, %d]", grow_pct, VD_MASK_GROW_MAX);
    ctx->mask_shape = shape;
    ctx->mask_grow = grow_pct;
    return VD_OK;
}

int vd_cells(vd_ctx* h, int cells) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (cells != 0 && (cells < VD_CELLS_MIN || cells > VD_CELLS_MAX))
        return vd_set_error(VD_ERR_ARG, "vd_cells: %d (expected 0 = off or [%d, %d])", cells, VD_CELLS_MIN,
                            VD_CELLS_MAX);
    ctx->cells = cells;
    return VD_OK;
}

int vd_cell_level(int W, int H, int level, int cells) {
    if (level < 1 || (cells != 0 && (cells < VD_CELLS_MIN || cells > VD_CELLS_MAX)))
        return vd_set_error(VD_ERR_ARG, "vd_cell_level: level >= 1 and cells 0 or in [%d, %d] required (got %d, %d)",
                            VD_CELLS_MIN, VD_CELLS_MAX, level, cells);
    return vd_cell_level_hd((long long)W, (long long)H, level, cells);
}

int vd_mask_boxes(vd_ctx* h, const vd_boxes* in, int n, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!out || !out->count || !out->xyxy || out->cap <= 0)
        return vd_set_error(VD_ERR_ARG, "vd_mask_boxes: vd_boxes needs count, xyxy, cap>0");
    if (n <= 0) return vd_set_error(VD_ERR_ARG, "vd_mask_boxes: n=%d", n);
    BoxListIn b;
    int rc = ctx->box_list_in("vd_mask_boxes", in, n, false, 0, &b);
    if (rc) return rc;
    // the blur path's kernel; whole rows are copied out, so entries past the count are zeroed
    if ((rc = ctx->launch_mask_grow(n, b.cnt, b.xy, in->cap, nullptr, nullptr, 0, 1))) return rc;
    const hipMemcpyKind kind = out->where == VD_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t wb = (size_t)std::min(in->cap, out->cap) * 16;
    VD_CHECK_HIP(hipMemcpyAsync(out->count, b.cnt, (size_t)n * 4, kind, ctx->stream));   // complete counts, as given
    VD_CHECK_HIP(hipMemcpy2DAsync(out->xyxy, (size_t)out->cap * 16, ctx->mask_last.m_xy, (size_t)in->cap * 16, wb, n,
                                  kind, ctx->stream));
    if (b.staged || out->where == VD_HOST) VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused, host results
    return VD_OK;
}

}  // extern "C"
