// frames.cpp — frames and box lists in and out of the device; the face path around the net
// (letterbox, forward, post) and tiled detection.

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

// cv2.resize mode selection (resize.cpp hal::resize [ext]; oracle/letterbox.py)
void vd_resize_mode(int ih, int iw, int nh, int nw, int* mode, double* sx, double* sy) {
    if (nh == ih && nw == iw) { *mode = LB_COPY; *sx = *sy = 1.0; return; }
    double inv_x = (double)nw / iw, inv_y = (double)nh / ih;
    double scx = 1.0 / inv_x, scy = 1.0 / inv_y;
    int isx = (int)std::nearbyint(scx), isy = (int)std::nearbyint(scy);
    bool area_fast = std::fabs(scx - isx) < 2.220446049250313e-16 && std::fabs(scy - isy) < 2.220446049250313e-16;
    *mode = (area_fast && isx == 2 && isy == 2) ? LB_AREA2 : LB_LINEAR;
    *sx = scx;
    *sy = scy;
}

const uint8_t* Ctx::frames_to_device(const uint8_t* frames, int n, int h, size_t pitch, int where, int* rc) {
    *rc = VD_OK;
    if (where == VD_DEVICE) return frames;
    size_t bytes = (size_t)n * h * pitch;
    *rc = ensure_staging(&stage_in, &stage_in_bytes, bytes);
    if (*rc) return nullptr;
    hipError_t e = hipMemcpyAsync(stage_in, frames, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
        *rc = vd_set_error(VD_ERR_HIP, "H2D frames: %s", hipGetErrorString(e));
        return nullptr;
    }
    return (const uint8_t*)stage_in;
}

int Ctx::check_frames(int n, int h, int w, size_t pitch) {
    if (n <= 0 || n > cfg.max_batch) return vd_set_error(VD_ERR_ARG, "n=%d outside [1, max_batch=%d]", n, cfg.max_batch);
    if (h <= 0 || w <= 0 || pitch < (size_t)w * 3) return vd_set_error(VD_ERR_ARG, "bad frame geometry %dx%d pitch %zu", w, h, pitch);
    return VD_OK;
}

// ---- NV12 surfaces (include/vdmi.h at vd_nv12) ----
int vd_nv12_check(const char* who, const vd_nv12* d, int n, int h, int w, bool colour) {
    static const char* const rule[] = {"", "null descriptor or base", "n > 0 and even, positive h and w required",
                                       "pitch < w (or >= 2^31)", "uv_offset < h * pitch (or >= 2^47)",
                                       "frame_stride < uv_offset + (h/2) * pitch (or >= 2^47)", "unknown matrix",
                                       "unknown range"};
    const int r = vd_nv12_layout(d, n, h, w, colour);
    if (!r) return VD_OK;
    if (r == 1) return vd_set_error(VD_ERR_ARG, "%s: NV12 frames: %s", who, rule[r]);
    return vd_set_error(VD_ERR_ARG, "%s: NV12 frames: %s (n=%d, %d x %d, pitch %zu, uv_offset %zu, frame_stride %zu, "
                        "matrix %d, range %d)", who, rule[r], n, w, h, d->pitch, d->uv_offset, d->frame_stride, d->matrix,
                        d->range);
}

int vd_yuv420_check(const char* who, const vd_yuv420* d, int n, int h, int w, bool colour, size_t* extent) {
    static const char* const rule[] = {"", "null descriptor or base", "n > 0 and even, positive h and w required",
                                       "pitch < w (or >= 2^31)", "chroma_step outside {1, 2}",
                                       "chroma_pitch < (w/2) * chroma_step (or >= 2^31)",
                                       "chroma_step 2 needs |u_offset - v_offset| == 1",
                                       "u_offset: the U plane overlaps the luma plane (or >= 2^47)",
                                       "v_offset: the V plane overlaps the luma or the U plane (or >= 2^47)",
                                       "frame_stride: a plane reaches past it (or >= 2^47)", "unknown matrix",
                                       "unknown range"};
    size_t end = 0;
    const int r = vd_yuv420_layout(d, n, h, w, colour, &end);
    if (!r) {
        if (extent) *extent = (size_t)(n - 1) * d->frame_stride + end;
        return VD_OK;
    }
    if (r == 1) return vd_set_error(VD_ERR_ARG, "%s: 4:2:0 frames: %s", who, rule[r]);
    return vd_set_error(VD_ERR_ARG, "%s: 4:2:0 frames: %s (n=%d, %d x %d, pitch %zu, u_offset %zu, v_offset %zu, "
                        "chroma_pitch %zu, chroma_step %d, frame_stride %zu, matrix %d, range %d)", who, rule[r], n, w, h,
                        d->pitch, d->u_offset, d->v_offset, d->chroma_pitch, d->chroma_step, d->frame_stride, d->matrix,
                        d->range);
}

int vd_yuv420_16_check(const char* who, const vd_yuv420_16* d, int n, int h, int w, bool colour, size_t* extent) {
    static const char* const rule[] = {"", "null descriptor or base", "n > 0 and even, positive h and w required",
                                       "pitch < 2 * w, odd (or >= 2^31)", "chroma_step outside {1, 2}",
                                       "chroma_pitch < w * chroma_step, odd (or >= 2^31)",
                                       "chroma_step 2 needs |u_offset - v_offset| == 2",
                                       "u_offset: odd, or the U plane overlaps the luma plane (or >= 2^47)",
                                       "v_offset: odd, or the V plane overlaps the luma or the U plane (or >= 2^47)",
                                       "frame_stride: odd, or a plane reaches past it (or >= 2^47)", "unknown matrix",
                                       "unknown range", "depth outside {10, 12}", "shift outside [0, 16 - depth]",
                                       "base is not 2-byte aligned"};
    size_t end = 0;
    const int r = vd_yuv420_16_layout(d, n, h, w, colour, &end);
    if (!r) {
        if (extent) *extent = (size_t)(n - 1) * d->frame_stride + end;
        return VD_OK;
    }
    if (r == 1) return vd_set_error(VD_ERR_ARG, "%s: 16-bit 4:2:0 frames: %s", who, rule[r]);
    return vd_set_error(VD_ERR_ARG, "%s: 16-bit 4:2:0 frames: %s (n=%d, %d x %d, pitch %zu, u_offset %zu, v_offset %zu, "
                        "chroma_pitch %zu, chroma_step %d, frame_stride %zu, matrix %d, range %d, depth %d, shift %d)", who,
                        rule[r], n, w, h, d->pitch, d->u_offset, d->v_offset, d->chroma_pitch, d->chroma_step,
                        d->frame_stride, d->matrix, d->range, d->depth, d->shift);
}

// The planes of one frame between a caller's host layout c and its packed staging o (the same
// step and plane order): the picture's bytes of every row only, 1.5 B/px (16-bit words: 3 B/px).
static int yuv420_copy_planes(const Yuv420Dev& c, const Yuv420Dev& o, int n, int h, int w, bool to_device, hipStream_t stream) {
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const size_t es = (size_t)c.es();
    // interleaved: one chroma plane of w bytes a row from the lower offset; planar: U and V of w / 2
    const size_t coff[2][2] = {{c.step == 2 ? c.c0() : c.u, c.step == 2 ? o.c0() : o.u}, {c.v, o.v}};
    const int nchroma = c.step == 2 ? 1 : 2;
    const size_t crow = (c.step == 2 ? (size_t)w : (size_t)(w / 2)) * es, lrow = (size_t)w * es;
    for (int f = 0; f < n; ++f) {
        uint8_t* hp = c.base + (size_t)f * c.stride;
        uint8_t* dp = o.base + (size_t)f * o.stride;
        if (to_device) VD_CHECK_HIP(hipMemcpy2DAsync(dp, o.pitch, hp, c.pitch, lrow, h, kind, stream));
        else VD_CHECK_HIP(hipMemcpy2DAsync(hp, c.pitch, dp, o.pitch, lrow, h, kind, stream));
        for (int p = 0; p < nchroma; ++p) {
            if (to_device)
                VD_CHECK_HIP(hipMemcpy2DAsync(dp + coff[p][1], o.cpitch, hp + coff[p][0], c.cpitch, crow, h / 2, kind, stream));
            else
                VD_CHECK_HIP(hipMemcpy2DAsync(hp + coff[p][0], c.cpitch, dp + coff[p][1], o.cpitch, crow, h / 2, kind, stream));
        }
    }
    return VD_OK;
}

int Ctx::nv12_in(const Nv12Dev& d, int n, int h, int w, int where, Nv12Dev* o) {
    if (where == VD_DEVICE) {
        *o = d;
        return VD_OK;
    }
    int rc = ensure_staging(&stage_in, &stage_in_bytes, (size_t)n * h * w / 2 * 3 * d.es());
    if (rc) return rc;
    *o = vd_yuv420_packed(stage_in, h, w, d.step, d.v < d.u, d.depth, d.shift);
    return yuv420_copy_planes(d, *o, n, h, w, true, stream);
}

int Ctx::nv12_out_begin(const Nv12Dev& d, int n, int h, int w, int where, Nv12Dev* o) {
    if (where == VD_DEVICE) {
        *o = d;
        return VD_OK;
    }
    int rc = ensure_staging(&stage_out, &stage_out_bytes, (size_t)n * h * w / 2 * 3 * d.es());
    if (rc) return rc;
    *o = vd_yuv420_packed(stage_out, h, w, d.step, d.v < d.u, d.depth, d.shift);
    return VD_OK;
}

int Ctx::nv12_out_finish(const Nv12Dev& d, const Nv12Dev& o, int n, int h, int w, int where) {
    if (where == VD_DEVICE) return VD_OK;
    return yuv420_copy_planes(d, o, n, h, w, false, stream);   // pad bytes and the bytes between the planes are not written
}

extern "C" int vd_yuv420_to_rgb(const vd_yuv420* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    int rc = vd_yuv420_check("vd_yuv420_to_rgb", in, n, h, w, true);
    if (rc) return rc;
    if (!rgb || rgb_pitch < (size_t)w * 3) return vd_set_error(VD_ERR_ARG, "vd_yuv420_to_rgb: null rgb or rgb_pitch < 3 * w");
    vd_yuv420_to_rgb_host(in, n, h, w, rgb, rgb_pitch);
    return VD_OK;
}

extern "C" int vd_yuv420_16_to_rgb(const vd_yuv420_16* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    int rc = vd_yuv420_16_check("vd_yuv420_16_to_rgb", in, n, h, w, true);
    if (rc) return rc;
    if (!rgb || rgb_pitch < (size_t)w * 3) return vd_set_error(VD_ERR_ARG, "vd_yuv420_16_to_rgb: null rgb or rgb_pitch < 3 * w");
    vd_yuv420_16_to_rgb_host(in, n, h, w, rgb, rgb_pitch);
    return VD_OK;
}

extern "C" int vd_nv12_to_rgb(const vd_nv12* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch) {
    int rc = vd_nv12_check("vd_nv12_to_rgb", in, n, h, w, true);
    if (rc) return rc;
    if (!rgb || rgb_pitch < (size_t)w * 3) return vd_set_error(VD_ERR_ARG, "vd_nv12_to_rgb: null rgb or rgb_pitch < 3 * w");
    vd_nv12_to_rgb_host(in, n, h, w, rgb, rgb_pitch);
    return VD_OK;
}

// Box outputs: kernels write straight into caller arrays when they are device
// memory; host outputs go through ctx staging + one D2H at the end. `out` may be
// NULL (no caller copy; the complete lists stay readable through vd_read_boxes).
int Ctx::box_targets(vd_boxes* out, int n, BoxTargets& t) {
    t = BoxTargets{};
    if (!out) return VD_OK;
    if (!out->count || !out->xyxy || out->cap <= 0) return vd_set_error(VD_ERR_ARG, "vd_boxes needs count, xyxy, cap>0");
    t.cap = out->cap;
    if (out->where == VD_DEVICE) {
        t.count = out->count; t.xyxy = out->xyxy; t.xyxy_f = out->xyxy_f; t.score = out->score; t.label = out->label;
        return VD_OK;
    }
    return host_box_staging(&stage_box, &stage_box_bytes, out->cap, n, t);
}

int Ctx::host_box_staging(void** buf, size_t* have, int cap, int n, BoxTargets& t) {
    size_t nb = (size_t)n * cap;
    size_t need = n * 4 + nb * (16 + 16 + 4 + 4);
    int rc = ensure_staging(buf, have, need + 64);
    if (rc) return rc;
    char* p = (char*)*buf;
    t.cap = cap;
    t.count = (int*)p; p += ((n * 4 + 15) / 16) * 16;
    t.xyxy = (int*)p; p += nb * 16;
    t.xyxy_f = (float*)p; p += nb * 16;
    t.score = (float*)p; p += nb * 4;
    t.label = (int*)p;
    return VD_OK;
}

// Host outputs: one D2H of the staged arrays. count[f] is the complete keep count,
// which may exceed cap: the arrays then hold the first cap boxes, the rest stay
// readable through vd_read_boxes, and the mosaic used every box regardless.
int Ctx::box_finish(vd_boxes* out, int n, const BoxTargets& t) {
    if (!out || out->where == VD_DEVICE) return VD_OK;
    size_t nb = (size_t)n * out->cap;
    VD_CHECK_HIP(hipMemcpyAsync(out->count, t.count, n * 4, hipMemcpyDeviceToHost, stream));
    VD_CHECK_HIP(hipMemcpyAsync(out->xyxy, t.xyxy, nb * 16, hipMemcpyDeviceToHost, stream));
    if (out->xyxy_f) VD_CHECK_HIP(hipMemcpyAsync(out->xyxy_f, t.xyxy_f, nb * 16, hipMemcpyDeviceToHost, stream));
    if (out->score) VD_CHECK_HIP(hipMemcpyAsync(out->score, t.score, nb * 4, hipMemcpyDeviceToHost, stream));
    if (out->label) VD_CHECK_HIP(hipMemcpyAsync(out->label, t.label, nb * 4, hipMemcpyDeviceToHost, stream));
    VD_CHECK_HIP(hipStreamSynchronize(stream));
    return VD_OK;
}

int vd_count_check(const char* who, const int* count, int rows, int cap) {
    for (int i = 0; i < rows; ++i)
        if (count[i] > cap)
            return vd_set_error(VD_ERR_CAPACITY, "%s: list %d has count %d > cap %d", who, i, count[i], cap);
    return VD_OK;
}

int Ctx::box_list_in(const char* who, const vd_boxes* b, int rows, bool vec16, size_t stage_off, BoxListIn* o,
                     size_t stage_bytes) {
    if (!b || !b->count || !b->xyxy || b->cap <= 0)
        return vd_set_error(VD_ERR_ARG, "%s: vd_boxes needs count, xyxy, cap>0", who);
    const bool host = b->where == VD_HOST;
    int rc;
    if (host && (rc = vd_count_check(who, b->count, rows, b->cap))) return rc;
    o->cnt = b->count;
    o->xy = b->xyxy;
    o->staged = host || (vec16 && ((uintptr_t)b->xyxy & 15));
    if (!o->staged) return VD_OK;
    const size_t nb = (size_t)rows * b->cap;
    if ((rc = ensure_staging(&stage_box2, &stage_box2_bytes,
                             std::max(stage_bytes, stage_off + (size_t)rows * 4 + nb * 16 + 16))))
        return rc;
    int* dc = (int*)((char*)stage_box2 + stage_off);
    int* dx = dc + ((rows + 3) / 4) * 4;          // the boxes start 16-byte aligned
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    VD_CHECK_HIP(hipMemcpyAsync(dc, b->count, (size_t)rows * 4, kind, stream));
    VD_CHECK_HIP(hipMemcpyAsync(dx, b->xyxy, nb * 16, kind, stream));
    o->cnt = dc;
    o->xy = dx;
    return VD_OK;
}

int Ctx::rows_out(const HoldArgs& view, int n, int held_only, vd_boxes* out, const char* what) {
    BoxTargets t{};
    if (out->where == VD_DEVICE) {
        t.count = out->count; t.xyxy = out->xyxy; t.label = out->label;
    } else {
        int rc = host_box_staging(&stage_box, &stage_box_bytes, out->cap, n, t);
        if (rc) return rc;
        if (!out->label) t.label = nullptr;
    }
    hipError_t e = vd_launch_hold_gather(view, n, held_only, t.count, t.xyxy, t.label, out->cap, stream);
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "%s gather: %s", what, hipGetErrorString(e));
    if (out->where == VD_DEVICE) return VD_OK;
    // arrays past min(count, cap) are not written by the gather: copy whole arrays as box_finish does
    const size_t nbx = (size_t)n * out->cap;
    VD_CHECK_HIP(hipMemcpyAsync(out->count, t.count, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    VD_CHECK_HIP(hipMemcpyAsync(out->xyxy, t.xyxy, nbx * 16, hipMemcpyDeviceToHost, stream));
    if (out->label) VD_CHECK_HIP(hipMemcpyAsync(out->label, t.label, nbx * 4, hipMemcpyDeviceToHost, stream));
    VD_CHECK_HIP(hipStreamSynchronize(stream));
    return VD_OK;
}

int Ctx::face_letterbox(const uint8_t* dframes, int n, int h, int w, size_t pitch) {
    LetterboxArgs a;
    face_letterbox_args(dframes, n, h, w, pitch, &a);
    t_begin(2, (double)n * (a.nh * (double)w * vd_src_bpp(a.nv) + (double)a.oh * a.ow * a.cpad * (f32 ? 4 : 2)));
    hipError_t e = vd_launch_letterbox(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "letterbox: %s", hipGetErrorString(e));
    return VD_OK;
}

void Ctx::face_letterbox_args(const uint8_t* dframes, int n, int h, int w, size_t pitch, LetterboxArgs* out) {
    LetterboxArgs a{};
    a.src = dframes; a.n = n; a.ih = h; a.iw = w; a.pitch = pitch;
    a.nv = nv12_src;       // an NV12 call in flight: dframes / pitch describe the surfaces
    a.oh = face.in_h; a.ow = face.in_w;
    // utils/utils.py:9-13 (Python doubles)
    double scale = std::min((double)a.ow / w, (double)a.oh / h);
    a.nw = (int)(w * scale);
    a.nh = (int)(h * scale);
    a.top = (a.oh - a.nh) / 2;
    a.left = (a.ow - a.nw) / 2;
    vd_resize_mode(h, w, a.nh, a.nw, &a.mode, &a.scale_x, &a.scale_y);
    a.pad_value = 128.f;
    a.mean[0] = 104.f; a.mean[1] = 117.f; a.mean[2] = 123.f;
    a.div = 1.f;
    a.flip = 0;
    // fp32 plan with the fused stem: an fp16 space-to-depth canvas (integer values, exact)
    a.out = face.input.p; a.cpad = face.input.c; a.out_f32 = face.input.f32 ? 1 : 0;
    a.out_f16 = (f16 || (f32 && !face.input.f32)) ? 1 : 0;
    a.s2d = face.s2d ? 1 : 0;
    const int geom[6] = {h, w, a.top, a.nh, a.left, a.nw};
    memcpy(bands.geom, geom, sizeof geom);                // what the next plain forward's canvases look like
    *out = a;
}

// ---- letterbox bands (face_bands.h, bands.hip) ----
int Ctx::bands_alloc() {
    bands.plan = false;
    const Net& net = face.net;
    if (!f32 || tune.f32_split != 2 || face.mnet || cfg.max_batch > VD_BAND_FRAMES) return VD_OK;
    // the four band ops: the fused stem + pool, then layer1 as three fused fp32 bottlenecks
    if (net.stage_end[0] != 1 || net.stage_end[1] != 4 || net.ops.size() < 4 || net.ops[0].kind != OP_STEMPOOL ||
        !net.ops[0].y.f32 || !net.ops[0].y.amax)
        return VD_OK;
    for (int k = 1; k < VD_BAND_OPS; ++k)
        if (net.ops[k].kind != OP_BLOCK || !blocks[net.ops[k].blk].f32 || net.ops[k].x.p != net.ops[k - 1].y.p) return VD_OK;
    const size_t mb = cfg.max_batch;
    const int rows = VD_BAND_OPS + (int)((2 * VD_BAND_OPS + mb - 1) / mb);   // scratch, then the stats
    if (amax_next[0] + rows > kAmaxActs) return VD_OK;
    int rc;
    if ((rc = dalloc((void**)&bands.tag, VD_BAND_OPS * mb * 8))) return rc;
    if ((rc = dalloc((void**)&bands.bmax, VD_BAND_OPS * mb * 4))) return rc;
    VD_CHECK_HIP(hipMemset(bands.tag, 0, VD_BAND_OPS * mb * 8));
    VD_CHECK_HIP(hipMemset(bands.bmax, 0, VD_BAND_OPS * mb * 4));
    bands.scratch = amax_region(0) + (size_t)amax_next[0] * mb;
    amax_next[0] += rows;
    bands.stats = bands.scratch + VD_BAND_OPS * mb;
    for (int k = 0; k < VD_BAND_OPS; ++k) {
        bands.op[k] = k;
        face.net.ops[k].band = k;
    }
    bands.plan = true;
    return VD_OK;
}

bool Ctx::bands_begin(int n, bool plain) {
    bands.active = bands.ran = false;
    if (!bands.plan) return false;
    const FaceBandPlan P = vd_face_band_plan(face.in_h, bands.geom[2], bands.geom[3], bands.geom[4]);
    bool any = false;
    for (int k = 0; k < VD_BAND_OPS; ++k) any |= P.lo[k] > 0 || P.hi[k] < P.tile_rows[k];
    // the pipelined bottleneck forms and whole-batch launches only (vd_common.h BandArgs)
    const bool on = plain && any && tune.face_bands && tune.block32_pipe && tune.block32_pipe_ds && cfg.microbatch <= 0 &&
                    !tune.block32_dbg;
    if (!on || memcmp(bands.geom, bands.last_geom, sizeof bands.geom)) bands.forget();
    if (!on) return false;   // this forward rewrites every tile: no tag survives it (forgotten above)
    memcpy(bands.last_geom, bands.geom, sizeof bands.geom);
    bands.cur = P;
    bands.active = bands.ran = true;
    return true;
}

void Ctx::band_args(int k, int f0, BandArgs* a) const {
    *a = BandArgs{};
    const FaceBandPlan& P = bands.cur;
    if (!bands.active || k < 0 || (P.lo[k] == 0 && P.hi[k] == P.tile_rows[k])) return;
    const size_t mb = cfg.max_batch;
    a->on = 1;
    a->lo = P.lo[k];
    a->hi = P.hi[k];
    a->epoch = bands.epoch;
    a->nchain = k;                                        // op k's tiles depend on the inputs' scales of ops 1..k
    for (int i = 0; i < k; ++i) a->chain[i] = face.net.ops[bands.op[i + 1]].x.amax + f0;
    a->tag = bands.tag + k * mb + f0;
    a->bmax = bands.bmax + k * mb + f0;
    a->scratch = bands.scratch + k * mb + f0;
}

int Ctx::bands_publish(int f0, int n) {
    if (!bands.active) return VD_OK;
    BandPublishArgs p{};
    const size_t mb = cfg.max_batch;
    for (int k = 0; k < VD_BAND_OPS; ++k) {
        band_args(k, f0, &p.op[k]);
        p.tag[k] = bands.tag + k * mb + f0;
        p.bmax[k] = bands.bmax + k * mb + f0;
    }
    p.stats = bands.stats;
    p.n = n;
    hipError_t e = vd_launch_band_publish(p, stream);
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "band publish: %s", hipGetErrorString(e));
    return VD_OK;
}

int Ctx::face_forward(int n, bool plain) {
    const bool with_bands = bands_begin(n, plain);
    int rc = face_forward_run(n);
    bands.active = false;
    if (rc && with_bands) bands.forget();                 // some band tiles may have been left half written
    return rc;
}

int Ctx::face_forward_run(int n) {
    const int mb = cfg.microbatch;                        // frames per micro-batch (0 = off)
    const int stage = cfg.microbatch_stage > 0 ? cfg.microbatch_stage : 2;   // micro-batch through layer<stage>
    const int split = face.net.stage_end[std::min(std::max(stage, 0), 4)];
    const int G = std::min(std::min(tune.face_groups, 4), n);
    if (G >= 2 && mb <= 0 && lane_ev.empty()) {
        // G frame groups on G streams (group 0 on the context stream): each layer's last
        // partial round of workgroups leaves CUs that the other groups' launches take.
        // Every kernel is batch-invariant (a frame's sums do not depend on its batch
        // position or the launch's frame count), so the results are bit-identical to
        // one launch over n frames.
        const Net& net = face.net;
        while ((int)group_streams.size() < G - 1) {
            hipStream_t st;
            hipEvent_t ev;
            VD_CHECK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            VD_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            group_streams.push_back(st);
            group_events.push_back(ev);
        }
        if (!ev_half) VD_CHECK_HIP(hipEventCreateWithFlags(&ev_half, hipEventDisableTiming));
        if (net.amax) VD_CHECK_HIP(hipMemsetAsync(net.amax, 0, net.amax_bytes, stream));
        VD_CHECK_HIP(hipEventRecord(ev_half, stream));
        const int ne = (int)net.ops.size();
        hipStream_t main = stream;
        for (int g = 0; g < G; ++g) {
            const int f0 = (int)((long)n * g / G), f1 = (int)((long)n * (g + 1) / G);
            stream = g ? group_streams[g - 1] : main;
            if (g) VD_CHECK_HIP(hipStreamWaitEvent(stream, ev_half, 0));
            int rc = run_ops(net, 0, ne, f0, f1 - f0);
            if (!rc) rc = bands_publish(f0, f1 - f0);
            if (!rc && g && hipEventRecord(group_events[g - 1], stream) != hipSuccess)
                rc = vd_set_error(VD_ERR_HIP, "group event");
            stream = main;
            if (rc) return rc;
        }
        for (int g = 1; g < G; ++g) VD_CHECK_HIP(hipStreamWaitEvent(stream, group_events[g - 1], 0));
        return VD_OK;
    }
    const int rc = run_net(face.net, n, mb, split);
    return rc ? rc : bands_publish(0, n);
}

int Ctx::face_post(int n, int img_h, int img_w, const BoxTargets& t, const TileGrid* tiles) {
    face_rows_merged = false;
    PostArgs p{};
    p.mode = POST_FACE;
    for (int l = 0; l < 3; ++l) {
        p.heads[l] = (const float*)face.heads[l].p;
        p.lh[l] = face.heads[l].h;
        p.lw[l] = face.heads[l].w;
        p.loff[l] = face.loff[l];
    }
    p.hstride = face.heads[0].c;
    p.anchors = face.anchors; p.A = face.A; p.B = n;
    p.conf = cfg.confidence; p.iou = cfg.nms_iou; p.max_det = 0;
    p.low = rescue_low[0]; p.low_on = rescue_low[0] > 0.f;       // rescue: the keep list at face_low
    p.cand_keys = face.post.keys; p.cand_count = face.post.count;
    p.scratch_box = face.post.box; p.scratch_cls = face.post.cls; p.scratch_nbox = face.post.nbox;
    p.scratch_area = face.post.area; p.scratch_keys = face.post.sort; p.scratch_supp = face.post.supp;
    p.sort_cap = face.post.sort_cap;
    p.img_h = img_h; p.img_w = img_w;
    // retinaface_correct_boxes factors (utils_bbox.py:118-132), float32 tensor arithmetic
    const float inh = (float)face.in_h, inw = (float)face.in_w, ih = (float)img_h, iw = (float)img_w;
    const float rh = inh / ih, rw = inw / iw;
    const float mn = rh < rw ? rh : rw;
    const float nh = ih * mn, nw = iw * mn;
    p.offy = ((inh - nh) / 2.0f) / inh;
    p.offx = ((inw - nw) / 2.0f) / inw;
    p.scy = inh / nh;
    p.scx = inw / nw;
    if (tiles) {   // the same factors for a tile as a frame of its own
        const float th = (float)tiles->th, tw = (float)tiles->tw;
        const float trh = inh / th, trw = inw / tw;
        const float tmn = trh < trw ? trh : trw;
        const float tnh = th * tmn, tnw = tw * tmn;
        p.tile_T = tiles->T; p.tile_h = tiles->th; p.tile_w = tiles->tw;
        p.tile_offy = ((inh - tnh) / 2.0f) / inh;
        p.tile_offx = ((inw - tnw) / 2.0f) / inw;
        p.tile_scy = inh / tnh;
        p.tile_scx = inw / tnw;
    }
    p.cap = t.cap; p.out_count = t.count; p.out_xyxy = t.xyxy; p.out_xyxy_f = t.xyxy_f;
    p.out_score = t.score; p.out_label = t.label;
    vd_post_keep_args(face.post, p, n);
    t_begin(3, (double)n * face.A * 32 * 4);
    hipError_t e = vd_launch_post(p, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "face post: %s", hipGetErrorString(e));
    return VD_OK;
}

// ---- tiled face detection (tiles.hip, pre.hip letterbox_tiles_kernel) ----
int Ctx::tiles_set(int rows, int cols, int overlap_pct) {
    if (rows < 1 || rows > VD_TILES_MAX || cols < 1 || cols > VD_TILES_MAX || overlap_pct < 0 || overlap_pct > 50)
        return vd_set_error(VD_ERR_ARG, "vd_tiles: rows, cols in [1, %d] and overlap_pct in [0, 50] required (got %d, "
                            "%d, %d)", VD_TILES_MAX, rows, cols, overlap_pct);
    if (rows == tile_rows && cols == tile_cols && overlap_pct == tile_overlap) return VD_OK;
    if (rescue_on() && !rescue_tiles)
        return vd_set_error(VD_ERR_STATE, "vd_tiles: tiled detection and rescue (vd_rescue) cannot be combined");
    if (lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_tiles: %d frames are pending in the look-ahead ring (flush first)", lead.pend);
    VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued launch may still read the merged rows
    tile_rows = rows; tile_cols = cols; tile_overlap = overlap_pct;
    tiles_kn = ptiles_kn = 0;
    face_rows_merged = plate_rows_merged = false;
    hold.reset();                                 // the merged rows change capacity: a new stream
    if (rescue_on()) {                            //   ... for the rescue too (vd_rescue_tiles)
        rescue_hs.reset();
        rescue_n = 0;
    }
    return VD_OK;
}

int Ctx::tiles_grid(int h, int w, TileGrid* g) {
    int32_t r[VD_TILE_INPUTS_MAX][4];
    int cnt = 0;
    if (vd_tile_rects_host(h, w, tile_rows, tile_cols, tile_overlap, &r[0][0], &cnt))
        return vd_set_error(VD_ERR_ARG, "tiles: bad frame geometry %dx%d", w, h);
    *g = TileGrid{};
    g->T = cnt; g->tw = r[1][2]; g->th = r[1][3];
    for (int k = 0; k < cnt; ++k) { g->x0[k] = r[k][0]; g->y0[k] = r[k][1]; }
    return VD_OK;
}

int Ctx::face_letterbox_tiles(const uint8_t* dframes, int n, int h, int w, size_t pitch, const TileGrid& g) {
    LetterboxArgs wa, ta;
    face_letterbox_args(dframes, n, h, w, pitch, &wa);
    face_letterbox_args(dframes, n, g.th, g.tw, pitch, &ta);
    const double canvas = (double)wa.oh * wa.ow * wa.cpad * (f32 ? 4 : 2);
    const double bpp = vd_src_bpp(wa.nv);         // a surface call in flight: 1.5 B/px of source (16-bit words: 3)
    t_begin(2, (double)n * (wa.nh * (double)w * bpp + (g.T - 1) * (ta.nh * (double)g.tw * bpp) + g.T * canvas));
    hipError_t e = vd_launch_letterbox_tiles(wa, ta, g, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "tile letterbox: %s", hipGetErrorString(e));
    return VD_OK;
}

// Merged rows and spill scratch for the floor(max_batch / T) frames a call can carry: T * kcap
// boxes per frame, so the bytes do not grow with T (the sort keys alone round up to a power of two).
// plates: the plate lists, class-aware at cfg.plate_iou, in a buffer of their own (both nets' rows
// are live after a vd_process call).
int Ctx::tiles_merge(int n, const TileGrid& g, const int* cnt, const float* xyxy_f, const float* score, const int* label,
                     int icap, const BoxTargets& t, bool plates, bool split, bool low_on, float thr) {
    const int kcap = plates ? plate.post.kcap : face.post.kcap;
    const size_t F = std::max(cfg.max_batch / g.T, 1);
    const size_t mcap = (size_t)g.T * kcap;
    if ((size_t)n > F || icap > kcap || mcap > 0x3fffffffu)
        return vd_set_error(VD_ERR_ARG, "tiles merge: n=%d frames of lists of cap %d outside [1, %zu] x [1, %d]", n, icap,
                            F, kcap);
    size_t sort_cap = 1;
    while (sort_cap < mcap) sort_cap <<= 1;
    const size_t rows = F * mcap;
    const size_t need = rows * (16 + 16 + 16 + 4 + 4 + 4 + 1 + (plates ? 4 : 0)) + F * sort_cap * 8 + 2 * (F * 4 + 16) + 256;
    int rc = plates ? ensure_staging(&ptiles_buf, &ptiles_buf_bytes, need) : ensure_staging(&tiles_buf, &tiles_buf_bytes, need);
    if (rc) return rc;
    TileMergeArgs a{};
    a.n = n; a.g = g; a.A = face.A; a.iou = plates ? cfg.plate_iou : cfg.nms_iou;
    a.cnt = cnt; a.xyxy_f = xyxy_f; a.score = score; a.label = label; a.icap = icap;
    a.plate = plates ? 1 : 0; a.split = split ? 1 : 0;
    char* p = (char*)(plates ? ptiles_buf : tiles_buf);
    a.m_xyxy = (int*)p; p += rows * 16;
    a.m_xyxy_f = (float*)p; p += rows * 16;
    a.s_box = (float4*)p; p += rows * 16;
    a.s_keys = (uint64_t*)p; p += F * sort_cap * 8;
    a.m_score = (float*)p; p += rows * 4;
    a.m_label = (int*)p; p += rows * 4;
    a.s_area = (float*)p; p += rows * 4;
    if (plates) { a.s_cls = (int*)p; p += rows * 4; }
    a.m_count = (int*)p; p += (F * 4 + 15) / 16 * 16;
    a.m_all = (int*)p; p += (F * 4 + 15) / 16 * 16;   // the whole merged counts (low_on)
    a.s_supp = (uint8_t*)p;
    a.low_on = low_on ? 1 : 0; a.thr = thr;
    a.sort_cap = (int)sort_cap; a.mcap = (int)mcap;
    a.cap = t.cap; a.out_count = t.count; a.out_xyxy = t.xyxy; a.out_xyxy_f = t.xyxy_f;
    a.out_score = t.score; a.out_label = t.label;
    t_begin(3, (double)n * g.T * icap * 24);      // the lists' capacity: the counts are known to the device only
    hipError_t e = vd_launch_tiles_merge(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "tiles merge: %s", hipGetErrorString(e));
    if (plates) {
        ptiles_last = a;
        ptiles_kn = n;
        plate_rows_merged = true;
    } else {
        tiles_last = a;
        tiles_kn = n;
        face_rows_merged = true;
    }
    return VD_OK;
}

int Ctx::tiles_nets_set(int nets) {
    if (nets != VD_TILE_FACES && nets != VD_TILE_PLATES && nets != (VD_TILE_FACES | VD_TILE_PLATES))
        return vd_set_error(VD_ERR_ARG, "vd_tiles_nets: nets %d (expected VD_TILE_FACES = 1, VD_TILE_PLATES = 2 or both = 3)",
                            nets);
    if (nets == tile_nets) return VD_OK;
    if (lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_tiles_nets: %d frames are pending in the look-ahead ring (flush first)",
                            lead.pend);
    if (tiles_on()) {
        VD_CHECK_HIP(hipStreamSynchronize(stream));   // a queued launch may still read the merged rows
        tiles_kn = ptiles_kn = 0;
        face_rows_merged = plate_rows_merged = false;
        hold.reset();                                 // the merged rows change capacity: a new stream
        if (rescue_on()) {                            //   ... for the rescue too (vd_rescue_tiles)
            rescue_hs.reset();
            rescue_n = 0;
        }
    }
    tile_nets = nets;
    return VD_OK;
}

int Ctx::tiles_surfaces_set(int on) {
    if (on != 0 && on != 1) return vd_set_error(VD_ERR_ARG, "vd_tiles_surfaces: on %d (expected 0 or 1)", on);
    if (on == tile_surfaces) return VD_OK;
    if (lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_tiles_surfaces: %d frames are pending in the look-ahead ring (flush first)",
                            lead.pend);
    tile_surfaces = on;
    return VD_OK;
}

// The switch alone: no capacity depends on it, so every history stays. Off while both are on would leave a
// combination the setters refuse.
int Ctx::rescue_tiles_set(int on) {
    if (on != 0 && on != 1) return vd_set_error(VD_ERR_ARG, "vd_rescue_tiles: on %d (expected 0 or 1)", on);
    if (on == rescue_tiles) return VD_OK;
    if (lead.pend)
        return vd_set_error(VD_ERR_STATE, "vd_rescue_tiles: %d frames are pending in the look-ahead ring (flush first)",
                            lead.pend);
    if (!on && rescue_on() && tiles_on())
        return vd_set_error(VD_ERR_STATE, "vd_rescue_tiles: rescue (vd_rescue) and tiled detection (vd_tiles) are both on: "
                            "turn one off first");
    rescue_tiles = on;
    return VD_OK;
}

int Ctx::tiles_surfaces_check(const char* who, int flags) const {
    if (tile_surfaces) return VD_OK;
    if (((flags & VD_PROC_FACES) && faces_tiled()) || ((flags & VD_PROC_PLATES) && plates_tiled()))
        return vd_set_error(VD_ERR_STATE, "%s: tiled detection (vd_tiles) reads RGB frames only while vd_tiles_surfaces "
                            "is off", who);
    return VD_OK;
}

int Ctx::tiles_check(int n, int h, int w, TileGrid* g) {
    int rc = tiles_grid(h, w, g);
    if (rc) return rc;
    if ((long long)n * g->T > cfg.max_batch)
        return vd_set_error(VD_ERR_ARG, "tiles: n=%d frames x %d net inputs exceed max_batch=%d (largest n: %d)", n,
                            g->T, cfg.max_batch, cfg.max_batch / g->T);
    return VD_OK;
}

// after face_forward(n * T): the per-input keep lists (face.post, no caller copy), then their merge
int Ctx::face_post_tiled(int n, int h, int w, const TileGrid& g, const BoxTargets& t) {
    int rc = face_post(n * g.T, h, w, BoxTargets{}, &g);
    if (rc) return rc;
    const PostScratch& ps = face.post;
    const bool low = rescue_low[0] > 0.f;         // rescue: the inputs' lists at face_low, whole (kall)
    return tiles_merge(n, g, low ? ps.kall : ps.kcount, ps.kxyxy_f, ps.kscore, ps.klabel, ps.kcap, t, false, false, low,
                       cfg.confidence);
}

// vd_tiles_merge / vd_tiles_merge_plates: the merge step alone on caller lists
int vd_tiles_merge_lists(Ctx* ctx, const char* who, bool plates, const vd_boxes* lists, int n, int fh, int fw, vd_boxes* out,
                         bool low_on, float thr) {
    if (!ctx->tiles_on()) return vd_set_error(VD_ERR_STATE, "%s: tiling is off (vd_tiles)", who);
    if (!(plates ? ctx->plate.loaded : ctx->face.loaded))
        return vd_set_error(VD_ERR_STATE, "%s: %s weights not loaded", who, plates ? "plate" : "RetinaFace");
    if (!lists || !lists->count || !lists->xyxy_f || !lists->score || lists->cap <= 0)
        return vd_set_error(VD_ERR_ARG, "%s: lists need count, xyxy_f, score, cap>0", who);
    if (n <= 0 || fh <= 0 || fw <= 0) return vd_set_error(VD_ERR_ARG, "%s: bad geometry", who);
    TileGrid g;
    int rc = ctx->tiles_check(n, fh, fw, &g);
    if (rc) return rc;
    const int kcap = plates ? ctx->plate.post.kcap : ctx->face.post.kcap;
    if (lists->cap > kcap)
        return vd_set_error(VD_ERR_ARG, "%s: lists of cap %d (at most the net's %d %s)", who, lists->cap, kcap,
                            plates ? "kept boxes per input" : "anchors");
    const int rows = n * g.T;
    const bool host = lists->where == VD_HOST;
    if (host && (rc = vd_count_check(who, lists->count, rows, lists->cap))) return rc;
    BoxTargets t;
    if ((rc = ctx->box_targets(out, n, t))) return rc;
    const int* cnt = lists->count;
    const float* xf = lists->xyxy_f;
    const float* sc = lists->score;
    const int* lab = lists->label;
    if (host) {
        const size_t nb = (size_t)rows * lists->cap;
        const size_t c16 = ((size_t)rows * 4 + 15) / 16 * 16;
        if ((rc = ctx->ensure_staging(&ctx->tiles_in, &ctx->tiles_in_bytes, c16 + nb * 24))) return rc;
        char* p = (char*)ctx->tiles_in;
        int* dc = (int*)p; p += c16;
        float* dx = (float*)p; p += nb * 16;
        float* ds = (float*)p; p += nb * 4;
        int* dl = (int*)p;
        VD_CHECK_HIP(hipMemcpyAsync(dc, lists->count, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
        VD_CHECK_HIP(hipMemcpyAsync(dx, lists->xyxy_f, nb * 16, hipMemcpyHostToDevice, ctx->stream));
        VD_CHECK_HIP(hipMemcpyAsync(ds, lists->score, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        if (lab) VD_CHECK_HIP(hipMemcpyAsync(dl, lists->label, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        cnt = dc; xf = dx; sc = ds; lab = lab ? dl : nullptr;
    }
    if ((rc = ctx->tiles_merge(n, g, cnt, xf, sc, lab, lists->cap, t, plates, false, low_on, thr))) return rc;
    if ((rc = ctx->box_finish(out, n, t))) return rc;
    if (host && !(out && out->where == VD_HOST))
        VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // staging reused by the next call
    return VD_OK;
}


extern "C" {

int vd_tile_rects(int fh, int fw, int rows, int cols, int overlap_pct, int32_t* xywh, int* count) {
    if (vd_tile_rects_host(fh, fw, rows, cols, overlap_pct, xywh, count))
        return vd_set_error(VD_ERR_ARG, "vd_tile_rects: h, w > 0, rows, cols in [1, %d] and overlap_pct in [0, 50] "
                            "required (got %d x %d, %d, %d, %d)", VD_TILES_MAX, fw, fh, rows, cols, overlap_pct);
    return VD_OK;
}

int vd_tiles(vd_ctx* h, int rows, int cols, int overlap_pct) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->tiles_set(rows, cols, overlap_pct);
}

int vd_tiles_surfaces(vd_ctx* h, int on) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->tiles_surfaces_set(on);
}

int vd_rescue_tiles(vd_ctx* h, int on) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->rescue_tiles_set(on);
}

int vd_tiles_merge(vd_ctx* h, const vd_boxes* lists, int n, int fh, int fw, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return vd_tiles_merge_lists(ctx, "vd_tiles_merge", false, lists, n, fh, fw, out);
}

int vd_tiles_merge_plates(vd_ctx* h, const vd_boxes* lists, int n, int fh, int fw, vd_boxes* out) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return vd_tiles_merge_lists(ctx, "vd_tiles_merge_plates", true, lists, n, fh, fw, out);
}

int vd_tiles_nets(vd_ctx* h, int nets) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    return ctx->tiles_nets_set(nets);
}

}  // extern "C"
