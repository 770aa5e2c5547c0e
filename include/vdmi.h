/*
 * vdmi.h — C-ABI of libvdmi.so, the MI355X-native detect-and-blur hot path.
 *
 * This is the drop-in boundary for the per-frame path of the reference
 * (xdu-Liu-learn/Video-desensitization). Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root):
 *
 *   vd_create / vd_load_weights  <- Retinaface.__init__/generate   detect_face/face.py:29-60
 *                                   YOLO(plate_model_path).cuda()   combine_detect.py:872
 *   vd_detect                    <- Retinaface.detect_images        detect_face/face.py:120-150
 *                                   (preprocess :65-88, net :133, postprocess :93-115,
 *                                    scaling :139-146) + int() at combine_detect.py:243
 *   vd_detect_plates             <- plate_detector(batch, verbose=False, conf=0.5)
 *                                                                    combine_detect.py:217
 *   vd_mosaic                    <- mosaic_rectangle_region_single  combine_detect.py:138-161,
 *                                   applied per box in order at     combine_detect.py:246-249
 *   vd_blur                      <- the same loop with cv2.GaussianBlur(region, (k, k), sigma) in
 *                                   place of the resize pair (BASELINE.json names it; the
 *                                   reference has no such function)
 *   vd_process                   <- the per-batch body of batch_process_images
 *                                                                    combine_detect.py:214-251
 *   vd_jpeg_decode / vd_jpeg_info <- cv2.imread(path) + cvtColor(BGR2RGB) of the ffmpeg-split
 *                                   frames                         combine_detect.py:167-172,
 *                                   (frames from convert_video_to_frames :279-476)
 *   vd_hold / vd_hold_reset / vd_hold_motion / vd_read_held: boxes held across frames (cfg.hold_frames; no
 *                                   reference equivalent: the reference treats every frame alone)
 *   vd_lead / vd_process_lead / vd_lead_lists / vd_read_lead / vd_lead_pending: boxes blurred before their
 *                                   first detection (look-ahead hold; no reference equivalent)
 *   vd_rescue / vd_rescue_lists / vd_read_rescue: weak detections that continue a track stay in the blur
 *                                   list (two thresholds; no reference equivalent)
 *   vd_mask / vd_mask_boxes: where the blur lies (a margin around every box, an elliptical mask inside it;
 *                                   no reference equivalent: the reference blurs the detector's rectangle)
 *   vd_cells / vd_smooth / vd_cell_level: blur strength that follows the box size (at most N cells across a
 *                                   box; no reference equivalent: the reference's cell is level px for every box)
 *   vd_process_nv12 / vd_process_lead_nv12 / vd_mosaic_nv12 / vd_nv12_to_rgb: the same path on NV12 video surfaces (vd_nv12: what a
 *                                   decoder hands out and an encoder takes back; no reference equivalent: the
 *                                   reference works on the RGB frames of ffmpeg-split images)
 *   vd_process_yuv420 / vd_mosaic_yuv420 / vd_smooth_yuv420 / vd_yuv420_to_rgb: the same path on 8-bit 4:2:0 frames in
 *                                   any layout (vd_yuv420: I420 / YV12 from a software decoder, NV12, NV21)
 *   vd_process_yuv420_16 / vd_mosaic_yuv420_16 / vd_smooth_yuv420_16 / vd_yuv420_16_to_rgb: ... on 10- and 12-bit
 *                                   4:2:0 frames (vd_yuv420_16: P010, P012, yuv420p10le, yuv420p12le)
 *   vd_read_boxes                <- the complete per-frame box lists the reference's
 *                                   loop iterates (combine_detect.py:241-249), past any cap
 *   vd_sync / vd_last_error / vd_destroy: runtime plumbing (no reference equivalent;
 *                                   errors map to the reference's drop-the-batch
 *                                   behaviour at combine_detect.py:226-228 in the
 *                                   Python wrapper).
 *
 * Conventions: plain pointers and sizes only. Frames are uint8 RGB, HxWx3,
 * row pitch in bytes, frame i at base + i*h*pitch (the *_nv12 entries: NV12
 * surfaces described by a vd_nv12; the *_yuv420 entries: a vd_yuv420). `where` says whether a
 * pointer is host (VD_HOST) or device (VD_DEVICE) memory of the context's GPU.
 * The caller owns frames and box arrays; the library owns weights, device
 * workspace and its stream. No pointer is retained past a call. Calls are
 * asynchronous on the context stream only when every pointer is VD_DEVICE;
 * otherwise they return after results are in the caller's host memory.
 * Return value: VD_OK (0) or a negative VD_ERR_*; vd_last_error() gives a
 * thread-local message. Calls on one context are serialised by a mutex;
 * different contexts are independent (one per device/stream).
 */
#ifndef VDMI_H
#define VDMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDMI_ABI_VERSION 2   /* 2: complete keep lists (count may exceed cap, vd_read_boxes) */

#define VD_OK            0
#define VD_ERR_ARG      -1   /* bad argument / shape */
#define VD_ERR_HIP      -2   /* HIP runtime error */
#define VD_ERR_CAPACITY -3   /* vd_mosaic: a host box list's count exceeds its cap */
#define VD_ERR_WEIGHTS  -4   /* weight blob missing a tensor / wrong shape */
#define VD_ERR_STATE    -5   /* call out of order (e.g. detect before weights) */
#define VD_ERR_NOMEM    -6   /* device allocation failed */

#define VD_HOST   0
#define VD_DEVICE 1

#define VD_PREC_BF16 0       /* bf16 operands, f32 accumulate (performance mode) */
#define VD_PREC_FP32 1       /* f32 operands and activations (parity mode): operands
                              * scaled by powers of two (per frame / per output
                              * channel) and split into fp16 pairs, 3 products on
                              * the f16 matrix cores, f32 accumulate; option
                              * f32_split=1: exact 3-term bf16 split (6 products),
                              * 0: exact-f32 MFMA */
#define VD_PREC_FP16 2       /* fp16 operands, f32 accumulate on                  *
                              * v_mfma_f32_16x16x32_f16; the bf16 plan's fused     *
                              * kernels (stem + pool, layer1 blocks, layer2        *
                              * chains, phased 256x256) templated on the 16-bit type */

#define VD_NET_RETINAFACE 0  /* detect_face/retinaface.py, cfg_re50 */
#define VD_NET_YOLOV8N    1  /* ultralytics YOLOv8n plate detector [ext] */

#define VD_WEIGHTS_VDW1   1  /* "VDW1" named-tensor container, see DESIGN.md */

/* vd_mosaic modes */
#define VD_MOSAIC_OUT_OF_PLACE 0   /* out = in with boxes applied (reference new-array semantics) */

/* vd_cfg.blur_mode: the anonymisation vd_process applies under VD_PROC_MOSAIC */
#define VD_BLUR_PIXELATE 0         /* INTER_NEAREST down/up mosaic (combine_detect.py:138-161), the default */
#define VD_BLUR_GAUSSIAN 1         /* Gaussian blur of each clipped box (vd_blur) */
#define VD_BLUR_KSIZE_MAX 127

#define VD_HOLD_MAX 8              /* largest vd_cfg.hold_frames */

/* vd_process flags */
#define VD_PROC_FACES        1     /* run the RetinaFace branch */
#define VD_PROC_PLATES       2     /* run the YOLOv8n branch (forward + NMS) */
#define VD_PROC_MOSAIC       4     /* write mosaicked frames to `out` */
#define VD_PROC_MOSAIC_PLATES 8    /* "intended mode": mosaic plate boxes too. Without it
                                      plate boxes are discarded like the reference
                                      (combine_detect.py:239 always yields []). */

typedef struct vd_ctx vd_ctx;

typedef struct vd_cfg {
    int32_t input_h, input_w;      /* RetinaFace net input; combine_detect.py:860 uses 640x640 */
    int32_t max_batch;             /* frames per call (config.ini:35 batch_size = 64) */
    int32_t max_frame_h, max_frame_w;
    int32_t precision;             /* VD_PREC_* */
    int32_t max_boxes;             /* per-frame capacity of the NMS output list */
    float   confidence;            /* face score threshold, inclusive (utils_bbox.py:116) */
    double  nms_iou;               /* face NMS IoU (combine_detect.py:862 -> 0.4) */
    int32_t mosaic_level;          /* combine_detect.py:249 -> 8 */
    int32_t plate_imgsz;           /* ultralytics imgsz (640) */
    int32_t plate_nc;              /* plate model classes */
    float   plate_conf;            /* combine_detect.py:217 conf=0.5 */
    double  plate_iou;             /* ultralytics default 0.7 [ext] */
    int32_t plate_max_det;         /* ultralytics default 300 [ext] */
    /* the former reserved[8], offsets unchanged: zero in every field = the behaviour before
     * they were named (no micro-batching, pixelation) */
    int32_t microbatch;            /* frames per depth-first backbone micro-batch (0 = off) */
    int32_t microbatch_stage;      /* micro-batch through layer<stage> (0 -> 2) */
    int32_t blur_mode;             /* VD_BLUR_*: what vd_process's VD_PROC_MOSAIC applies to the boxes */
    int32_t blur_ksize;            /* VD_BLUR_GAUSSIAN: odd kernel size in [3, 127]; 0 -> 31 */
    float   blur_sigma;            /* VD_BLUR_GAUSSIAN: sigma; <= 0 -> 0.3*((k-1)*0.5 - 1) + 0.8 (cv2's rule) */
    int32_t hold_frames;           /* box hold: frames a box stays in the blur list after its last match,
                                    * in [0, VD_HOLD_MAX]; 0 = off (every frame alone, no extra launch) */
    int32_t hold_iou_pct;          /* box hold: match threshold P in [1, 100] (100 * inter >= P * union); 0 -> 30 */
    int32_t reserved[1];
} vd_cfg;

/* Per-frame box lists, caller-allocated. Frame f's boxes live at
 * [f*cap, f*cap + min(count[f], cap)). count[f] is always the COMPLETE keep count
 * and may exceed cap: the arrays then hold the first cap boxes (NMS order), the
 * call still succeeds, vd_read_boxes hands out the complete lists, and the
 * mosaic of vd_process always covers every kept box (the reference blurs every
 * box, combine_detect.py:241-249). A NULL vd_boxes* skips the caller copy. */
typedef struct vd_boxes {
    int32_t  cap;
    int32_t  where;     /* VD_HOST or VD_DEVICE for every array below */
    int32_t* count;     /* [n]            */
    int32_t* xyxy;      /* [n][cap][4]    int() of the source-pixel box (combine_detect.py:243) */
    float*   xyxy_f;    /* [n][cap][4]    float32 source-pixel box before int(); may be NULL */
    float*   score;     /* [n][cap]       may be NULL */
    int32_t* label;     /* [n][cap]       anchor index (faces) / class id (plates); may be NULL */
} vd_boxes;

int         vd_default_cfg(vd_cfg* cfg);
int         vd_abi_version(void);
const char* vd_last_error(void);

int   vd_create(const vd_cfg* cfg, int device, vd_ctx** out);
int   vd_destroy(vd_ctx* ctx);
int   vd_load_weights(vd_ctx* ctx, int net, const void* blob, size_t bytes, int fmt);
int   vd_set_stream(vd_ctx* ctx, void* hip_stream);   /* NULL -> library-owned stream */
/* Kernel-selection switches (A/B measurement, tests that force a kernel form onto
 * small shapes); the defaults are the production plan. Plan switches (block_fuse,
 * chain, stem_pool, ssh_fuse, plate_s2d, f32_split) apply to weights loaded afterwards, the
 * rest to the next launch. Names: conv_stream conv_stream512 conv_dual conv_taps
 * conv_n192 conv_small conv_big conv_big_kmin stream_ntt lb_pair mosaic_map
 * block_fuse chain stem_pool ssh_fuse plate_s2d f32_split x6_small_k x6_small_tiles x6_stream
 * x6_small_k2 x6_bn256 x6_exact x6_stream256 plate_stage jenc_gpu (the full list:
 * runtime.cpp vd_set_option).
 * VD_ERR_ARG for unknown names. */
int   vd_set_option(vd_ctx* ctx, const char* name, int value);
/* Test / profiling only: timing experiments that skip work and give WRONG results
 * while set ("x6_dbg": conv epilogues, "block32_dbg": layer1 block stages). They are
 * not vd_set_option names (that call refuses them). VD_ERR_ARG for unknown names. */
int   vdt_set_debug(vd_ctx* ctx, const char* name, int value);
void* vd_get_stream(vd_ctx* ctx);
int   vd_sync(vd_ctx* ctx);

int vd_detect(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
              int where, vd_boxes* faces);
int vd_detect_plates(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                     int where, vd_boxes* plates);
/* Mosaic of caller box lists; host lists with count[f] > cap are refused
 * (VD_ERR_CAPACITY: boxes the caller does not hold would go unblurred).
 * Out of place only, as the reference blurs a copy (combine_detect.py:142):
 * `out` equal to `in`, or (VD_DEVICE) any overlap of the two n*h*pitch ranges, is
 * VD_ERR_ARG. vd_process with VD_PROC_MOSAIC and VD_DEVICE frames refuses
 * overlapping `in` / `out` the same way (its one-launch output pass gathers cell
 * colours from `in` while other workgroups write `out`); VD_HOST frames are staged
 * in separate device buffers, so host in == out is allowed there. */
int vd_mosaic(vd_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
              int where, const vd_boxes* boxes, int level, int mode);
/* Gaussian blur of caller box lists: the Gaussian counterpart of vd_mosaic, with its
 * staging rules (host frames / host boxes staged, VD_ERR_CAPACITY for a host list with
 * count[f] > cap, VD_ERR_ARG for out == in or overlapping device ranges). Per box, in
 * list order: clip to the frame (combine_detect.py:145-151), replace the clipped region
 * by GaussianBlur(region, (ksize, ksize), sigma) of the region ALONE -- the border is
 * BORDER_REFLECT_101 at the clipped box's edges (any number of reflections: boxes may be
 * narrower than the radius) -- and box j reads the output of box j-1. Fixed point, so the
 * result is defined to the bit (r = ksize / 2):
 *   weights (host, double): w_i = exp(-(i-r)^2 / (2 sigma^2)) / sum; q_i = floor(w_i * 2^20 + 0.5)
 *                           for i != r, q_r = 2^20 - sum of the others (vdt_blur_weights)
 *   horizontal, per channel: t = sum_i q_i * px(y, refl(x+i-r, bw)); h = (t + 2^15) >> 16   (Q8.4)
 *   vertical:                s = sum_i q_i * h(refl(y+i-r, bh), x);  out = (s + 2^23) >> 24
 * which stays within 0.5925 of the real-valued Gaussian (|delta| <= 1 after rounding).
 * ksize odd in [3, VD_BLUR_KSIZE_MAX]; sigma <= 0: 0.3*((ksize-1)*0.5 - 1) + 0.8; a NaN or
 * infinite sigma, an even or out-of-range ksize: VD_ERR_ARG. */
int vd_blur(vd_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
            int where, const vd_boxes* boxes, int ksize, float sigma);
/* With VD_PROC_MOSAIC and cfg.blur_mode == VD_BLUR_GAUSSIAN the boxes are blurred as by
 * vd_blur(cfg.blur_ksize, cfg.blur_sigma) instead of pixelated: the same complete keep
 * lists, faces then plates; detection outputs are the same either way. */
/* With cfg.hold_frames > 0 the blurred list is B_t = D_t ++ H_t (box hold, below). */
int vd_process(vd_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
               int where, int flags, vd_boxes* faces, vd_boxes* plates);
/* Baseline JPEG frames -> RGB frames: the frame read of the reference's loop
 * (cv2.imread + BGR->RGB of the ffmpeg-split frames, combine_detect.py:167-172),
 * libjpeg-turbo's default decode (ISLOW IDCT, fancy upsampling, table YCbCr->RGB),
 * bit-identical. data[i] / sizes[i]: n host JPEG buffers, all h x w with one
 * component layout (1 or 3 components, 1x1 / 2x1 / 2x2 sampling; no progressive /
 * arithmetic coding). Headers parsed and scan segments staged on host threads; the
 * entropy decode runs on the device (chunked speculative Huffman decode with
 * resynchronisation passes; option jdec_gpu=0: host Huffman threads, same pixels),
 * then dequantize + IDCT + upsample + colour in HIP kernels writing `out`
 * (VD_DEVICE: queued on the context stream, the frames feed vd_process directly;
 * VD_HOST: returns when `out` is filled). */
int vd_jpeg_decode(vd_ctx* ctx, const uint8_t* const* data, const size_t* sizes, int n, uint8_t* out,
                   int h, int w, size_t pitch, int where);
int vd_jpeg_info(const uint8_t* data, size_t size, int* h, int* w, int* comps);
/* RGB frames -> baseline JFIF: the frame write of the reference's loop (cv2.imwrite
 * of the processed frames, combine_detect.py:174-180, :259-262; cv2's defaults are
 * quality 95, 4:2:0), libjpeg-turbo's compressor with its defaults bit-identical
 * (Pillow Image.save(..., quality, subsampling) bytes). frames: n frames h x w x 3
 * RGB at `where`; subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0. Colour conversion,
 * downsampling, ISLOW FDCT and quantisation in a HIP kernel; Huffman coding and 0xFF
 * stuffing in HIP kernels (option jenc_gpu=0: on host threads, same bytes); frames
 * up to 2,000,000 scan blocks (8K). Frame i goes to out + i * cap, its length to sizes[i]; VD_ERR_CAPACITY
 * if a frame needs more than cap bytes -- with the device coder sizes[i] then holds an
 * upper bound of frame i's length (re-size and call again), with host threads 0.
 * Returns when every frame is written. */
int vd_jpeg_encode(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch, int where,
                   int quality, int subsampling, uint8_t* out, size_t cap, size_t* sizes);
/* The complete keep lists of the last vd_detect / vd_detect_plates / vd_process
 * call on this context for frames [0, n) of `net` (VD_NET_*), into `out`
 * (min(count, out->cap) boxes per frame; count = complete count). Ordered on the
 * context stream after that call; host targets return when the copy is done. */
int vd_read_boxes(vd_ctx* ctx, int net, int n, vd_boxes* out);

/* ---- box hold: boxes carried across frames ----------------------------------
 * A context created with cfg.hold_frames = K > 0 treats its calls as ONE stream of
 * consecutive frames t = 0, 1, 2, ... (since its last reset) and keeps a box in the blur
 * list for up to K frames after the last frame that matched it, so a face detected in
 * frames t-1 and t+1 and missed in frame t is never shown in the clear. Integers only, so
 * the result is defined to the bit:
 *   D_t      frame t's own boxes as vd_process blurs them: the complete face keep list in
 *            NMS order, then (VD_PROC_MOSAIC_PLATES) the plate keep list;
 *   clip(b)  b clipped to [0, w] x [0, h] as the mosaic clips it (combine_detect.py:145-148);
 *            a box that is empty after clipping never matches and is never held;
 *   match    two non-empty clipped boxes match iff 100 * inter >= P * union, in 64-bit
 *            (union = area_a + area_b - inter; P = cfg.hold_iou_pct; inclusive);
 *   H_t      for a = 1..K (t - a >= 0) and, within each a, in the order of D_{t-a}: box b of
 *            D_{t-a}, unclipped as stored, iff it matches NO box of D_t, .., D_{t-a+1} -- the
 *            most recent sighting of anything not seen since; every candidate is judged on
 *            its own (no greedy chain);
 *   B_t      = D_t ++ H_t, the list frame t is blurred with (vd_process with VD_PROC_MOSAIC).
 * The history -- the D lists of the last K frames, in device memory -- is carried across
 * calls, updated by EVERY vd_process that runs detection in such a context (with or without
 * VD_PROC_MOSAIC: running the K frames before a shard's first frame without it warms the
 * shard up) and by vd_hold; a call of n < K frames shifts it (history = the last K of old
 * history ++ the call's frames). It is cleared by vd_hold_reset and by a call whose (h, w)
 * differs from the previous call's. Detection outputs (faces, plates, vd_read_boxes) are
 * the detections only, exactly as without hold. One extra launch per call (timing family
 * 3); the merged rows hold (K + 1) x (face + plate keep capacity) boxes per frame, so no
 * box is ever dropped (DESIGN.md gives the bytes). hold_frames == 0: no launch, no memory.
 *
 * Motion (vd_hold_motion, VD_HOLD_MOTION_LINEAR; off by default): membership, order and ages
 * of H_t are exactly the above; only the coordinates of a held box change. It is stretched
 * along the displacement the face showed between its last two sightings, so it covers where
 * the face was and where it is heading. For b = D_{t-a}[i] held with age a, c = clip(b):
 *   predecessor  among the boxes p of D_{t-a-1}, the frame before the sighting, with
 *            non-empty clip(p) and match(c, clip(p)) under the same P: the one of greatest
 *            IoU on the clipped boxes, compared exactly (p1 beats p2 iff inter1 * union2 >
 *            inter2 * union1 in 64-bit integers), ties to the lowest list index (faces then
 *            plates, as stored); none if that frame does not exist (before the stream's
 *            start or the last reset) or nothing matches;
 *   velocity v = c - clip(p) and prediction q = c + a * v, per coordinate (q may be inverted);
 *   held     = (min(b.x1, q.x1), min(b.y1, q.y1), max(b.x2, q.x2), max(b.y2, q.y2)): the hull
 *            of the box as stored and its extrapolation, which always contains b; without a
 *            predecessor held = b.
 * With P = 100 a predecessor equals c, so nothing moves. Motion mode needs h, w <= 32768
 * (VD_ERR_ARG otherwise; inter * union <= 2^61 is then exact, and |q| <= 9 * 32768 fits
 * int32) and keeps K + 1 frames of history, so a shard warms up on K + 1 frames.
 *
 * vd_hold: the same step for callers with their own detectors. det: the D lists of n
 * consecutive h x w frames (host or device; a host list with count[f] > cap is refused,
 * VD_ERR_CAPACITY, as by vd_mosaic). out (may be NULL): B_t per frame under the vd_boxes
 * contract (count complete, arrays truncated at cap); label = age (0: the frame's own
 * box, a: held from frame t - a); score and xyxy_f are not written. Same kernel and same
 * history as vd_process. VD_ERR_STATE in a context with hold_frames == 0. */
int vd_hold(vd_ctx* ctx, const vd_boxes* det, int n, int h, int w, vd_boxes* out);
/* Forget the history: the next frame is frame 0 of a new stream (a cut, a new video, a
 * dropped batch). VD_OK and no effect in a context with hold_frames == 0. */
int vd_hold_reset(vd_ctx* ctx);
/* The motion model of held boxes (above): VD_HOLD_MOTION_OFF (the default) or
 * VD_HOLD_MOTION_LINEAR; any other mode is VD_ERR_ARG. A change of mode forgets the history
 * as vd_hold_reset does; setting the mode the context already has changes nothing. In a
 * context with hold_frames == 0: VD_ERR_STATE for LINEAR, VD_OK and no effect for OFF. */
#define VD_HOLD_MOTION_OFF 0
#define VD_HOLD_MOTION_LINEAR 1
int vd_hold_motion(vd_ctx* ctx, int mode);
/* H_t (the held boxes alone, label = age) of frames [0, n) of the last vd_process / vd_hold
 * call, under the vd_boxes contract; ordered on the context stream like vd_read_boxes.
 * VD_ERR_STATE with hold_frames == 0 or before the first holding call. */
int vd_read_held(vd_ctx* ctx, int n, vd_boxes* out);

/* ---- look-ahead hold: a face is blurred before its first detection ----------------
 * The box hold looks backwards only: a person walking towards the camera is first detected in
 * some frame t0, and frames t0-1, t0-2, .. show the face in the clear. A context has a lead
 * setting (J, motion): J in [0, VD_LEAD_MAX], motion VD_HOLD_MOTION_OFF or
 * VD_HOLD_MOTION_LINEAR. J == 0 (the default) is off: no launch, no memory, every byte as
 * before. P is cfg.hold_iou_pct (0 -> 30, whether or not hold_frames is set). For a stream
 * S = D_0 .. D_{T-1} of h x w frames -- T counts the frames between two stream ends; a stream
 * ends at a flush or a reset -- with clip, match and D_t as in the box hold:
 *   A_t      ("lead list") is H_{T-1-t} of the reversed stream D_{T-1} .. D_0 under the hold
 *            definition with K = J and the same P, h, w. Written out: for a = 1..J (t + a < T)
 *            and, within each a, in the order of D_{t+a}: box b of D_{t+a}, unclipped as
 *            stored, iff it is non-empty after clipping and matches NO box of D_t, ..,
 *            D_{t+a-1}; every candidate is judged on its own; a box that is empty after
 *            clipping is never led;
 *   motion   membership, order and ages are the same; only the coordinates change. The
 *            predecessor of c = clip(b) is sought in D_{t+a+1} by the rules of vd_hold_motion
 *            (best exact IoU among the matches, ties to the lowest index, none if that frame
 *            does not exist); the stored box is the hull of b and q = c + a * (c - clip(p)):
 *            it stretches backwards along the way the face came. Needs h, w <= 32768;
 *   delay    = J + (motion ? 1 : 0): frame t can be emitted once D_{t+delay} is known, or the
 *            stream has ended;
 *   B_t      = D_t ++ H_t ++ A_t, the list frame t is blurred with; H_t is the hold list exactly
 *            as above, empty when hold_frames == 0. The order matters (pixelation: box j reads
 *            box j-1; smooth blur: ties to the lower index) and is fixed as written. Mask
 *            growth, cells and the ellipse restore act on B_t as they act on D_t ++ H_t.
 * Detection outputs (faces, plates, vd_read_boxes, vd_read_held) and the hold history are
 * untouched. The result does not depend on how the stream is cut into calls, calls of fewer
 * than `delay` frames and of one frame included.
 *
 * What the library keeps between calls: the last `delay` input frames in a device ring of its
 * own, allocated on first use (no caller pointer is retained past a call), those frames' D
 * lists, and their already merged D ++ H rows (H_t depends only on the past, so it is final
 * when frame t is pushed). One list launch per lead call (lead.hip, timing family 3); the
 * merged rows hold (K + 1 + J) x (face + plate keep capacity) boxes per frame, so no box is
 * ever dropped; the pixel ring is updated by device-to-device copies on the context stream
 * (family 4). DESIGN.md gives the bytes.
 *
 * vd_lead: the setting. Bad J, bad motion, or motion with J == 0: VD_ERR_ARG. A change while
 * frames are pending: VD_ERR_STATE; the setting the context already has changes nothing.
 * vd_hold_motion and vd_tiles that would change state while frames are pending, vd_hold and
 * vd_process while frames are pending: VD_ERR_STATE. vd_process with VD_PROC_MOSAIC in a
 * context with J > 0 is VD_ERR_STATE (it would silently skip A_t); without the flag it stays
 * legal while nothing is pending, which is how a shard warms up. vd_hold_reset is the explicit
 * "abandon": it drops the pending frames unemitted and forgets both histories.
 *
 * vd_process_lead pushes n frames, frames [p, p + n) of the stream: detection and the hold
 * step run exactly as in vd_process, faces / plates are the detections of the PUSHED frames,
 * and the m oldest unemitted frames go to out[0..m), blurred with B_t. m = max(0, pending + n
 * - delay), or pending + n with `flush` (the stream ends); *n_out = m, computed on the host
 * from counts, so an all-device call stays asynchronous. Emitted frames come partly from the
 * ring and partly from `in`; `out` (m frames of h * pitch bytes) must overlap neither `in` nor
 * itself. n == 0 is allowed only with flush; `in` may then be NULL, and h, w, pitch are those
 * of the pending frames. flags must include VD_PROC_MOSAIC (VD_ERR_ARG). Refusals, each checked
 * before any state changes: m > out_cap VD_ERR_CAPACITY; J == 0 VD_ERR_STATE; (h, w, pitch)
 * differing from the pending frames' VD_ERR_STATE (flush first); frames pending from
 * vd_lead_lists or vd_process_lead_nv12 (or its vd_yuv420 / vd_yuv420_16 forms) VD_ERR_STATE; motion with
 * h or w > 32768 VD_ERR_ARG.
 *
 * vd_lead_lists: the same step for callers with their own detectors, lists only, by the same
 * kernel. det: the D lists of n consecutive h x w frames as for vd_hold (a host list with
 * count[f] > cap: VD_ERR_CAPACITY); det may be NULL when n == 0 (flush). out (may be NULL;
 * room for pending + n frames): B_t of the m emitted frames under the vd_boxes contract, label
 * 0 for an own box, +a for a box held from frame t - a, -a for a box led from frame t + a;
 * score and xyxy_f are not written. The hold history advances as by vd_hold. Frames pending
 * from vd_process_lead or vd_process_lead_nv12: VD_ERR_STATE.
 *
 * vd_read_lead: the lists of emitted frames [0, n) of the last lead call under the vd_boxes
 * contract, which 0: A_t alone (labels -a), 1: B_t; ordered on the context stream like
 * vd_read_held. VD_ERR_STATE with J == 0 or when the last lead call emitted nothing. */
#define VD_LEAD_MAX 8
int vd_lead(vd_ctx* ctx, int frames, int motion);
int vd_lead_pending(vd_ctx* ctx, int* frames);
int vd_process_lead(vd_ctx* ctx, const uint8_t* in, int n, int h, int w, size_t pitch, int where, int flags,
                    vd_boxes* faces, vd_boxes* plates, uint8_t* out, int out_cap, int flush, int* n_out);
int vd_lead_lists(vd_ctx* ctx, const vd_boxes* det, int n, int h, int w, int flush, vd_boxes* out, int* n_out);
int vd_read_lead(vd_ctx* ctx, int n, int which, vd_boxes* out);   /* which 0: A_t alone, 1: B_t */

/* ---- weak-detection rescue: a weak box that continues a track stays hidden ----------
 * A face that turns to profile, is half occluded or motion-blurred keeps firing the detector
 * at a score below `confidence` for longer than any hold lasts. A context has a rescue setting
 * (face_low, plate_low, S); face_low == 0 && plate_low == 0 (the default) is off: no launch, no
 * memory, every byte as before. A net whose low is 0 has no weak boxes. S, the span, is in
 * [1, VD_RESCUE_SPAN_MAX]. W = max(1, cfg.hold_frames), P = cfg.hold_iou_pct (0 -> 30); clip and
 * match are exactly the box hold's. Per frame t of the context's stream (a stream ends at
 * vd_hold_reset or at a change of (h, w), like the hold's):
 *   keep list at low: faces: the candidate test is score >= face_low; plates: best > plate_low
 *            (strict, as the plate test is). Everything else in post -- key, sort, NMS, max_det,
 *            emit -- is unchanged. A greedy NMS in descending score order has the prefix property:
 *            this list cut where the score falls below the net's threshold IS the keep list at
 *            that threshold.
 *   D_t      (strong) the prefix of that list that passes the net's own threshold (>= confidence,
 *            > plate_conf): bit-identical to what the context returns with rescue off -- count,
 *            xyxy, xyxy_f, score, label. The caller's faces / plates, vd_read_boxes, totals and
 *            records stay D_t only.
 *   W_t      (weak) the rest of the keep list, in NMS order, per net.
 *   since    since(e) = 0 for e in D_t. For w in W_t with a non-empty c = clip(w): m(w) = the
 *            minimum of since(e) + a over a = 1..W (t - a >= 0) and e in E_{t-a} with
 *            match(c, clip(e)); w is rescued iff such an e exists and m(w) <= S, and then
 *            since(w) = m(w): the frames since the strong sighting the chain goes back to.
 *            Rescued boxes are references themselves, so a face that stays weak stays hidden for
 *            at most S frames after its last strong detection. Faces and plates match each other
 *            as in the hold. A weak box that is empty after clipping is never rescued; an empty
 *            reference never matches.
 *   R_t      the rescued faces in W_t's order, then the rescued plates (plates take part only
 *            under VD_PROC_MOSAIC_PLATES, as for D_t).
 *   E_t      = D_t ++ R_t. Wherever the hold, lead, mask, cells and blur definitions say D_t,
 *            E_t stands: the history the hold keeps, H_t, A_t of vd_process_lead, and the
 *            blurred list B_t = E_t ++ H_t ++ A_t.
 * E_t depends on frames [t - S, t] only: a shard that first runs the S frames before its first
 * frame (plus K, +1 with motion, for the hold) gets the unsharded E_t. The result does not depend
 * on how the stream is cut into calls. One more timed step of family 3 per call (two kernel
 * launches: phase 1 parallel over the frames against the strong boxes and the history, phase 2
 * one workgroup walking the frames against the rescued boxes); the E rows hold face + plate keep
 * capacity boxes per frame, so no box is ever dropped.
 *
 * vd_rescue: the setting. VD_ERR_ARG: a low that is NaN, < 0 or >= that net's threshold
 * (cfg.confidence, cfg.plate_conf), S out of range. VD_ERR_STATE: a change while lead frames are
 * pending; rescue on while tiling is on (and vd_tiles in a rescue context) unless vd_rescue_tiles
 * (below) has been turned on. Each is checked before
 * any state changes. A change forgets the rescue history and the hold history as vd_hold_reset
 * does (which clears the rescue history too); setting the value the context has changes nothing.
 *
 * vd_rescue_lists: the same step for callers with their own detectors, through the same kernels.
 * strong / weak: D_t and W_t of n consecutive h x w frames, one list per frame (host or device;
 * a host list with count > cap: VD_ERR_CAPACITY). out (may be NULL): E_t under the vd_boxes
 * contract with label = since; score and xyxy_f are not written. It advances the rescue history
 * only: the caller hands E to vd_hold. VD_ERR_STATE with rescue off.
 *
 * vd_read_rescue: lists of frames [0, n) of the last vd_process / vd_process_lead call's rescue
 * step, of one net, under the vd_boxes contract. which 0: R_t of that net with label = since and
 * the score; which 1: W_t of that net with label and score as in the keep list (of the net's last
 * call of any kind). VD_ERR_STATE with rescue off, or for which 0 when that net took no part in
 * the last rescue step. */
#define VD_RESCUE_SPAN_MAX 255
int vd_rescue(vd_ctx* ctx, float face_low, float plate_low, int span);
int vd_rescue_lists(vd_ctx* ctx, const vd_boxes* strong, const vd_boxes* weak, int n, int h, int w, vd_boxes* out);
int vd_read_rescue(vd_ctx* ctx, int net, int n, int which, vd_boxes* out);   /* which 0: R_t, 1: W_t */

/* ---- rescue on tiled nets ------------------------------------------------------------
 * Tiling finds the 40-px face of a 4K frame, rescue keeps it hidden while its score sags: with on = 1
 * a context takes both settings. Nothing new is defined. For a tiled net (vd_tiles, vd_tiles_nets)
 * whose low is > 0 the T per-input keep lists are the lists at low (above), and the cross-tile merge
 * runs over the whole of them, unchanged: map, key (~score bits, t * icap + pos), the greedy sweep at
 * nms_iou (plates: per class at plate_iou), emit. The split is exact:
 *   - strong boxes score >= confidence (plates > plate_conf), weak ones below, so in the merged order
 *     every strong box precedes every weak box;
 *   - each per-input list at low has that input's list at the threshold as its prefix (max_det
 *     included), so a strong box has the position, and the key, it has with rescue off;
 *   - whether the sweep keeps a box depends on the boxes before it only.
 * So the merged list at low, cut where the score stops passing the net's threshold, is bit for bit
 * the merged list with rescue off (count, xyxy, xyxy_f, score, label).
 *   D_t      of a tiled net: that strong prefix. The caller's arrays, vd_read_boxes, totals and
 *            records stay D_t.
 *   W_t      the rest of the merged list, in merge order (label t*A + anchor for faces, the class for
 *            plates); vd_read_rescue reads the merged rows for a tiled net.
 *   From there the rescue definition applies unchanged: wherever it says keep list, the merged rows
 *   stand for a tiled net; an untiled net keeps its own (vd_tiles_nets VD_TILE_PLATES: the faces of
 *   the whole-frame net beside the merged plates, and the reverse). E_t = D_t ++ R_t feeds hold,
 *   lead, mask, cells and the blur as it does untiled, on RGB frames and (vd_tiles_surfaces) surfaces.
 * Opt-in, because vd_rescue in a tiling context and vd_tiles in a rescue context were promised a
 * refusal, and at low every one of the T inputs sorts and sweeps several times the candidates: on = 0
 * (the default) keeps both refusals, code and message. on outside {0, 1}: VD_ERR_ARG. Setting the
 * value the context has changes nothing. VD_ERR_STATE while lead frames are pending, and for on = 0
 * while rescue and tiling are both on (turn one off first; nothing changes). Otherwise it sets a flag
 * and keeps every history. With on = 1 a vd_tiles / vd_tiles_nets call that changes the tiling of a
 * rescue context forgets the rescue history with the hold history (the rows change capacity: a new
 * stream); vd_rescue forgets as it always does. Memory: the E rows take n * ecap * 20 B with ecap the
 * sum over the nets of (T or 1) * the keep capacity, n <= max_batch / T; the two history buffers take
 * W * ecap * 20 B each. Nothing is allocated while rescue or the switch is off.
 * vd_tiles_merge / vd_tiles_merge_plates on caller lists never split: their output is in descending
 * score order, so a caller with their own detector merges the lists at their low threshold, cuts at
 * their own threshold and hands both parts to vd_rescue_lists. */
int vd_rescue_tiles(vd_ctx* ctx, int on);

/* ---- mask shaping: grow the blurred boxes by a margin, blur ellipses -------------
 * A context has a mask setting (shape, g). The default (VD_MASK_RECT, 0) blurs the boxes as
 * stored: no extra launch, no extra memory. With any other setting every list L the context is
 * about to blur -- vd_process with VD_PROC_MOSAIC (the complete keep lists, or B_t = D_t ++ H_t
 * under hold), vd_mosaic, vd_blur -- is shaped first. Integers only, so the result is defined
 * to the bit:
 *   grow(b, g)  b = (x1, y1, x2, y2) as stored, unclipped; W = x2 - x1, H = y2 - y1. W <= 0 or
 *            H <= 0: b unchanged (an empty box stays empty). Otherwise gx = (W*g + 199) / 200 and
 *            gy = (H*g + 199) / 200 in 64 bits (floor division of non-negative numbers: the
 *            ceiling of half the growth, so a grown box never covers less than the real-valued
 *            one) and b' = (x1-gx, y1-gy, x2+gx, y2+gy), each coordinate clamped to
 *            [-2^30, 2^30]. g is a percentage in [0, VD_MASK_GROW_MAX]: a side becomes about
 *            (1 + g/100) times as long.
 *   R        L' = grow(L) -- counts and order kept: faces, then plates, then held boxes -- goes
 *            through the rectangular pass of vd_mosaic / vd_blur unchanged (clip, box j reads box
 *            j-1, every output byte written). VD_MASK_RECT: out = R.
 *   ellipse  for a grown box b' with W, H > 0 (64-bit) and a pixel (x, y) of b' clipped to the
 *            frame: inside iff dx*dx*H*H + dy*dy*W*W <= W*W*H*H with dx = 2x + 1 - (x1 + x2),
 *            dy = 2y + 1 - (y1 + y2): the pixel centre against the ellipse inscribed in the
 *            UNCLIPPED grown box. In the clipped box |dx| <= W and |dy| <= H, so for W, H <= 32768
 *            both sides stay at or below 2^61. A box with W > 32768 or H > 32768 counts as inside
 *            everywhere in its clipped rectangle (it covers more, never less).
 *   VD_MASK_ELLIPSE  E_k = the pixels of box k's clipped rectangle inside its ellipse;
 *            out(p) = R(p) if p lies in some E_k, else in(p). A pixel in the corner of one box but
 *            inside another box's ellipse stays hidden; for a single box this is
 *            blur-the-rectangle, composite-by-ellipse.
 * Coverage: with g >= 42 every pixel of the box as stored lies inside the grown box's ellipse
 * (the corner pixel is the worst: ((W-1) / (W+2gx))^2 + ((H-1) / (H+2gy))^2 <= 2 / 1.42^2 < 1), for
 * every box size and wherever the frame clips it -- clipping removes pixels of the box, it moves
 * neither the ellipse nor the pixels left -- so ("ellipse", g >= 42) hides at least what the
 * default hides. At g = 41 corner pixels of larger boxes fall outside.
 * Squares of side <= 3 are wholly inside their ellipse; a 4 x 4 box loses its four corners.
 * Detection outputs, vd_read_boxes, vd_read_held, vd_hold outputs, hold matching and history work
 * on the detections as stored: shaping happens after the hold merge and only on the list being
 * blurred. The VD_ERR_CAPACITY / VD_ERR_ARG rules of the three blurring calls are unchanged.
 * Launches (mask.hip): one grow launch per blurring call (timing family 3; merged rows of the
 * lists' capacity) and, under VD_MASK_ELLIPSE, one restore launch after the rectangular pass
 * (family 1) that copies in -> out the pixels of the clipped boxes outside every ellipse; for
 * host frames it reads the staged input. */
#define VD_MASK_RECT 0
#define VD_MASK_ELLIPSE 1
#define VD_MASK_GROW_MAX 200
/* Unknown shape or grow_pct outside [0, VD_MASK_GROW_MAX]: VD_ERR_ARG (setting unchanged). Takes
 * effect from the next blurring call. */
int vd_mask(vd_ctx* ctx, int shape, int grow_pct);
/* grow() of caller lists by the context's g, under the vd_boxes contract: out->count = in->count
 * (complete counts, as given), out->xyxy = the grown boxes (min(count, in->cap, out->cap) per
 * frame); xyxy_f, score and label are not written. in / out may be host or device, each on its
 * own; a host `in` with count[f] > cap is VD_ERR_CAPACITY. The kernel of the blur path, so a
 * caller can log or draw what was actually hidden. */
int vd_mask_boxes(vd_ctx* ctx, const vd_boxes* in, int n, vd_boxes* out);

/* ---- box-scaled strength: at most N cells across a face -------------------------
 * The strength of the hiding is otherwise a constant number of pixels (a mosaic cell of about
 * `level` px, a Gaussian of blur_ksize taps), so the largest faces are hidden worst. A context has
 * a cells setting N: 0 (the default) is off -- no extra launch, every byte as before -- or N in
 * [VD_CELLS_MIN, VD_CELLS_MAX]. Integers only, so the result is defined to the bit.
 *   L(b)     the cell level of a box b = (x1, y1, x2, y2) of the list being blurred, as stored and
 *            unclipped, after mask growth if any: W = x2 - x1, H = y2 - y1 in 64 bits, `level` the
 *            call's base level (cfg.mosaic_level in vd_process);
 *              L(b) = level                                                  if N == 0, W <= 0 or H <= 0
 *              L(b) = max(level, min(32768, (max(W, H) + N - 1) / N))        otherwise (floor division).
 *            Never below `level`; a box longer than level * N px gets at most N cells along each
 *            side; the level follows the face, not its clipped remainder.
 *   pixelation (vd_mosaic, vd_process under VD_BLUR_PIXELATE): exactly the mosaic above with L(b)
 *            in place of `level` for box b: sw = max(1, bw / L(b)), sh = max(1, bh / L(b)); the
 *            clipping, the resizeNN maps and "box j reads the output of box j-1" are unchanged.
 *   smooth   (vd_smooth, vd_process under VD_BLUR_GAUSSIAN): the scaled smooth blur. For box k with
 *            the non-empty clipped rectangle (cx1, cy1, cx2, cy2), bw = cx2 - cx1, bh = cy2 - cy1,
 *            f = L(k):
 *              cells  cell (i, j) covers columns [cx1 + i*f, min(cx1 + (i+1)*f, cx2)) and rows
 *                     likewise; sw = ceil(bw / f), sh = ceil(bh / f), both at most N;
 *              mean   a(i, j) = (16 * S + n / 2) / n per channel (Q8.4), S the sum of the cell's
 *                     pixels of `in`, n their number;
 *              across for x in [0, bw): u = 2x + 1 - f, i0 = floor(u / 2f) (toward minus infinity),
 *                     r = u - 2f * i0, i0 and i0 + 1 each clamped to [0, sw - 1]:
 *                     t(x, j) = ((2f - r) * a(i0, j) + r * a(i0 + 1, j) + f) / (2f);
 *              down   for y in [0, bh): j0, j1, s the same from v = 2y + 1 - f:
 *                     out = ((2f - s) * t(x, j0) + s * t(x, j1) + 16f) / (32f).
 *            Every box reads `in`. A pixel takes the value of the box with the largest f among the
 *            boxes whose clipped rectangle contains it, ties to the lowest list index (faces before
 *            plates before held boxes); a pixel in no box is out = in: a small weak box over a large
 *            face never re-exposes it at fine scale, and no box waits for another. f = 1 is the
 *            identity and a constant region stays constant. Needs h, w <= 32768 and 1 <= level <=
 *            32768 (VD_ERR_ARG otherwise). The cost does not grow with the strength: every box
 *            pixel is read once and written once.
 * Order: merge lists, hold merge, mask growth, L from the grown boxes, the rectangular pass; the
 * ellipse restore pass runs afterwards, unchanged. Detection outputs, vd_read_boxes, vd_read_held
 * and the hold history are untouched. vd_blur stays the fixed-kernel Gaussian. Launches
 * (smooth.hip): the copy in -> out and the box pass, both timing family 1; no scratch memory. */
#define VD_CELLS_MIN 2
#define VD_CELLS_MAX 64
/* 0 is off; a value outside {0} and [VD_CELLS_MIN, VD_CELLS_MAX]: VD_ERR_ARG (setting unchanged).
 * Takes effect from the next blurring call: vd_process with VD_PROC_MOSAIC in both blur modes,
 * and vd_mosaic. */
int vd_cells(vd_ctx* ctx, int cells);
/* The scaled smooth blur of caller box lists: the counterpart of vd_mosaic and vd_blur, with their
 * staging rules (host frames / host boxes staged, VD_ERR_CAPACITY for a host list with count[f] >
 * cap, VD_ERR_ARG for out == in or overlapping device ranges). cells in [VD_CELLS_MIN,
 * VD_CELLS_MAX]; the context's mask setting applies to it as to the other two. */
int vd_smooth(vd_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
              int where, const vd_boxes* boxes, int level, int cells);
/* L of a W x H box (host only: no context, no GPU): the routine the launch path itself calls.
 * VD_ERR_ARG (negative) for level < 1 or cells outside {0} and [VD_CELLS_MIN, VD_CELLS_MAX]. */
int vd_cell_level(int W, int H, int level, int cells);

/* ---- tiled face detection: small faces in high-resolution frames -----------------
 * Every frame is letterboxed onto the one input_h x input_w canvas (detect_face/face.py:77-78),
 * so a 3840x2160 frame is shrunk 6x and a face 40 px wide reaches the net about 7 px wide, below
 * its smallest anchor. A context has a tiling setting (R, C, O): R rows and C columns in [1, 4], O
 * percent of overlap in [0, 50]. R*C == 1 (the default) is off: no extra launch, no extra memory,
 * every output as before. Otherwise each h x w frame gives T = 1 + R*C net inputs -- input 0 the
 * whole frame, input 1 + r*C + c tile (r, c) -- and all tiles have one size, so one letterbox
 * geometry serves them. Integers, defined to the bit; per axis of length L cut into K tiles
 * (h, R give th and y0; w, C give tw and x0; floor division throughout):
 *   t   = min(L, (L*(100+O) + 100*K - 1) / (100*K))      the tile's extent
 *   o_k = 0 if K == 1, else (k*(L - t)) / (K - 1)         the origin of tile k
 * The first tile starts at 0, the last ends at L, origins never decrease, consecutive tiles leave
 * no gap, and whenever t < L neighbours overlap by at least floor(L*O/(100*K)); on very small
 * frames tiles may coincide (the merge removes the duplicates). 3840x2160 with (2, 2, 20): tiles
 * of 2304x1296 at x 0, 1536 and y 0, 864.
 * vd_detect and vd_process (VD_PROC_FACES) then:
 *   capacity   n*T <= cfg.max_batch, else VD_ERR_ARG (the message names the largest n);
 *   letterbox  one launch fills the n*T canvases, frame f's inputs at rows f*T .. f*T+T-1, canvas
 *              f*T+t bit-identical to the letterbox of a frame holding exactly that rectangle;
 *   net, post  unchanged over n*T inputs: the per-input keep lists are exactly what vd_detect
 *              returns for each rectangle as a frame of its own;
 *   merge      per frame (one launch, timing family 3): box i of input t moves by the tile's
 *              origin, X = x + (float)x0_t and Y = y + (float)y0_t on both corners (one float32
 *              add each, no FMA; input 0 unchanged); the boxes are ordered by descending score
 *              (bit pattern), ties to the lower t, then to the lower position in that input's
 *              list; greedy NMS over that order on the mapped boxes, the rule and the op order of
 *              the per-input NMS (IoU in float32 against cfg.nms_iou as a double, area =
 *              (x2 - x1) * (y2 - y1)); each kept box gives xyxy_f = the mapped box, xyxy = int()
 *              of it, its score, and label = t*A + anchor (A = the net's anchor count, so
 *              whole-frame boxes keep their labels). The merged rows hold T*A boxes per frame:
 *              nothing is ever dropped.
 * No border rule drops tile boxes near a tile edge: a face cut by a tile edge gives a partial box,
 * which the merge suppresses or keeps beside the full one -- for an anonymiser covering more is
 * harmless. The merged lists ARE the face detections of the call: the caller's `faces` (vd_boxes
 * contract), vd_read_boxes(VD_NET_RETINAFACE), D_t of the box hold, and what the blur hides.
 * Which nets the tiling applies to is a second setting (vd_tiles_nets below): faces alone by
 * default, and plates are then detected on the whole frame exactly as in an untiled context. The
 * paired face+plate letterbox is not used while the face net is tiled. */
#define VD_TILES_MAX 4
/* The rectangles (x, y, w, h) of an h x w frame: xywh[0] the frame, xywh[1 + r*cols + c] tile
 * (r, c); *count = 1 + rows*cols (either pointer may be NULL). Host only, no context, no GPU: the
 * routine the launch path itself calls. VD_ERR_ARG outside the ranges above or for h, w <= 0. */
int vd_tile_rects(int h, int w, int rows, int cols, int overlap_pct, int32_t* xywh, int* count);
/* The context's tiling setting. Bad values: VD_ERR_ARG, setting unchanged. Takes effect from the
 * next call; a change forgets the hold history as vd_hold_reset does (the merged rows change
 * capacity); setting the value the context already has changes nothing. In a rescue context:
 * VD_ERR_STATE unless vd_rescue_tiles is on, and then the rescue history is forgotten too. */
int vd_tiles(vd_ctx* ctx, int rows, int cols, int overlap_pct);
/* The merge step alone on caller lists, by the kernel of the detect path. lists: n*T rows, frame
 * f's input t at row f*T+t, boxes relative to their rectangle of an h x w frame; xyxy_f and score
 * are required, label is optional and read as 0, xyxy is not read; host or device; cap at most
 * the net's anchor count. A host list with count > cap: VD_ERR_CAPACITY. out: n rows under the
 * vd_boxes contract (may be NULL: vd_read_boxes hands the rows out). VD_ERR_STATE with tiling off
 * or before the RetinaFace weights are loaded; n*T > cfg.max_batch: VD_ERR_ARG. */
int vd_tiles_merge(vd_ctx* ctx, const vd_boxes* lists, int n, int h, int w, vd_boxes* out);

/* ---- tiled plate detection: small plates in high-resolution frames -----------------
 * The plate net sees a frame shrunk onto its plate_imgsz canvas too: a 3840x2160 frame is scaled by
 * 1/6, and a 440 x 140 mm plate 25 m ahead of a 3840-px-wide, 60-degree camera (about 58 x 19 px in
 * the source) reaches the net about 10 x 3 px, under one cell of the stride-8 head; on a (2, 2, 20)
 * tile it is 16 x 5 px. With a tiling (R, C, O) set by vd_tiles, vd_tiles_nets says which nets are
 * tiled: VD_TILE_FACES (the default: nothing changes by a byte, no launch is added, no memory is
 * allocated), VD_TILE_PLATES or both. A face net that is not tiled runs exactly as in an untiled
 * context. When plates are tiled, every call that runs the plate net (vd_detect_plates, vd_process /
 * vd_process_lead with VD_PROC_PLATES) runs it on the whole frame and on the R x C rectangles of
 * vd_tile_rects (the face tiling's rectangles), moves the tile boxes back to frame coordinates and
 * merges the T = 1 + R*C lists per frame into one. To the bit:
 *   per input  the keep list of input t of frame f is exactly what vd_detect_plates returns for a
 *              standalone frame holding rectangle t of frame f: the ultralytics letterbox of that
 *              rectangle (scale-up included, pad 114, stride-32 auto padding; each tile canvas is
 *              bit-identical to the plate letterbox of a frame holding those pixels), the forward,
 *              the candidate test, the class-offset NMS at cfg.plate_iou, plate_max_det, and
 *              scale_boxes with the rectangle's own gain and pad, clipped to the rectangle. The whole
 *              frame and the tiles can need canvases of different sizes (360x640 with (1, 3, 0):
 *              384x640 against 640x384), so the tile inputs go through a forward of their own
 *              (inputs f*R*C + (t-1)); the result does not depend on how the inputs are batched.
 *   map        box i of input t > 0 becomes X = x + (float)x0_t, Y = y + (float)y0_t on both corners
 *              (one float32 add each, no FMA); input 0 is left as it is;
 *   order      descending score compared as bit patterns, ties to the lower t, then to the lower list
 *              position (the key of the face merge);
 *   NMS        greedy over that order on the mapped boxes: a kept box a suppresses a later box b iff
 *              label(a) == label(b) and IoU(a, b) > cfg.plate_iou, with area = (x2 - x1) * (y2 - y1)
 *              in float32 and the float32 quotient compared against the double. No class offset is
 *              added (7680 is smaller than the frames accepted here, and an offset would cost the
 *              higher classes mantissa bits); for class 0 the arithmetic equals the per-input rule's;
 *   no cap     the merged list has no max_det: the merged rows hold T x the per-input keep capacity,
 *              so nothing is ever dropped, and no border rule drops tile boxes;
 *   emit       xyxy_f = the mapped box, xyxy = int() of it, score, label = the class id.
 * One launch (timing family 3) on the plate stream, before the plate branch joins. The merged list IS
 * the plate detections of the call: the caller's `plates` (vd_boxes contract, unchanged),
 * vd_read_boxes(VD_NET_YOLOV8N), the plate part of D_t for hold, lead and the blur list under
 * VD_PROC_MOSAIC_PLATES. Capacity: a call that runs a tiled net needs n*T <= cfg.max_batch
 * (VD_ERR_ARG, the message names the largest n), whichever net is tiled. Rescue with tiling is
 * refused for any nets value unless vd_rescue_tiles (above) is on, and a 4:2:0 surface call (the *_nv12,
 * *_yuv420 and *_yuv420_16 entries)
 * that would run a tiled net is VD_ERR_STATE unless vd_tiles_surfaces (below) has been turned on. */
#define VD_TILE_FACES 1
#define VD_TILE_PLATES 2
/* Which nets the tiling applies to: nets in {VD_TILE_FACES, VD_TILE_PLATES, VD_TILE_FACES |
 * VD_TILE_PLATES}; anything else is VD_ERR_ARG and the setting stays unchanged. Stored, with no
 * effect, while R*C == 1. VD_ERR_STATE while lead frames are pending. A change while tiling is on
 * forgets the hold history, as vd_tiles does (the merged rows change capacity); setting the value
 * the context already has changes nothing. */
int vd_tiles_nets(vd_ctx* ctx, int nets);
/* The plate merge step alone on caller lists, by the kernel of the detect path: vd_tiles_merge's
 * layout (row f*T+t), staging, capacity and state rules, with cap at most the plate net's per-input
 * keep capacity; `label` is read as the class (NULL: 0). VD_ERR_STATE with tiling off or before the
 * plate weights are loaded. */
int vd_tiles_merge_plates(vd_ctx* ctx, const vd_boxes* lists, int n, int h, int w, vd_boxes* out);

/* ---- tiled detection on 4:2:0 surfaces ----------------------------------------------
 * 4K footage arrives as decoder surfaces, and tiling exists for 4K footage. With on = 1 the surface
 * entries vd_process_nv12, vd_process_yuv420, vd_process_yuv420_16, vd_process_lead_nv12,
 * vd_process_lead_yuv420 and vd_process_lead_yuv420_16 run the tiled nets of the context (vd_tiles,
 * vd_tiles_nets) instead of refusing. Nothing new is computed: net input f*T + t (plates: f*R*C + t - 1)
 * is bit-identical to the RGB tile letterbox of rectangle t of *_to_rgb(frame f), so every list
 * (detected, merged, held, led) equals the RGB tiled call's on the converted frames and every output
 * sample is what the surface pass writes for those lists. The conversion is per pixel with the chroma
 * sample of (y >> 1, x >> 1) of the FRAME, so the tile letterbox reads a tile at origin (y0, x0) with
 * its luma at (y0, x0), its chroma at (y0 >> 1, x0 >> 1) and the origin's parities (y0 & 1, x0 & 1):
 * tile origins and extents are odd in ordinary settings (1920x1080, (3, 3, 15): y0 = 333). 16-bit
 * surfaces: detection sees the 8-bit picture, as untiled. Capacity as for RGB: n*T <= cfg.max_batch
 * (VD_ERR_ARG, the message names the largest n).
 * Opt-in, because a caller of a surface entry in a tiling context was promised a refusal and must
 * not silently get 1 + R*C net passes per frame: on = 0 (the default) keeps the refusal, VD_ERR_STATE
 * with a message that names vd_tiles_surfaces. on outside {0, 1} is VD_ERR_ARG; VD_ERR_STATE while
 * lead frames are pending; setting the value the context already has changes nothing. The hold
 * history is kept (the merged rows' capacities depend on vd_tiles / vd_tiles_nets only). Rescue with
 * tiling is refused unless vd_rescue_tiles is on (then it runs on surfaces as on RGB frames); the fixed
 * 31-tap Gaussian on surfaces, 4:2:2 / 4:4:4 and depth conversion stay refused. */
int vd_tiles_surfaces(vd_ctx* ctx, int on);

/* ---- NV12 frames: detect and blur video surfaces directly -------------------------
 * A video decoder hands out NV12 surfaces and an encoder takes them back: a pitched luma plane
 * followed by an interleaved half-resolution chroma plane. These entries take and write that
 * format; no full-resolution RGB copy of a frame exists in device memory on this path. Integers
 * only, so every result is defined to the bit.
 *   layout   h and w are even. A frame is h luma rows of `pitch` bytes (pitch >= w) and, at
 *            uv_offset >= h*pitch from the frame's first byte, h/2 chroma rows of `pitch` bytes holding
 *            U, V interleaved: U(y,x) = uv[(y>>1)*pitch + (x & ~1)], V the next byte. Frame i lies at
 *            base + i*frame_stride, frame_stride >= uv_offset + (h/2)*pitch. Decoders pad the luma
 *            height (1080 becomes 1088), so uv_offset and frame_stride are explicit. matrix and range
 *            of an output descriptor are ignored.
 *   colour   rgb(y,x) = C(Y(y,x), U(y,x), V(y,x)): chroma is nearest (no chroma interpolation);
 *            int32 arithmetic, >> arithmetic, clip8 clamps to [0, 255]:
 *              t = cy*(Y - yoff) + 128
 *              R = clip8((t + crv*(V-128)) >> 8)
 *              G = clip8((t + cgu*(U-128) + cgv*(V-128)) >> 8)
 *              B = clip8((t + cbu*(U-128)) >> 8)
 *              limited: yoff 16, cy 298      full: yoff 0, cy 256
 *                                 crv   cgu   cgv   cbu
 *              BT.601 limited     409  -100  -208   516
 *              BT.709 limited     459   -55  -136   541
 *              BT.601 full        359   -88  -183   454
 *              BT.709 full        403   -48  -120   475
 *            each coefficient round(256 * real coefficient) for Kr/Kb = 0.299/0.114 and 0.2126/0.0722,
 *            with 255/219 and 255/224 excursions in limited range. One function (csrc/nv12.h) is
 *            compiled into the letterbox kernels and into vd_nv12_to_rgb.
 *   detection  vd_process_nv12 returns exactly what vd_process returns on the RGB frames C(frame) in
 *            the same context with the same flags -- count, xyxy, xyxy_f, score, label of faces and
 *            plates, vd_read_boxes, vd_read_held, vd_read_rescue, the hold and rescue history --
 *            because every canvas it builds is bit-identical to the RGB letterbox of C(frame). An NV12
 *            call is a call of the context's one stream: it advances the same history as an RGB call
 *            of the same (h, w).
 *   pixelation  the list being blurred is what vd_process would blur (the complete keep lists, faces
 *            then plates; E_t ++ H_t under rescue and hold; after mask growth; L(b) from vd_cell_level
 *            under cells). For box b with luma clip c = clip(b) to [0,w] x [0,h]: an empty c touches
 *            neither plane; luma is the mosaic above on the Y plane as an h x w one-channel image with
 *            box c and level L(b); chroma is the same mosaic on the UV plane as an (h/2) x (w/2)
 *            two-channel image with box cc = (c.x1>>1, c.y1>>1, (c.x2+1)>>1, (c.y2+1)>>1) and level
 *            Lc = (L(b)+1)>>1. Every chroma sample that colours a hidden luma pixel is hidden, and a
 *            chroma cell never spans fewer luma pixels than a luma cell. Per plane box j reads the
 *            output of box j-1. Every output byte of both planes inside [0,w) of each row is written
 *            exactly once; pad bytes beyond w and rows between the planes are not written.
 *   smooth   (VD_PROC_MOSAIC / vd_mosaic_nv12 in a VD_BLUR_GAUSSIAN context with vd_cells on, and
 *            vd_smooth_nv12) the scaled smooth blur of vd_cells, plane by plane, on the same list with
 *            the same c, cc and L(b). Luma: the blur on the Y plane as an h x w one-channel image with
 *            rectangle c and f = L(b). Chroma: the blur on the UV plane as an (h/2) x (w/2)
 *            two-channel image with rectangle cc and fc = (L(b)+1)>>1, U and V each treated as the RGB
 *            path treats a channel. Cells, Q8.4 means, across, down and the rounding terms are exactly
 *            vd_cells' formulas; every box reads `in`. Owner: per plane, the owner of a sample is the
 *            box with the largest L(b) -- the luma level in both planes, so ownership is the same in
 *            both (L = 7 and L = 8 share fc = 4) -- among the boxes whose rectangle of that plane (c
 *            or cc) holds the sample, ties to the lowest list index; a sample in no rectangle is
 *            out = in. Every byte inside [0,w) of both planes' rows is written exactly once; pad
 *            bytes and the rows between the planes are never written. Chroma grid bound: a luma grid
 *            has at most N = cells cells per side, a chroma grid at most N + 1, since cw <= bw/2 + 1
 *            <= N*L/2 + 1 <= N*fc + 1; the bound is reached (N = 2, level 1, box (1, 0, 5, 4): L = 2,
 *            fc = 1, cc = (0, 0, 3, 2), 3 cells across). Needs h, w <= 32768 and 1 <= level <= 32768
 *            (VD_ERR_ARG otherwise). Launches (smooth.hip): one copy of both planes and one box pass
 *            of both planes, family 1, no scratch memory.
 *   ellipse  (a VD_MASK_ELLIPSE context, over pixelation and the smooth blur alike) R is the
 *            rectangular NV12 pass above on the grown list, E_k the luma pixels of box k's clipped
 *            rectangle inside its ellipse by the unchanged predicate of vd_mask. Luma: out_Y(p) =
 *            R_Y(p) if p lies in some E_k, else in_Y(p). Chroma: sample (cy, cx) is hidden iff at
 *            least one of its four luma pixels (2cy + {0,1}, 2cx + {0,1}) lies in some E_k; out_UV =
 *            R_UV where hidden, else in_UV. So a hidden luma pixel has both its Y and its UV from R,
 *            for a pixel that is not hidden and whose chroma sample is not hidden C(out) = C(in)
 *            exactly, and the g >= 42 coverage guarantee carries over unchanged. In span form the
 *            hidden samples of chroma row cy for box k are the union of [xl >> 1, (xr + 1) >> 1) over
 *            the non-empty spans [xl, xr) of E_k in luma rows 2cy and 2cy + 1. One restore launch
 *            after the rectangular pass (mask.hip, family 1, work 0).
 * Order, as for RGB frames: hold merge, rescue, mask growth, L from the grown boxes, the rectangular
 * pass, the restore.
 * VD_ERR_ARG, each checked before any state changes: odd or non-positive h or w; pitch < w;
 * uv_offset < h*pitch; frame_stride too small; unknown matrix or range; device in / out ranges that
 * overlap (whole n*frame_stride ranges); the smooth blur's limits above. Limits of this version
 * (VD_ERR_STATE, the message names the setting): VD_PROC_MOSAIC / vd_mosaic_nv12 in a
 * VD_BLUR_GAUSSIAN context with cells off (the fixed 31-tap Gaussian has no NV12 pass: set cells);
 * any NV12 detection call with tiling on. The look-ahead hold has its own NV12 entry point,
 * vd_process_lead_nv12 below (vd_process_nv12 obeys vd_process's rules in a lead context). Pixelation is one output launch per
 * call for both planes (nv12.hip, timing family 1, work 2 * 1.5 * h * w per frame); the NV12
 * letterbox is family 2. */
#define VD_NV12_BT601 0
#define VD_NV12_BT709 1
#define VD_NV12_LIMITED 0
#define VD_NV12_FULL 1
typedef struct vd_nv12 {
    uint8_t* base; size_t pitch, uv_offset, frame_stride;
    int32_t matrix;   /* VD_NV12_BT601 | VD_NV12_BT709 */
    int32_t range;    /* VD_NV12_LIMITED | VD_NV12_FULL */
} vd_nv12;
/* vd_process on NV12 frames: flags and box contracts are vd_process's; `out` may be NULL without
 * VD_PROC_MOSAIC. Host frames are staged as NV12 (1.5 B/px). */
int vd_process_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, int where, int flags,
                    vd_boxes* faces, vd_boxes* plates);
/* vd_mosaic on NV12 frames: caller lists, with vd_mosaic's staging and capacity rules; the context's
 * mask setting and cells apply as they do to vd_mosaic. The context's blur mode chooses the pass as
 * it does for vd_process_nv12: pixelation, or in a VD_BLUR_GAUSSIAN context with cells on the
 * scaled smooth blur at `level` (cells off: VD_ERR_STATE). */
int vd_mosaic_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, int where,
                   const vd_boxes* boxes, int level);
/* vd_smooth on NV12 frames: the scaled smooth blur of both planes with caller lists in any context,
 * with vd_mosaic_nv12's staging, capacity and overlap rules; cells in [VD_CELLS_MIN, VD_CELLS_MAX],
 * h, w <= 32768 and 1 <= level <= 32768 (VD_ERR_ARG otherwise); the context's mask setting applies. */
int vd_smooth_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, int where,
                   const vd_boxes* boxes, int level, int cells);
/* vd_process_lead on NV12 frames: the look-ahead hold (vd_lead with J > 0) on video surfaces. The n
 * surfaces of `in` are pushed and the m oldest unemitted ones are written, blurred, to the first m of
 * the out_cap surfaces `out` describes (emitted frame i at out->base + i * out->frame_stride; `out` may
 * be NULL when nothing is emitted). Nothing new is defined: with C the conversion above,
 *   lists   faces / plates of the pushed frames, the hold history, m, *n_out and vd_read_lead of the
 *           emitted frames are exactly vd_process_lead's on the RGB stream C(frame) in a context
 *           with the same settings;
 *   pixels  emitted surface t is exactly what vd_mosaic_nv12 writes for input surface t and the list
 *           B_t = D_t ++ H_t ++ A_t under the context's settings (pixelation, or in a VD_BLUR_GAUSSIAN
 *           context with cells on the scaled smooth blur; mask growth, the ellipse restore and cells
 *           act on B_t as in vd_process_nv12). Bytes of `out` outside [0, w) of the two planes' rows
 *           are not written.
 * Neither depends on how the stream is cut into calls (calls of one frame and of fewer than `delay`
 * frames included), on `where`, or on the surface layout of any call: the pending surfaces live in a
 * ring of the library's own, packed (pitch w, chroma at h * w, 1.5 * h * w bytes per frame, `delay`
 * slots: half the RGB ring), so pitch, uv_offset and frame_stride may differ from call to call, as
 * decoders hand out surfaces from pools; matrix and range may differ too (they enter the detection
 * of the pushed frames only). h and w must equal the pending frames'. Delay, flush and n == 0 follow
 * vd_process_lead: with n == 0 `in` may be NULL and flush is required; the end of an empty stream is
 * VD_OK with *n_out = 0. Per call one launch packs the kept surfaces into the ring (nv12.hip, timing
 * family 4, work = bytes read + written); the slots that stay move down by device-to-device copies.
 * Refusals, each checked before any state changes (a VD_ERR_STATE message names the setting): a bad
 * descriptor or odd h or w VD_ERR_ARG; J == 0 VD_ERR_STATE; flags without VD_PROC_MOSAIC, or with
 * neither VD_PROC_FACES nor VD_PROC_MOSAIC_PLATES, VD_ERR_ARG; m > out_cap VD_ERR_CAPACITY; m > 0 with
 * `out` NULL VD_ERR_ARG; device in / out ranges (n * frame_stride, m * frame_stride) that overlap
 * VD_ERR_ARG; a VD_BLUR_GAUSSIAN context with cells off VD_ERR_STATE; a call that would run a tiled net
 * while vd_tiles_surfaces is off VD_ERR_STATE; h or w differing from the pending frames' VD_ERR_STATE (flush first); frames pending
 * from vd_process_lead or vd_lead_lists VD_ERR_STATE, as are those two calls while NV12 frames are
 * pending; motion with h or w > 32768 VD_ERR_ARG. Everything vd_lead lists as refused while frames are
 * pending is refused for pending NV12 frames too, and vd_hold_reset abandons them. */
int vd_process_lead_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, int where, int flags,
                         vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);
/* C(frame) of n frames into packed RGB rows of rgb_pitch >= 3*w bytes, frame i at rgb + i*h*rgb_pitch
 * (host only: no context, no GPU): the routine the kernels' conversion function is compiled from. */
int vd_nv12_to_rgb(const vd_nv12* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch);

/* ---- 8-bit 4:2:0 frames in any layout: I420, YV12, NV12, NV21 ----------------------
 * A software decoder hands out planar 4:2:0 (yuv420p: a luma plane, a U plane and a V plane of
 * (h/2) x (w/2) bytes each), a hardware decoder NV12. All that differs between the 8-bit 4:2:0
 * layouts is where chroma sample (cy, cx) of U and of V lives, so one descriptor covers them:
 *   layout   h and w are even. A frame is h luma rows of `pitch` bytes (pitch >= w) at the frame's
 *            first byte, and
 *              U(cy, cx) = frame[u_offset + cy*chroma_pitch + cx*chroma_step]
 *              V(cy, cx) = frame[v_offset + cy*chroma_pitch + cx*chroma_step]
 *            for cy in [0, h/2), cx in [0, w/2). chroma_step 1: two planes of h/2 rows of w/2 bytes
 *            (I420: U first; YV12: V first). chroma_step 2: one plane of h/2 rows of w bytes of
 *            interleaved pairs, |u_offset - v_offset| = 1 (NV12: v_offset = u_offset + 1; NV21:
 *            u_offset = v_offset + 1). chroma_pitch >= (w/2)*chroma_step. Frame i lies at base +
 *            i*frame_stride. The luma plane is bytes [0, (h-1)*pitch + w) of a frame, a chroma plane
 *            [offset, offset + (h/2-1)*chroma_pitch + (w/2)*chroma_step) (interleaved: one plane from
 *            min(u_offset, v_offset), w bytes a row); the planes of a frame must not overlap and,
 *            when n > 1, must end within frame_stride. matrix and range of an output descriptor
 *            are ignored.
 *   N(S)     for a surface S, N(S) is the NV12 surface with the same Y, U and V samples.
 *   results  nothing new is defined. Every list a *_yuv420 call returns or stores (detections,
 *            vd_read_boxes, vd_read_held, vd_read_rescue, grown lists, the hold and rescue history)
 *            is exactly what the *_nv12 call returns on N(in); for the output O, N(O) equals the
 *            *_nv12 call's output on every sample of the picture. `in` and `out` are independent
 *            descriptors and their layouts may differ (I420 in, NV12 out; NV12 in, YV12 out): a
 *            blurring call thereby also converts between a decoder's and an encoder's layout.
 *            Bytes outside [0, w) of luma rows and outside [0, (w/2)*chroma_step) of chroma rows,
 *            and everything between planes and surfaces, are never written, and nothing outside
 *            those ranges is read for a result. A descriptor with chroma_step 2 and v_offset =
 *            u_offset + 1 and chroma_pitch = pitch gives byte for byte what the *_nv12 entry gives
 *            (it runs the same kernels). A *_yuv420 call is a call of the context's one stream, as
 *            an NV12 or RGB call of the same (h, w) is.
 * Flags, box contracts, staging and capacity rules of vd_process_yuv420 / vd_mosaic_yuv420 /
 * vd_smooth_yuv420 are those of vd_process_nv12 / vd_mosaic_nv12 / vd_smooth_nv12. Host frames are
 * staged in their own layout, packed, at 1.5 B/px.
 * VD_ERR_ARG, each checked before any state changes, the message naming the field: a NULL
 * descriptor or base; odd or non-positive h or w; pitch < w; chroma_step outside {1, 2};
 * chroma_pitch < (w/2)*chroma_step; chroma_step 2 with |u_offset - v_offset| != 1; planes that
 * overlap each other or the luma plane (u_offset / v_offset); a plane that reaches past
 * frame_stride when n > 1; unknown matrix or range (detection and conversion); device `out`
 * overlapping device `in` (the whole extents of the n frames). VD_ERR_STATE, with the messages of
 * vd_process_nv12: a VD_BLUR_GAUSSIAN context with cells off; a call that would run a tiled net while
 * vd_tiles_surfaces is off;
 * VD_PROC_MOSAIC in a look-ahead context (the look-ahead call is vd_process_lead_yuv420, below). Not in
 * this version: rescue with tiling and the fixed Gaussian on surfaces (refused: the first unless
 * vd_rescue_tiles is on, the second always), 4:2:2 and 4:4:4. 10- and 12-bit surfaces (P010, yuv420p10le) have a descriptor of their own: vd_yuv420_16, below. */
typedef struct vd_yuv420 {
    uint8_t* base;        /* first luma byte of frame 0 */
    size_t   pitch;       /* luma row pitch, bytes */
    size_t   u_offset;    /* from a frame's first luma byte to its first U sample */
    size_t   v_offset;    /* ... to its first V sample */
    size_t   chroma_pitch;/* pitch of a chroma row, bytes (planar: often pitch/2; interleaved: pitch) */
    size_t   frame_stride;
    int32_t  chroma_step; /* 1: planar (U and V planes of h/2 x w/2 bytes); 2: interleaved pairs */
    int32_t  matrix, range;   /* VD_NV12_BT601|BT709, VD_NV12_LIMITED|FULL */
} vd_yuv420;
int vd_process_yuv420(vd_ctx* ctx, const vd_yuv420* in, const vd_yuv420* out, int n, int h, int w, int where, int flags,
                      vd_boxes* faces, vd_boxes* plates);
int vd_mosaic_yuv420(vd_ctx* ctx, const vd_yuv420* in, const vd_yuv420* out, int n, int h, int w, int where,
                     const vd_boxes* boxes, int level);
int vd_smooth_yuv420(vd_ctx* ctx, const vd_yuv420* in, const vd_yuv420* out, int n, int h, int w, int where,
                     const vd_boxes* boxes, int level, int cells);
/* vd_process_lead_nv12 on 8-bit 4:2:0 surfaces in any layout. Nothing new is defined: lists (faces / plates
 * of the pushed frames), the hold history, m, *n_out and vd_read_lead are exactly vd_process_lead_nv12's on
 * N(in), and for each emitted surface O, N(O) equals that call's output on every sample of the picture.
 * `in` and `out` are independent descriptors and may differ in layout (I420 in, NV12 out costs no extra
 * pass); either may change from call to call, h and w may not. Pad bytes, and bytes between the planes and
 * surfaces of `out`, are never written. The pending surfaces live in vd_process_lead_nv12's ring -- packed
 * NV12, whatever the callers' layouts -- under the same pending mode, so one stream may be pushed by
 * vd_process_lead_nv12 and vd_process_lead_yuv420 in turn; per call one launch packs the kept surfaces
 * from the input's layout into the ring (nv12.hip; timing family 4, work = bytes read + written). A
 * descriptor that is NV12 gives byte for byte what vd_process_lead_nv12 gives, by the same kernels.
 * Delay, flush, n == 0 (`in` may be NULL; h and w those of the pending surfaces) and the end of an empty
 * stream (VD_OK, *n_out = 0) follow vd_process_lead_nv12. Refusals are vd_process_lead_nv12's with
 * vd_process_yuv420's descriptor rules, each checked before any state changes and with *n_out untouched:
 * a bad descriptor VD_ERR_ARG (the message names the field); J == 0 VD_ERR_STATE; flags without
 * VD_PROC_MOSAIC, or with neither VD_PROC_FACES nor VD_PROC_MOSAIC_PLATES, VD_ERR_ARG; m > out_cap
 * VD_ERR_CAPACITY; m > 0 with `out` NULL VD_ERR_ARG; device extents of `in` and `out` that overlap
 * VD_ERR_ARG; a VD_BLUR_GAUSSIAN context with cells off VD_ERR_STATE; a call that would run a tiled net
 * while vd_tiles_surfaces is off VD_ERR_STATE; h or w differing from the pending surfaces' VD_ERR_STATE (flush first); frames pending
 * from vd_process_lead, vd_lead_lists or vd_process_lead_yuv420_16 VD_ERR_STATE, as are those calls while
 * these surfaces are pending; motion with h or w > 32768 VD_ERR_ARG. vd_hold_reset abandons pending
 * surfaces, and everything vd_lead refuses while frames are pending stays refused. */
int vd_process_lead_yuv420(vd_ctx* ctx, const vd_yuv420* in, const vd_yuv420* out, int n, int h, int w, int where, int flags,
                           vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);
/* vd_nv12_to_rgb for any layout: C(frame) of n frames (host only: no context, no GPU), by the same function. */
int vd_yuv420_to_rgb(const vd_yuv420* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch);

/* ---- 10- and 12-bit 4:2:0 frames: P010, P012, yuv420p10le, yuv420p12le --------------
 * Main10 HEVC leaves a hardware decoder as P010 and a software decoder as yuv420p10le. Such a
 * surface goes in as it is: detection sees an 8-bit picture the library already defines, the blur
 * acts on the 16-bit samples, and every sample outside a hidden box comes back bit for bit.
 *   layout   vd_yuv420's fields, all offsets and pitches in BYTES, followed by depth and shift. A
 *            sample is a little-endian uint16_t. chroma_step counts samples (1 planar, 2
 *            interleaved pairs): a luma row holds w words (pitch >= 2*w), a chroma row
 *            (w/2)*chroma_step words (chroma_pitch >= w*chroma_step), and
 *              U(cy, cx) = word at frame + u_offset + cy*chroma_pitch + 2*cx*chroma_step
 *            (V likewise). pitch, chroma_pitch, u_offset, v_offset and frame_stride are even and
 *            base is 2-byte aligned. chroma_step 2: |u_offset - v_offset| = 2. depth is 10 or 12,
 *            0 <= shift <= 16 - depth, and the value of a word is
 *              v = (word >> shift) & ((1 << depth) - 1).
 *            yuv420p10le / yuv420p12le: shift 0, step 1. P010: depth 10, shift 6, step 2, V after
 *            U. P012: depth 12, shift 4. The V-first variants of all of these by the offsets. The
 *            plane-overlap and frame_stride rules are vd_yuv420's on the byte extents (a luma row
 *            is 2*w bytes, a chroma row w*chroma_step).
 *   D(S)     the 8-bit surface with S's layout (pitches and offsets counted in samples) whose
 *            samples are v >> (depth - 8). lo(S) / hi(S): the 8-bit surfaces of the low / high bytes
 *            of S's words.
 *   lists    nothing new is computed for detection: every list a *_yuv420_16 call returns or stores
 *            (detections, vd_read_boxes, vd_read_held, vd_read_rescue, grown lists, the hold and
 *            rescue history) is exactly what the *_yuv420 call gives on D(in).
 *   pixelation  a pure copy of words: the output's low bytes are what vd_mosaic_yuv420 writes for
 *            lo(in) with the same list, level and cells, its high bytes likewise for hi(in); unused
 *            bits travel with their word.
 *   smooth   the formulas of vd_cells, plane by plane as vd_smooth_nv12 defines them (owner by luma
 *            level, chroma box cc, chroma grid of at most N + 1 cells), on the values v: means are
 *            Q(depth).4, (16*S + n/2) / n; t, T and the result follow the same expressions. At depth
 *            12 t <= 65520 and T + 16f <= 65536*65520 + 16*32768 < 2^32, which is why depth 16 is not
 *            offered. A blurred sample is written as result << shift with its unused bits zero; a
 *            sample owned by no box is out word = in word.
 *   ellipse  the predicate and the chroma rule of vd_mask on NV12 frames (a chroma sample is hidden
 *            iff one of its four luma pixels is); the restore copies words.
 *   in/out   `in` and `out` may differ in layout, pitches and offsets; depth and shift of `out` must
 *            equal `in`'s (VD_ERR_ARG: no depth conversion). matrix and range of an output
 *            descriptor are ignored. Pad bytes, and bytes between planes and surfaces, are never
 *            written.
 * Flags, box contracts, capacity and overlap rules are those of the *_yuv420 calls; host frames are
 * staged in their own layout, packed, at 3 B/px. VD_ERR_ARG, before any state changes, the message
 * naming the field: every rule of vd_yuv420 on the byte extents; an odd pitch, chroma_pitch,
 * u_offset, v_offset or frame_stride or a base that is not 2-byte aligned; pitch < 2*w; depth
 * outside {10, 12}; shift outside [0, 16 - depth]; chroma_step 2 with |u_offset - v_offset| != 2.
 * VD_ERR_STATE with the messages of vd_process_yuv420: a VD_BLUR_GAUSSIAN context with cells off; a
 * call that would run a tiled net while vd_tiles_surfaces is off; VD_PROC_MOSAIC in a look-ahead
 * context (the look-ahead call is vd_process_lead_yuv420_16, below). Not in this version: rescue with
 * tiling and the fixed Gaussian on surfaces (refused: the first unless vd_rescue_tiles is on, the second
 * always), depth or shift conversion between in and out, 16-bit-deep samples, 4:2:2 and 4:4:4. */
typedef struct vd_yuv420_16 {
    uint8_t* base;        /* first luma word of frame 0 (2-byte aligned) */
    size_t   pitch;       /* luma row pitch, bytes (even, >= 2*w) */
    size_t   u_offset;    /* bytes from a frame's first luma word to its first U word */
    size_t   v_offset;    /* ... to its first V word */
    size_t   chroma_pitch;/* pitch of a chroma row, bytes (even) */
    size_t   frame_stride;/* bytes (even) */
    int32_t  chroma_step; /* in samples: 1 planar, 2 interleaved pairs */
    int32_t  matrix, range;   /* VD_NV12_BT601|BT709, VD_NV12_LIMITED|FULL */
    int32_t  depth;       /* 10 or 12 */
    int32_t  shift;       /* position of the sample in the word, 0 .. 16 - depth */
} vd_yuv420_16;
int vd_process_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int h, int w, int where,
                         int flags, vd_boxes* faces, vd_boxes* plates);
int vd_mosaic_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int h, int w, int where,
                        const vd_boxes* boxes, int level);
int vd_smooth_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int h, int w, int where,
                        const vd_boxes* boxes, int level, int cells);
/* vd_process_lead_yuv420 on surfaces of 16-bit words. Lists are exactly vd_process_lead_yuv420's on D(in);
 * emitted surface t is exactly what vd_mosaic_yuv420_16 (or, as the context's settings ask, the smooth blur
 * and the ellipse restore above) writes for input surface t over B_t = D_t ++ H_t ++ A_t, and every word
 * that no box owns comes back bit for bit, unused bits included. The pending surfaces live in a second
 * form of the pixel ring: packed whole words, interleaved chroma with U first, luma pitch 2*w bytes, chroma
 * at 2*h*w, 3*h*w bytes a slot (the size of the RGB ring's slot), under a pending mode of its own. depth
 * and shift belong to the pending geometry: `out` must have `in`'s (VD_ERR_ARG, as above); a push whose
 * depth or shift differs from the pending surfaces' is VD_ERR_STATE (flush first), as for h and w; a
 * flush alone (n == 0) takes them from `out`, and they must equal the pending ones. Everything else --
 * layouts that change from call to call, delay, flush, the refusals, vd_hold_reset -- is
 * vd_process_lead_yuv420's with vd_process_yuv420_16's descriptor rules; 8-bit surfaces pending refuse
 * this call and the reverse (VD_ERR_STATE). */
int vd_process_lead_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int h, int w, int where,
                              int flags, vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);
/* C(D(frame)) of n frames (host only: no context, no GPU), by the same conversion function. */
int vd_yuv420_16_to_rgb(const vd_yuv420_16* in, int n, int h, int w, uint8_t* rgb, size_t rgb_pitch);

/* ---- instrumentation (bench / profiling) ---------------------------------- */
/* When enabled, every launch of kernel family `fam` is bracketed by HIP events
 * on the context stream; vd_timing_read returns the summed duration (ms), the
 * launch count and the summed algorithmic work (FLOP or bytes) since the last
 * reset. Families: 0 = RetinaFace conv (implicit GEMM / streaming 1x1), 1 = mosaic
 * output pass (or the Gaussian blur's launches, or the smooth blur's copy and box pass; the mask's restore pass, work 0: its bytes follow
 * from the boxes; the NV12 output pass or the NV12 smooth blur's copy, work 2 * 1.5 * h * w per frame, its box pass and the NV12 restore, work 0), 2 = letterbox (the tile letterbox too; NV12: 1.5 B/px of source), 3 = post (decode/NMS, box hold,
 * look-ahead lists, mask grow, tile merge), 4 = other (the look-ahead pixel ring's copies and the NV12 ring push), 5 = YOLOv8n plate
 * conv, 6 = mosaic cell table (box prep + walked cell colours). */
int vd_timing_enable(vd_ctx* ctx, int on);
int vd_timing_reset(vd_ctx* ctx);
int vd_timing_read(vd_ctx* ctx, int fam, double* ms, int64_t* launches, double* work);

/* ---- test hooks (parity tests call these; same kernels as the product path) -- */
/* Letterboxed RetinaFace input, NHWC with cpad channels (f32 regardless of precision). */
int vdt_letterbox(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                  int where, float* out_nhwc, int cpad);
/* vdt_letterbox for the n*T canvases of a tiling context (vd_tiles; VD_ERR_STATE when off), by
 * the tile letterbox kernel of the detect path: out_nhwc [n*T][H][W][cpad], canvas f*T+t. */
int vdt_letterbox_tiles(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                        int where, float* out_nhwc, int cpad);
/* vdt_letterbox_tiles for surfaces, by the tile letterbox kernel of the product path with the pixel
 * source the entries of that family use (NV12: source 1; any vd_yuv420 layout: 2; 16-bit words: 3).
 * The switch vd_tiles_surfaces is not read. */
int vdt_letterbox_tiles_nv12(vd_ctx* ctx, const vd_nv12* frames, int n, int h, int w, int where, float* out_nhwc, int cpad);
int vdt_letterbox_tiles_yuv420(vd_ctx* ctx, const vd_yuv420* frames, int n, int h, int w, int where, float* out_nhwc,
                               int cpad);
int vdt_letterbox_tiles_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* frames, int n, int h, int w, int where, float* out_nhwc,
                                  int cpad);
/* vdt_letterbox for NV12 frames (vd_nv12), by the NV12 letterbox kernel of the product path. */
int vdt_letterbox_nv12(vd_ctx* ctx, const vd_nv12* frames, int n, int h, int w, int where, float* out_nhwc, int cpad);
/* ... for 4:2:0 frames in any layout (vd_yuv420), by the letterbox kernel the product path runs for that layout. */
int vdt_letterbox_yuv420(vd_ctx* ctx, const vd_yuv420* frames, int n, int h, int w, int where, float* out_nhwc, int cpad);
/* ... for 10- and 12-bit 4:2:0 frames (vd_yuv420_16), by the letterbox kernel the product path runs for them. */
int vdt_letterbox_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* frames, int n, int h, int w, int where, float* out_nhwc,
                            int cpad);
/* Raw head outputs after the forward, host f32: loc [n][A][4], conf logits [n][A][2],
 * landm [n][A][10], A = number of anchors. */
int vdt_forward_heads(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                      int where, float* loc, float* conf, float* landm);
/* Letterbox bands (option face_bands). Host arithmetic only, no context: for a canvas of canvas_h
 * rows with image rows [top, top + nh) and left margin `left`, per band op k (0 the fused stem +
 * pool, 1-3 layer1.0-2) out[k] = {first row past the top band rows, first bottom band row,
 * tile rows, lo, hi}: tile rows [0, lo) and [hi, tile rows) are band tiles (none: lo 0, hi = tile rows). */
int vdt_face_band_rows(int canvas_h, int top, int nh, int left, int32_t out[4][5]);
/* The last face forward of the context: out[k] = {lo, hi, tile rows, frames whose tag matched (band
 * tiles left alone), frames whose tag did not}; all zero for a forward that ran without bands. */
int vdt_face_band_stats(vd_ctx* ctx, int32_t out[4][5]);
/* Post-processing only (decode, score, threshold, NMS, correction, int()) on
 * caller-provided host head outputs; img_hw = [n][2] source sizes. */
int vdt_postprocess(vd_ctx* ctx, const float* loc, const float* conf, int n,
                    const int32_t* img_hw, vd_boxes* faces);
/* One convolution through the product conv kernel (host f32 NHWC in/out,
 * weights [cout][kh][kw][cin] f32, BN as per-channel scale/shift, act 0=none
 * 1=relu 2=leaky(slope) 3=silu; res (optional, NHWC [n][oh][ow][cout]) added
 * before the activation when res_mode=1, after it when res_mode=2). */
int vdt_conv2d(vd_ctx* ctx, const float* x, int n, int h, int w, int cin,
               const float* wgt, int cout, int kh, int kw, int stride, int pad,
               const float* scale, const float* shift, int act, float slope,
               const float* res, int res_mode, float* y, int* oh, int* ow);
/* One plan op through the production executor (Ctx::run_ops on a one-op plan), on whole NHWC
 * buffers with the channel strides, channel offsets and frame offset a network plan would use.
 * Buffers are host f32 images converted to the context's element type on the way in and back
 * on the way out (use values exact in that type):
 *   x   [frames][xh][xw][ldx]   the op reads channels [xcoff, ...) of it
 *   y   [frames][yh][yw][ldy]   in: the prior contents, out: the contents after the op
 *   res [frames][rh][rw][res_ld] optional (conv): residual slice at res_coff, res_mode 1 = before
 *       the activation, 2 = after it; res_up: the residual is the nearest-2x source (rh, rw =
 *       the half-size map); r_is_y: the residual is another slice of the y buffer (res unused)
 *   x2  [frames][xh2][xw2][ldx2] optional (conv): a second 1x1 conv (w2, cin2, stride2, BN
 *       scale2 / shift2, no activation) summed before the activation
 * Only frames [f0, f0 + n) are run; frames <= cfg.max_batch.
 * y_is_x: the output slice lies in the x buffer (one allocation, one set of range slots); y is
 *   then only written (the x buffer after the op) and has x's shape.
 * out16: in bf16 / fp16 contexts the y buffer is kept in the context's 16-bit type as the
 *   networks keep it (0: f32, as vdt_conv2d has it); ignored in fp32 contexts. out16 = 0 with
 *   y_is_x or r_is_y in a 16-bit context is VD_ERR_ARG.
 * VDT_OP_CONV: weights w [cout][cin][kh][kw] f32, BN scale / shift [cout], act as vdt_conv2d.
 *   grp_co > 0 (fp32 contexts): output channel n reads input channels
 *   xcoff + (n / grp_co) * grp_ci + [0, cin).
 * VDT_OP_MAXPOOL: ch channels, window k, stride s, padding p (padded taps ignored).
 * VDT_OP_UPSAMPLE: ch channels, nearest 2x (yh = 2 xh, yw = 2 xw).
 * VDT_OP_DWCONV: depthwise 3x3, pad 1, w [cout][3][3] (cout = cin channels, stride 1 / 2), BN,
 *   act; the plan form: xcoff = ycoff = 0.
 * fp16-pair plan (fp32 context, option f32_split = 2) only, else untouched: xslots [frames]
 *   out: the x buffer's per-frame range slots after the op (initialised to the host max |x| of
 *   the whole x buffer of each frame); yslots [frames] in / out: the y buffer's slots (with
 *   y_is_x: the x slots). ranged = 1 when the slots exist.
 * family (out): the kernel family that took the conv (the dispatch record), "" for the others. */
enum { VDT_OP_CONV = 0, VDT_OP_MAXPOOL = 1, VDT_OP_UPSAMPLE = 2, VDT_OP_DWCONV = 3 };
typedef struct vdt_op {
    int32_t kind, frames, f0, n;
    const float* x; int32_t xh, xw, ldx, xcoff;
    float* y; int32_t yh, yw, ldy, ycoff;
    int32_t y_is_x, r_is_y, out16;
    const float* res; int32_t rh, rw, res_ld, res_coff, res_mode, res_up;
    const float* x2; int32_t xh2, xw2, ldx2;
    int32_t cin, cout, kh, kw, stride, pad, act; float slope;
    const float* w; const float* scale; const float* shift;
    int32_t grp_co, grp_ci;
    int32_t cin2, stride2; const float* w2; const float* scale2; const float* shift2;
    int32_t ch, k, s, p;
    float* xslots; float* yslots; int32_t ranged;
    char family[32];
} vdt_op;
int vdt_run_op(vd_ctx* ctx, vdt_op* op);
/* One ResNet layer1 bottleneck on host f32 NHWC x [n][h][w][cin] -> y [n][h][w][256]
 * (bf16 context): conv1 1x1 cin->64, conv2 3x3 64->64 pad 1, conv3 1x1 64->256, each
 * OIHW weights + BN as bn = [scale[cout] | shift[cout]]; ReLU after each, the residual
 * (x, or bn(downsample(x)) when wd != NULL, cin 64) added before the last ReLU.
 * fused = 1: the one-kernel fused block (block.hip); 0: the conv-by-conv chain. */
int vdt_bottleneck(vd_ctx* ctx, const float* x, int n, int h, int w, int cin,
                   const float* w1, const float* bn1, const float* w2, const float* bn2,
                   const float* w3, const float* bn3, const float* wd, const float* bnd,
                   int fused, float* y);
/* Raw YOLO Detect outputs [n][64+nc][A] (per-side DFL logits | class logits),
 * host f32, anchors in level -> y -> x order at the letterboxed canvas; *anchors
 * receives A. `out` may be NULL to query A. */
/* JPEG host entropy stage alone (no GPU): quantized coefficients [nblocks][64]
 * (natural order; blocks by component, block row, block col); out may be NULL to
 * query nblocks. */
int vdt_jpeg_coefficients(const uint8_t* data, size_t size, int16_t* out, size_t cap_blocks, int* nblocks);
int vdt_plate_raw(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                  int where, float* out, int* anchors);
/* vdt_plate_raw for the n*R*C tile inputs of a tiling context (vd_tiles; VD_ERR_STATE when off), by
 * the tile letterbox kernel and the forward of the product path: input f*R*C + (t-1) in
 * vdt_plate_raw's layout; out NULL queries A. n*T <= cfg.max_batch as for the detect calls. */
int vdt_plate_raw_tiles(vd_ctx* ctx, const uint8_t* frames, int n, int h, int w, size_t pitch,
                        int where, float* out, int* anchors);
/* vdt_plate_raw_tiles for 4:2:0 frames in any layout (vd_yuv420), by the tile-only letterbox kernel with
 * the surfaces' pixel source; the switch vd_tiles_surfaces is not read. */
int vdt_plate_raw_tiles_yuv420(vd_ctx* ctx, const vd_yuv420* frames, int n, int h, int w, int where, float* out,
                               int* anchors);
/* The cross-tile merge in its rescue form alone (vd_rescue_tiles), by the kernel of the detect path:
 * vd_tiles_merge's (plates != 0: vd_tiles_merge_plates') layout, staging, capacity and state rules on
 * caller lists read as the lists at low, cut at thr (faces score >= thr, plates score > thr). Neither
 * the rescue setting nor the switch is read. out_strong (may be NULL): the strong prefix under the
 * vd_boxes contract, exactly what the merge hands the caller in a rescue context. out_all (may be NULL):
 * the whole merged rows, count = the whole merged count, arrays cut at cap. */
int vdt_tiles_merge_low(vd_ctx* ctx, const vd_boxes* lists, int n, int h, int w, int plates, float thr,
                        vd_boxes* out_strong, vd_boxes* out_all);
/* Plate post-processing only (score, threshold, DFL decode, NMS, scale_boxes) on caller-provided raw
 * heads in vdt_plate_raw's layout, host f32 [n][64 + nc][A], for n frames of h x w whose canvas the
 * context's last plate forward (vdt_plate_raw, vd_detect_plates, vd_process) was run for; honours the
 * rescue setting like vdt_postprocess. VD_ERR_STATE before such a forward or for another canvas. */
int vdt_plate_postprocess(vd_ctx* ctx, const float* raw, int n, int h, int w, vd_boxes* plates);
/* ---- .record container I/O (host; replaces foreign/recordDeal.so) ------------
 * vd_record_extract_h265: every *.record* file of record_dir (sorted; CyberRT
 * segments) -> <out_dir>/hevcs/<camera>.h265 per camera topic
 * /drivers/camera/<camera>/compressed/image: the CompressedImage data of its
 * messages from the first key frame on, concatenated (replaces
 * recordDeal.read_record2h265_all, combine_detect.py:839).
 * vd_record_repack_h265: the same records rewritten into out_dir with each
 * extracted message's data replaced by the matching access unit of
 * <videos_dir>/<camera>_processed.h265 (or _processed.hevc, processed_<camera>.h265:
 * the desensitised stream, named as combine_detect.py:658 names it; the un-suffixed
 * <camera>.h265 is the extract step's ORIGINAL stream and is refused); everything else
 * carried over, positions and sizes recomputed (replaces
 * recordDeal.write_allH265_record_all, combine_detect.py:958). Uncompressed
 * records only. */
int vd_record_extract_h265(const char* record_dir, const char* out_dir, int* topics_written);
int vd_record_repack_h265(const char* record_dir, const char* videos_dir, const char* out_dir, int* records_written);

/* The last vd_jpeg_decode's device entropy stage: synchronisation passes run (pass 0
 * included; 0 when the host entropy stage ran). */
int vdt_jdec_stats(vd_ctx* ctx, int* passes);

/* The Q20 tap weights q[ksize] of vd_blur (host only: no context, no GPU): the routine the
 * launch path itself calls. VD_ERR_ARG for an even / out-of-range ksize or a non-finite sigma. */
int vdt_blur_weights(int ksize, float sigma, uint32_t* q);

#ifdef __cplusplus
}
#endif
#endif /* VDMI_H */
