// nets.h — host-side context, network plans and builders (internal).
#pragma once
#include "../../include/vdmi.h"
#include "vd_common.h"
#include "hold_state.h"
#include "lead_state.h"
#include "face_bands.h"

#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <map>
#include <vector>

// Every context entry of the C-ABI: the context's lock and its device.
#define VD_ENTRY(ctx)                                                        \
    if (!(ctx)) return vd_set_error(VD_ERR_ARG, "null context");              \
    std::lock_guard<std::mutex> _lk((ctx)->mu);                                \
    if (hipSetDevice((ctx)->device) != hipSuccess)                             \
        return vd_set_error(VD_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device)

// [a, a + bytes) and [b, b + bytes) share a byte (device frame batches of one geometry)
static inline bool vd_ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return bytes && x < y + bytes && y < x + bytes;
}

static inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static inline uint16_t f32_to_f16_rne(float f) {   // IEEE binary16, round to nearest even (clang _Float16)
    const _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

static inline float f16_bits_to_f32(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}

// host-side 16-bit encoding of the context's half type
static inline uint16_t to_half(bool f16, float v) { return f16 ? f32_to_f16_rne(v) : f32_to_bf16_rne(v); }
static inline float from_half(bool f16, uint16_t u) {
    if (f16) return f16_bits_to_f32(u);
    uint32_t w = (uint32_t)u << 16;
    float v;
    memcpy(&v, &w, 4);
    return v;
}

struct HT {   // host tensor from the VDW1 container
    std::vector<int> shape;
    std::vector<float> data;
};
using WMap = std::unordered_map<std::string, HT>;
int vd_parse_vdw1(const void* blob, size_t bytes, WMap& out);
const HT* find_t(const WMap& W, const std::string& k);
void vd_resize_mode(int ih, int iw, int nh, int nw, int* mode, double* sx, double* sy);

struct Act {          // NHWC activation buffer sized for cfg.max_batch frames
    void* p = nullptr;
    int h = 0, w = 0, c = 0;   // c = channel stride
    bool f32 = false;
    // fp16-pair plan (f32_split = 2): per-frame running max |x| [max_batch] that every
    // producer folds its outputs into (vd_kernel.h AmaxTrack), or a static bound
    // for the letterboxed canvas (amax NULL)
    unsigned* amax = nullptr;
    float bound = 0.f;
    bool exact16 = false;      // every value an integer of |x| <= 2048 (the face letterbox canvas)
};

struct Conv {
    int cin = 0, cin_pad = 0, cout = 0, npad = 0, kh = 0, kw = 0, stride = 1, pad = 0, kpad = 0, act = 0;
    float slope = 0.f;
    void* w = nullptr;
    void* wx3 = nullptr;       // fp32 + f32_split: [npad][kpad/32][3][32] bf16 / [..][2][32] fp16 planes (conv_x6.hip)
    float* scale_x = nullptr;  // fp16 pairs: BN scale times the row's 2^-e
    void* wx3_chain = nullptr; // fp16 pairs as chain32.hip's conv1': K permuted inside each 32-step
    int split = 0;             // fp32: VdTune::f32_split when the weights were packed
    float* scale = nullptr;
    float* shift = nullptr;
    double flops_per_px = 0;   // algorithmic FLOPs per output pixel (real Cin, no padding)
    int grp_co = 0, grp_ci = 0; // grouped (conv_x6_halo only): rows [g grp_co, +grp_co) read input channels g grp_ci + [0, cin)
};

// One fused layer1 bottleneck (block.hip, block.cpp): the per-conv bf16 weights
// of conv1/conv2/conv3(/downsample) repacked for the fused kernel.
struct Block {
    int cin = 0, ds = 0;
    bool f32 = false;                         // fp32 plan (block32.hip): fp16-pair planes / fragments
    int c1 = -1, c2 = -1, c3 = -1, cd = -1;   // the per-conv plans (flops, unfused fallback)
    void* w1 = nullptr;
    void* w2 = nullptr;
    void* w3 = nullptr;
    void* wd = nullptr;
    float* bn = nullptr;
};

// Depthwise 3x3 conv + BN + activation (dwconv.hip): MobileNetV1 conv_dw.
struct DwConv {
    int c = 0, stride = 1, act = 0;
    float slope = 0.f;
    void* w = nullptr;                 // [9][c] in the compute type
    float* scale = nullptr;
    float* shift = nullptr;
};

enum { OP_CONV = 0, OP_MAXPOOL = 1, OP_UPSAMPLE = 2, OP_BLOCK = 3, OP_STEMPOOL = 4, OP_DWCONV = 5, OP_CHAIN = 6 };

struct Op {
    int kind = OP_CONV;
    int conv = -1;
    Act x; int xcoff = 0;
    Act y; int ycoff = 0;
    Act r; int rcoff = 0; int rmode = 0; int rup = 0;
    int conv2 = -1; Act x2;            // fused second 1x1 conv (downsample branch), summed pre-activation
    int ch = 0, k = 0, s = 0, p = 0;   // maxpool / upsample
    int blk = -1;                      // OP_BLOCK: index into Ctx::blocks (x -> y)
    void* wf = nullptr;                // OP_STEMPOOL: conv's weight fragments (conv = the stem conv)
    Act y2;                            // OP_CHAIN: conv = conv3 (x -> y, identity r), conv2 = next conv1 (y -> y2)
    int lane = 0;                      // 1: runs on Ctx::stream_side (face SSH levels 1-2)
    int dep = -1;                      // op index (other lane) whose completion this op waits for
    int band = -1;                     // face stem / layer1 (fp32 pairs): index into FaceBands (letterbox band tiles)
};

struct Net {
    std::vector<Op> ops;
    unsigned* amax = nullptr;                        // fp16-pair plan: this net's max slots, zeroed per run
    size_t amax_bytes = 0;
    int stage_end[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // op index after each backbone stage (face: 0=stem,1..4=layerN)
    int conv_fam = 0;                                // timing family of its convs (0 face, 5 plate)
};

struct PostScratch {   // per-net candidate / NMS scratch sized for max_batch x A
    uint64_t* keys = nullptr;
    int* count = nullptr;
    float4* box = nullptr;
    int* cls = nullptr;
    float4* nbox = nullptr;
    float* area = nullptr;
    uint64_t* sort = nullptr;
    uint8_t* supp = nullptr;
    int sort_cap = 0;
    // the last call's complete keep lists [max_batch][kcap] (library-owned): the
    // mosaic reads these, never the caller's cap-limited copies; vd_read_boxes
    // hands them out
    int kcap = 0;
    int* kcount = nullptr;
    int* kall = nullptr;               // rescue: the whole keep counts (kcount: the strong prefix)
    int* kxyxy = nullptr;
    float* kxyxy_f = nullptr;
    float* kscore = nullptr;
    int* klabel = nullptr;
    int kn = 0;                        // frames in the last call
};

// Letterbox bands (face_bands.h, bands.hip): the band tiles of the stem's and layer1's
// outputs stay in their buffers between face forwards; per band op and frame slot the device keeps
// the conditions they were written under (tag) and their maximum (bmax).
struct FaceBands {
    bool plan = false;                 // the face plan has the four band ops (fp32 pairs, ResNet-50, fused stem + pool)
    int op[VD_BAND_OPS] = {-1, -1, -1, -1};   // their indices in face.net.ops
    unsigned long long* tag = nullptr; // [4][max_batch], zero: never written
    unsigned* bmax = nullptr;          // [4][max_batch]
    unsigned* scratch = nullptr;       // [4][max_batch], then stats [4][2]: in the face net's per-call zeroed slots
    unsigned* stats = nullptr;
    unsigned epoch = 1;                // nonzero; a new value forgets every tag
    int geom[6] = {0, 0, 0, 0, 0, 0};  // the last letterbox: frame h, w, top, nh, left, nw (face_letterbox_args)
    int last_geom[6] = {0, 0, 0, 0, 0, 0};    // ... of the last forward that ran with bands
    bool active = false;               // a forward with bands is being queued (run_*_op fill BandArgs)
    FaceBandPlan cur{};                // its tile rows
    bool ran = false;                  // the last forward ran with bands (vdt_face_band_stats)
    void forget() { if (!++epoch) ++epoch; }
};

struct FaceNet {
    bool loaded = false;
    int in_h = 640, in_w = 640;
    bool s2d = false;               // 16-bit / fp32-pair plans: stem input in space-to-depth form (pre.hip letterbox_s2d_kernel)
    bool mnet = false;              // MobileNetV1-0.25 backbone (cfg_mnet) instead of ResNet-50
    Act input;
    Net net;
    Act heads[3];
    int loff[3] = {0, 0, 0};
    int A = 0;
    float* anchors = nullptr;
    PostScratch post;
};

struct PlateNet {
    bool loaded = false;
    int nc = 1;
    int imgsz = 640;
    int hstride = 0;                // head channel stride (64 DFL + nc, padded to 8)
    Act input;                      // letterboxed canvas, allocated for imgsz x imgsz
    bool s2d = false;               // 16-bit / fp32-pair plans: canvas in space-to-depth form, model.0 as a 2x2 conv
    std::vector<std::pair<std::string, Act>> bufs;   // named activation buffers (max canvas)
    std::vector<std::pair<std::string, int>> conv_idx;
    std::vector<std::pair<long long, Net>> plans;    // per canvas (h<<32|w)
    Act head[3];
    int A_max = 0;
    PostScratch post;
    // current call
    int ch = 0, cw = 0, A = 0, lh[3] = {0, 0, 0}, lw[3] = {0, 0, 0}, loff[3] = {0, 0, 0};
};

struct BoxTargets {
    int cap = 0;
    int* count = nullptr;
    int* xyxy = nullptr;
    float* xyxy_f = nullptr;
    float* score = nullptr;
    int* label = nullptr;
};

struct BoxListIn {   // a caller's box list as the kernels take it (Ctx::box_list_in)
    const int* cnt = nullptr;
    const int* xy = nullptr;
    bool staged = false;   // copied into the context's staging, which the next call reuses
};

struct PlaneRows {   // one plane of a ping-pong history: bytes of a slot's row before and after a regrow
    size_t old_row, new_row;
};

struct TimedEv {
    hipEvent_t a, b;
    int fam;
    double work;
};

struct Ctx {
    vd_cfg cfg{};
    int device = 0;
    bool f32 = false;
    bool f16 = false;                             // VD_PREC_FP16: fp16 operands/activations (the bf16 plan's kernels)
    VdTune tune;                                  // kernel-selection switches (vd_set_option)
    hipStream_t stream = nullptr, own_stream = nullptr;
    hipStream_t stream2 = nullptr;               // plate branch runs beside the face branch
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t stream_side = nullptr;           // the face net's second lane (SSH levels 1-2 beside level 0)
    std::vector<hipEvent_t> lane_ev;             // per face op: completion event for the other lane
    hipEvent_t ev_side = nullptr;                // side lane done (joined before the face decode)
    hipEvent_t ev_half = nullptr;                // option face_groups: fork of the frame groups
    std::vector<hipStream_t> group_streams;      // option face_groups: streams of frame groups 1..G-1
    std::vector<hipEvent_t> group_events;        //   and their completion events (joined by the context stream)
    std::map<int, unsigned*> amax_snaps;         // per conv: its input's range slots frozen (in-place concat)
    int fork_at = -1;                                // run_ops records ev_fork after this many face ops
    std::mutex mu;
    std::vector<void*> allocs;
    std::vector<Conv> convs;
    std::vector<Block> blocks;
    std::vector<DwConv> dwconvs;
    FaceNet face;
    PlateNet plate;
    void* stage_in = nullptr;  size_t stage_in_bytes = 0;
    void* stage_out = nullptr; size_t stage_out_bytes = 0;
    void* stage_box = nullptr; size_t stage_box_bytes = 0;
    void* stage_box2 = nullptr; size_t stage_box2_bytes = 0;
    void* mosaic_table = nullptr; size_t mosaic_table_bytes = 0;
    void* blur_table = nullptr; size_t blur_table_bytes = 0;   // Gaussian mode: box plan + dependent-box scratch
    // box hold (hold.hip; cfg.hold_frames > 0 only, allocated by the first holding call)
    HoldState hold;                               // K, P, motion mode, valid history slots, current buffer, last frame size
    int* hold_hist[2] = {nullptr, nullptr};       // ping-pong history: [depth] counts, then (64-B aligned) [depth][hcap][4]
    int hold_hcap = 0;                            // history row capacity (boxes)
    void* hold_rows = nullptr; size_t hold_rows_bytes = 0;   // the last call's merged rows, ages, |B|, |D|
    HoldArgs hold_last{};                         // the last launch (merged-row pointers for the readers)
    int hold_n = 0;                               // frames of the last holding call
    // look-ahead hold (lead.hip; vd_lead with J > 0 only, allocated by the first lead call)
    LeadState lead;                               // J, motion, pending frames, current list buffer, pending geometry
    int* lead_ring[2] = {nullptr, nullptr};       // ping-pong pending lists (vd_common.h LeadArgs gives the layout)
    int lead_hcap = 0;                            // D-list capacity of a ring slot (boxes); rows: (K + 1) * lead_hcap
    int lead_slots = 0;                           // slots the ring buffers were sized for (= delay)
    void* lead_pix = nullptr; size_t lead_pix_bytes = 0;     // pixel ring: delay frames (RGB, packed NV12, or packed 16-bit words U first), oldest first
    void* lead_rows = nullptr; size_t lead_rows_bytes = 0;   // the last call's merged rows, labels, |B|, |D|, |D ++ H|
    LeadArgs lead_last{};                         // the last launch (merged-row pointers for the readers)
    int lead_m = 0;                               // frames the last lead call emitted
    // weak-detection rescue (rescue.hip; vd_rescue): off = both lows 0, no launch, no memory
    float rescue_low[2] = {0.f, 0.f};             // face_low, plate_low (0: that net has no weak boxes)
    int rescue_span = 0;                          // S
    HoldState rescue_hs;                          // the history bookkeeping of hold_state.h with K = W = max(1, hold_frames)
    int* rescue_hist[2] = {nullptr, nullptr};     // ping-pong: [W] counts (64 B), [W][hcap][4] boxes, [W][hcap] since
    int rescue_hcap = 0;
    void* rescue_rows = nullptr; size_t rescue_rows_bytes = 0;   // the last call's E rows, since, |E|, |D|, |R faces|, w_since
    RescueArgs rescue_last{};                     // the last launch (row pointers for the readers)
    int rescue_n = 0;                             // frames of the last rescue call (0: none)
    bool rescue_on() const { return rescue_low[0] > 0.f || rescue_low[1] > 0.f; }
    // rescue on tiled nets (vd_rescue_tiles; 0: vd_rescue and vd_tiles refuse each other, as they always
    // did). On: a tiled net's lists run at `low`, the merge makes the split (tiles.hip LOW form)
    int rescue_tiles = 0;
    int rescue_tiles_set(int on);
    int rescue_set(float face_low, float plate_low, int span);
    int rescue_history(int hcap);                 // history buffers of at least this row capacity
    // E = D ++ R of n consecutive frames into rescue_last's rows, and the history update (RescueArgs' lists)
    int launch_rescue(int n, int h, int w, RescueArgs a);
    int rescue_read_rows(int n, vd_boxes* out);   // E rows -> caller lists (label = since)
    // mask shaping (mask.hip; vd_mask): nothing is allocated or launched while the setting is the default
    int mask_shape = VD_MASK_RECT, mask_grow = 0;
    void* mask_rows = nullptr; size_t mask_rows_bytes = 0;   // grown merged rows: [n][mcap][4], then counts [n]
    MaskArgs mask_last{};                         // the last grow launch (row pointers for the restore pass)
    // box-scaled strength (vd_cells): 0 = off, every launch and byte as before
    int cells = 0;
    // NV12 frames (include/vdmi.h at vd_nv12; pre.hip, nv12.hip). nv12_src.on marks an NV12 call in
    // flight: the letterbox argument builders hand it to the kernels, and `dframes` / `pitch` of the face
    // and plate paths are then the first luma byte and the planes' row pitch. Nv12Scope clears it.
    Nv12Src nv12_src{};
    // a batch of 4:2:0 surfaces in device memory, in any layout of vd_yuv420 (nv12.h); the *_nv12 entries
    // pass the NV12 descriptor through the same path
    using Nv12Dev = Yuv420Dev;
    // the caller's input surfaces on the device: as they are, or (host) staged packed in their own
    // layout in stage_in (1.5 B/px; 16-bit words: 3 B/px). d: the caller's surfaces, host or device
    int nv12_in(const Nv12Dev& d, int n, int h, int w, int where, Nv12Dev* o);
    // where the output pass writes: the caller's surfaces, or (host) packed surfaces in stage_out ...
    int nv12_out_begin(const Nv12Dev& d, int n, int h, int w, int where, Nv12Dev* o);
    // ... copied back plane by plane, the picture's bytes of every row only (queued; the caller synchronises)
    int nv12_out_finish(const Nv12Dev& d, const Nv12Dev& o, int n, int h, int w, int where);
    // the NV12 output pass behind the mask setting, what launch_shaped is to RGB frames: grow, the
    // rectangular pass (RECT_MOSAIC: nv12.hip, one launch; RECT_SMOOTH: smooth.hip, copy + box pass),
    // then under VD_MASK_ELLIPSE the restore of both planes; all family 1
    int launch_nv12_pass(const Nv12Dev& in, const Nv12Dev& out, int n, int h, int w, const int* cnt0, const int* xy0,
                         int cap0, const int* cnt1, const int* xy1, int cap1, int pass, int level, int cells);
    // the rectangular pass an NV12 blurring call of this context runs, or -1: the fixed-kernel Gaussian
    // (VD_BLUR_GAUSSIAN with cells off) has no NV12 pass
    int nv12_cfg_pass() const {
        return cfg.blur_mode != VD_BLUR_GAUSSIAN ? (int)RECT_MOSAIC : (cells ? (int)RECT_SMOOTH : -1);
    }
    // tiled face detection (tiles.hip, pre.hip letterbox_tiles_kernel; vd_tiles): nothing is allocated
    // or launched while rows * cols == 1
    int tile_rows = 1, tile_cols = 1, tile_overlap = 0;
    void* tiles_buf = nullptr; size_t tiles_buf_bytes = 0;   // merged rows + spill scratch, floor(max_batch / T) frames
    void* tiles_in = nullptr; size_t tiles_in_bytes = 0;     // vd_tiles_merge: host / unaligned caller lists staged
    TileMergeArgs tiles_last{};                   // the last merge (merged-row pointers for the readers)
    int tiles_kn = 0;                             // frames of the last merge
    bool face_rows_merged = false;                // the last face call's lists are tiles_last's rows, not face.post's
    bool tiles_on() const { return tile_rows * tile_cols > 1; }
    // which nets the tiling applies to (vd_tiles_nets; VD_TILE_FACES | VD_TILE_PLATES): faces alone by
    // default, so a tiling context runs the plate net exactly as an untiled one
    int tile_nets = VD_TILE_FACES;
    bool faces_tiled() const { return tiles_on() && (tile_nets & VD_TILE_FACES); }
    bool plates_tiled() const { return tiles_on() && (tile_nets & VD_TILE_PLATES); }
    int tiles_nets_set(int nets);
    // whether the 4:2:0 surface entries run a tiled net (vd_tiles_surfaces; 0: they refuse, as they always
    // did). Read by those entries only: no capacity depends on it, so setting it keeps the hold history.
    int tile_surfaces = 0;
    int tiles_surfaces_set(int on);
    // the surface entries' refusal of a call that would run a tiled net while the switch is off
    int tiles_surfaces_check(const char* who, int flags) const;
    // tiled plate detection: the plate lists' merged rows + spill scratch (allocated by the first merge)
    void* ptiles_buf = nullptr; size_t ptiles_buf_bytes = 0;
    TileMergeArgs ptiles_last{};                  // the last plate merge (merged-row pointers for the readers)
    int ptiles_kn = 0;                            // frames of the last plate merge
    bool plate_rows_merged = false;               // the last plate call's lists are ptiles_last's rows, not plate.post's
    int tiles_T() const { return 1 + tile_rows * tile_cols; }
    int tiles_set(int rows, int cols, int overlap_pct);
    int tiles_grid(int h, int w, TileGrid* g);    // the setting's rectangles of an h x w frame
    int face_letterbox_tiles(const uint8_t* dframes, int n, int h, int w, size_t pitch, const TileGrid& g);
    // the T lists of each of n frames (rows of icap, device) -> tiles_last's merged rows and the caller's targets
    // plates: the class-aware merge at cfg.plate_iou into ptiles_last's rows (split: TileMergeArgs)
    // low_on: the lists are the lists at `low` and the merge cuts the strong prefix at thr (TileMergeArgs)
    int tiles_merge(int n, const TileGrid& g, const int* cnt, const float* xyxy_f, const float* score, const int* label,
                    int icap, const BoxTargets& t, bool plates = false, bool split = false, bool low_on = false,
                    float thr = 0.f);
    int tiles_check(int n, int h, int w, TileGrid* g);   // the grid, and n * T <= max_batch
    // after face_forward(n * T): per-input post (sizes per input) + merge into the caller's targets
    int face_post_tiled(int n, int h, int w, const TileGrid& g, const BoxTargets& t);
    // the face lists a call leaves for the blur / the hold / vd_read_boxes: per-net keep lists or merged rows
    int face_rows_cap() const { return faces_tiled() ? tiles_T() * face.post.kcap : face.post.kcap; }
    int plate_rows_cap() const { return plates_tiled() ? tiles_T() * plate.post.kcap : plate.post.kcap; }
    // JPEG frame decode (jpeg_host.cpp): pinned host staging, device copy, planes
    void* jpeg_host = nullptr; size_t jpeg_host_bytes = 0;
    void* jpeg_dev = nullptr; size_t jpeg_dev_bytes = 0;
    void* jpeg_planes = nullptr; size_t jpeg_planes_bytes = 0;
    hipEvent_t jpeg_ev = nullptr;                 // last H2D out of jpeg_host / jenc_host
    // device entropy decode (jpeg_dec.hip): pinned segments + tables + metadata, device copy, dense blocks
    void* jdec_host = nullptr; size_t jdec_host_bytes = 0;
    void* jdec_dev = nullptr; size_t jdec_dev_bytes = 0;
    void* jdec_work = nullptr; size_t jdec_work_bytes = 0;
    int jdec_passes = 0;                          // sync passes of the last device decode (test hook)
    // JPEG frame encode (jpeg_enc.cpp): device coefficients + tables, pinned host copy
    void* jenc_dev = nullptr; size_t jenc_dev_bytes = 0;
    void* jhuf_dev = nullptr; size_t jhuf_dev_bytes = 0;   // device entropy stage buffers
    void* jseg_host = nullptr; size_t jseg_host_bytes = 0; // pinned: packed entropy-coded segments
    void* jenc_host = nullptr; size_t jenc_host_bytes = 0;
    int jpeg_threads = 16;                        // host entropy-decode threads
    // fp16-pair plan: per-frame activation max slots, one region per network (face 0,
    // plates 1) of kAmaxActs activations x max_batch frames
    static constexpr int kAmaxActs = 256;
    unsigned* amax_pool = nullptr;
    int amax_owner = 0;
    int amax_next[2] = {0, 0};
    int amax_begin(int owner);                    // builders: slots of `owner` restart
    unsigned* amax_region(int owner) const { return amax_pool ? amax_pool + (size_t)owner * kAmaxActs * cfg.max_batch : nullptr; }
    size_t amax_region_bytes() const { return (size_t)kAmaxActs * cfg.max_batch * 4; }
    bool timing = false;
    std::vector<TimedEv> ev_pool;
    size_t ev_used = 0;

    int dalloc(void** p, size_t bytes);
    int act(Act& a, int h, int w, int c, bool f32out = false, bool half = false);   // half: 2-byte elements
    int ensure_staging(void** p, size_t* have, size_t need);
    int ensure_pinned(void** p, size_t* have, size_t need);
    int upload_conv(Conv& cv, const std::vector<float>& w_oihw, const std::vector<float>& scale,
                    const std::vector<float>& shift);
    int make_conv_bn(const WMap& W, const std::string& wkey, const std::string& bn, float eps, int stride, int pad,
                     int act, float slope, int* out_idx);
    // convs + BatchNorms {(wkey, bn)} concatenated along Cout (same input, kernel, stride, pad)
    int make_conv_bn_cat(const WMap& W, const std::vector<std::pair<std::string, std::string>>& parts, float eps,
                         int stride, int pad, int act, float slope, int* out_idx);
    int make_conv_cat(const WMap& W, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys,
                      int act, int* out_idx,
                      const std::vector<int>* cin_perm = nullptr);
    int add_conv_dual(Net& net, int ci, const Act& x, int c2, const Act& x2, Act& y);
    bool dual_ok(int ci, int c2, const Act& y) const;
    int add_conv(Net& net, int ci, const Act& x, int xcoff, Act& y, int ycoff, const Act* res = nullptr,
                 int rcoff = 0, int rmode = 0, int rup = 0);
    bool block_ok(int c1, int c2, int c3, int cd, const Act& x) const;
    int make_block(int c1, int c2, int c3, int cd, int* idx);
    int add_block(Net& net, int bi, const Act& x, Act& y);
    int run_block_op(const Op& op, int f0, int n, int fam = 0);
    int add_stem_pool(Net& net, int ci, const Act& x, Act& y);
    int make_dwconv_bn(const WMap& W, const std::string& wkey, const std::string& bn, float eps, int stride, int act,
                       float slope, int* idx);
    int add_dwconv(Net& net, int di, const Act& x, Act& y);
    int run_dwconv_op(const Op& op, int f0, int n);
    int run_chain_op(const Op& op, int f0, int n, int fam = 0);
    void fuse_chains(Net& net, size_t begin);
    int run_stem_pool_op(const Op& op, int f0, int n, int fam = 0);
    void t_begin(int fam, double work);
    void t_end();
    int run_conv_op(const Op& op, int f0, int n, int fam = 0);
    int run_ops(const Net& net, int b, int e, int f0, int n);
    int face_lanes(const int (&fpn)[5], const int (&ssh_b)[3], const int (&ssh_e)[3]);
    int chain32_weights(Conv& c1);
    void fuse_chains32(Net& net, size_t begin);
    int run_net(const Net& net, int n, int mb = 0, int split = 0);
    const uint8_t* frames_to_device(const uint8_t* frames, int n, int h, size_t pitch, int where, int* rc);
    int check_frames(int n, int h, int w, size_t pitch);
    int box_targets(vd_boxes* out, int n, BoxTargets& t);
    int box_finish(vd_boxes* out, int n, const BoxTargets& t);
    int host_box_staging(void** buf, size_t* have, int cap, int n, BoxTargets& t);
    // A caller's list of `rows` rows as device pointers. A host list is refused (VD_ERR_CAPACITY) when a
    // count exceeds cap, then staged `stage_off` bytes into stage_box2 (sized for stage_bytes if that is
    // more: a call with two lists). vec16: the consumer reads boxes as 16-byte vectors (hold.hip,
    // lead.hip, rescue.hip), so a device list whose xyxy is not 16-byte aligned is staged too; the blur
    // and mask kernels read scalars and take a device list as it is. The next call reuses the staging:
    // a caller that staged and does not wait for host output synchronises before it returns.
    int box_list_in(const char* who, const vd_boxes* b, int rows, bool vec16, size_t stage_off, BoxListIn* o,
                    size_t stage_bytes = 0);
    // Merged rows (a HoldArgs view: rows, labels, counts, the offset to skip) -> the caller's lists
    // through the hold's gather; host lists are staged, copied whole, and waited for.
    int rows_out(const HoldArgs& view, int n, int held_only, vd_boxes* out, const char* what);
    // A ping-pong pair regrown to `bytes` each: both heads cleared; with cur >= 0 buf[cur]'s head_copy
    // bytes and its planes (consecutive behind the head, `slots` rows each) carried over from the old
    // row pitch to the new; then the stream is waited for and the old pair freed.
    int regrow_pair(int* (&buf)[2], size_t bytes, size_t head, int cur, size_t head_copy, int slots,
                    std::initializer_list<PlaneRows> planes, const char* what);
    int face_letterbox(const uint8_t* dframes, int n, int h, int w, size_t pitch);
    void face_letterbox_args(const uint8_t* dframes, int n, int h, int w, size_t pitch, LetterboxArgs* a);
    // plain: the n canvases are whole frames of the last face_letterbox_args geometry (not tile inputs)
    int face_forward(int n, bool plain = true);
    int face_forward_run(int n);                  // the forward itself: frame groups, or one launch per op
    FaceBands bands;
    int bands_alloc();                            // vd_build_face: the band ops' state, when the plan has them
    bool bands_begin(int n, bool plain);          // face_forward: does this forward run with bands?
    void band_args(int k, int f0, BandArgs* a) const;
    int bands_publish(int f0, int n);             // after a frame group's last op, on `stream`
    // tiles: net input b is a tile of tiles->th x tiles->tw source pixels unless b % tiles->T == 0
    int face_post(int n, int img_h, int img_w, const BoxTargets& t, const TileGrid* tiles = nullptr);
    int launch_mosaic(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                      const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int level, int cells);
    // the scaled smooth blur (smooth.hip): the copy and the box pass, family 1
    int launch_smooth(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                      const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int level, int cells);
    int launch_blur(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                    const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int ksize, float sigma);
    bool mask_on() const { return mask_shape != VD_MASK_RECT || mask_grow != 0; }
    // lists 0 / 1 grown by mask_grow into mask_last's merged rows (zero_tail: entries past the count zeroed)
    int launch_mask_grow(int n, const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1,
                         int zero_tail = 0);
    // VD_MASK_ELLIPSE: out <- in outside every ellipse of mask_last's rows, after the rectangular pass
    int launch_mask_restore(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch);
    // the rectangular pass of the blurring calls behind the mask setting: grow, blur / mosaic / smooth, restore
    enum { RECT_MOSAIC = 0, RECT_GAUSSIAN = 1, RECT_SMOOTH = 2 };
    int launch_shaped(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                      const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1, int pass, int level,
                      int ksize, float sigma, int cells);
    // launch_shaped with the pass the context is configured for (vd_process, the lead step): pixelation,
    // or in a Gaussian-mode context the fixed kernel / under vd_cells the scaled smooth blur
    int launch_cfg_pass(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch, const int* cnt0,
                        const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1);
    // B = D ++ H of n consecutive frames into hold_last's merged rows, and the history update
    int launch_hold(int n, int h, int w, const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1,
                    int cap1);
    int hold_history(int hcap);                   // history buffers of at least this row capacity
    int hold_set_motion(int mode);                // vd_hold_motion: a change forgets the history and its buffers
    int hold_read(int n, int held_only, vd_boxes* out);   // merged rows -> caller lists (label = age)
    // look-ahead hold: the list capacity a lead call over lists of cap0 + cap1 needs, the refusals shared by
    // both lead calls, and the ring buffers (a narrower pair's pending slots are carried over)
    int lead_need(int cap0, int cap1) const;
    int lead_check(const char* who, int mode, int n, int h, int w, size_t pitch, int flush, int depth = 0, int shift = 0);
    int lead_buffers(int need, size_t frame_bytes);
    void lead_free();                             // vd_lead: a change of setting drops the rings
    // One lead step: the n pushed frames' D lists (and, under hold, hold_last's rows) join the window, the m
    // oldest frames get B = D ++ H ++ A in lead_last's merged rows, the rest becomes the next ring. With
    // pixels (din / dout device pointers, dout for m frames) the emitted frames are blurred and the pixel
    // ring is updated. The state advances only when everything was queued. VD_LEAD_MODE_NV12: the frames
    // are the surfaces *nvin (n of them), the emitted ones go to *nvout (m of them), and the ring holds
    // packed surfaces (pitch w, chroma at h * w, 1.5 * h * w bytes a slot); din / dout / pitch are not used.
    int lead_step(int mode, const uint8_t* din, uint8_t* dout, int n, int h, int w, size_t pitch, int flush,
                  const int* cnt0, const int* xy0, int cap0, const int* cnt1, const int* xy1, int cap1,
                  const Nv12Dev* nvin = nullptr, const Nv12Dev* nvout = nullptr);
    int lead_read(int n, int which, vd_boxes* out);   // merged rows -> caller lists (label 0, +a, -a)
};

// An NV12 call's scope: the context reads NV12 sources from here to the end of the entry point.
struct Nv12Scope {
    Ctx* c;
    Nv12Scope(Ctx* ctx, const Ctx::Nv12Dev& d, int matrix, int range, bool on = true) : c(ctx) {
        if (!on) return;
        c->nv12_src.on = d.depth ? 3 : (d.nv12() ? 1 : 2);   // the NV12 letterbox kernels, the ones for any layout, or for 16-bit words
        c->nv12_src.sh16 = d.depth ? d.shift + d.depth - 8 : 0;
        c->nv12_src.uv_offset = d.u;
        c->nv12_src.v_offset = d.v;
        c->nv12_src.cpitch = d.cpitch;
        c->nv12_src.step = d.step;
        c->nv12_src.frame_stride = d.stride;
        c->nv12_src.k = vd_nv12_coef(matrix, range);
    }
    ~Nv12Scope() { c->nv12_src = Nv12Src{}; }
};
// the layout rules of a vd_nv12 descriptor for n frames of h x w (colour: matrix and range too); VD_ERR_ARG
int vd_nv12_check(const char* who, const vd_nv12* d, int n, int h, int w, bool colour);
// ... of a vd_yuv420 descriptor (the message names the field); extent: the bytes the n frames span
int vd_yuv420_check(const char* who, const vd_yuv420* d, int n, int h, int w, bool colour, size_t* extent = nullptr);
// ... of a vd_yuv420_16 descriptor
int vd_yuv420_16_check(const char* who, const vd_yuv420_16* d, int n, int h, int w, bool colour, size_t* extent = nullptr);
// bytes of source a letterbox reads per pixel of the frame rows it touches (timing work)
static inline double vd_src_bpp(const Nv12Src& nv) { return nv.on == 3 ? 3.0 : (nv.on ? 1.5 : 3.0); }   // 16-bit words: 3 B/px too

// a host list whose count[i] exceeds cap names boxes the caller does not hold: refused, never skipped silently
int vd_count_check(const char* who, const int* count, int rows, int cap);
int vd_alloc_post(Ctx& ctx, PostScratch& ps, int A, int kcap);
void vd_post_keep_args(PostScratch& ps, PostArgs& p, int n);
int vd_build_face(Ctx& ctx, const WMap& W);
int vd_build_plate(Ctx& ctx, const WMap& W);
// letterboxed: the canvas was already written (vd_launch_letterbox_pair in vd_process).
// tiles: the n * (T - 1) tile inputs of the n frames instead (input f * (T - 1) + (t - 1)).
int vd_plate_forward(Ctx& ctx, const uint8_t* dframes, int n, int h, int w, size_t pitch, bool letterboxed = false,
                     const TileGrid* tiles = nullptr);
int vd_plate_letterbox_args(Ctx& ctx, const uint8_t* dframes, int n, int h, int w, size_t pitch, LetterboxArgs* a);
// row0: the keep rows of the n inputs start at row row0 of plate.post (the tile inputs behind the whole frames)
int vd_plate_post(Ctx& ctx, int n, int img_h, int img_w, const BoxTargets& t, int row0 = 0);
// What a call that runs the plate net does: forward + post of the n frames, and with `tiles` (the
// plate net is tiled) the tile inputs' forward + post and the merge into ptiles_last's rows.
int vd_plate_detect(Ctx& ctx, const uint8_t* dframes, int n, int h, int w, size_t pitch, bool letterboxed,
                    const TileGrid* tiles, const BoxTargets& t);
// vd_tiles_merge / vd_tiles_merge_plates: the merge step alone on caller lists (staging, checks, the caller's
// `out`). low_on / thr: the test hook vdt_tiles_merge_low alone (TileMergeArgs); the entries keep 0.
int vd_tiles_merge_lists(Ctx* ctx, const char* who, bool plates, const vd_boxes* lists, int n, int fh, int fw, vd_boxes* out,
                         bool low_on = false, float thr = 0.f);
