// vd_common.h — what the host code and the kernels exchange: argument structs, VdTune,
// launcher prototypes. Device helpers shared by the kernel files: vd_kernel.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stddef.h>
#include "nv12.h"

enum VdAct { VD_ACT_NONE = 0, VD_ACT_RELU = 1, VD_ACT_LEAKY = 2, VD_ACT_SILU = 3 };
enum VdResMode { VD_RES_NONE = 0, VD_RES_PRE_ACT = 1, VD_RES_POST_ACT = 2 };

// Kernel-selection switches of one context. The defaults ARE the production plan;
// vd_set_option (include/vdmi.h) changes them per context for A/B measurements and
// for tests that force a kernel form onto small shapes. Plan-time switches
// (block_fuse, chain, stem_pool, ssh_fuse, plate_s2d) take effect at the next
// vd_load_weights; the others at the next launch. Nothing is read from the
// environment.
struct VdTune {
    int conv_stream = 1;      // streaming 1x1 kernel (conv1x1.hip) for K in {64,128,256}
    int conv_stream512 = 1;   //   ... and K = 512
    int conv_dual = 1;        // conv3 + downsample as one streaming launch
    int conv_taps = 1;        // streaming taps kernel for small K (YOLO)
    int conv_n192 = 1;        // 192-wide N tile for Cout 129..192 (fused SSH conv)
    int conv_small = 512;     // below this many 128-row tiles the GEMM takes 64-row tiles
    int conv_big = 100;       // min 256x256 tiles for the phased kernel (0: off)
    int conv_big_kmin = 512;  // min K for the phased kernel
    int stream_ntt = 16;      // streaming 1x1: 256-channel slices where Cout allows (8: 128)
    int lb_pair = 1;          // one letterbox launch for both canvases when geometry allows
    int mosaic_map = 1;       // mosaic output pass: per-band vector maps (0: generic path)
    int mosaic_nt = 0;        //   non-temporal output stores (1), and source loads (3)
    int mosaic_cells = 32;    //   cell-table kernel: workgroups per frame
    int mosaic_gather = 0;    //   fused output pass: a thread's band cells walked, then their loads issued together
    int mosaic_rows = 0;      //   fused output pass: rows per band (4 / 8 / 16 / 24 / 32; 0 = auto: 4 for rows
                              //   of >= 8 KB (4K), else 8)
    int mosaic_fused = 1;     //   one launch: the output pass computes its bands' cell colours itself (0: cell kernel + output pass)
    int block_fuse = 1;       // plan: fused layer1 bottlenecks (block.hip)
    int block32_xd = 2;       //   block32 stage-1 x loads in flight + 1 (register sets: 2, 3, 4)
    int block32_dbg = 0;      //   timing-only (vdt_set_debug, never vd_set_option): skip block32 stages (bits: 1 S1, 2 S2, 4 S3 math, 8 S3 stores, 16 S3 identity / downsample x loads)
    int block32_pipe = 1;     //   block32 (CIN 256): producer / consumer wave groups on consecutive tiles (0: one group)
    int block32_pipe_ds = 1;  //   block32 (layer1.0: CIN 64 + downsample): the same wave groups, bit-identical (0: one group)
    int block_fuse32 = 1;     // plan, fp32 (fp16 pairs): fused layer1 bottlenecks (block32.hip)
    int chain = 2;            // plan: conv3 + next conv1 as one kernel (chain.hip; fp32: chain32.hip: 2 = layer2,
                              //   1 = layer2 + layer3 -- level on the grouped headline, slower per launch)
    int stem_pool = 1;        // plan: stem conv + maxpool (stem.hip)
    int ssh_fuse = 2;         // plan: SSH conv3X3 + conv5X5_1 as one conv (2: and conv5X5_2 + conv7X7_2)
    int plate_s2d = 1;        // plan: YOLO space-to-depth stem input
    int jenc_gpu = 1;         // vd_jpeg_encode: Huffman coding on the device (0: host threads)
    int jdec_gpu = 1;         // vd_jpeg_decode: entropy decode on the device (0: host threads)
    int jdec_sync = 128;      //   states recorded per chunk: passes stop at the previous trajectory (0: off)
    int jdec_chunk = 1024;    //   raw scan bytes per decoding thread (tests force small chunks)
    int jdec_group = 4;       //   resynchronisation passes launched between host convergence checks
    int ssh_side = 0;         // 1: face SSH levels 1-2 (+ heads) on a second stream beside FPN merge / level 0
                              //   (at weight load; measured -0.1 ms/step, but overlapping launches inflate
                              //   the per-launch durations behind `roofline`: off by default)
    int chain_gpw = 1;        // chain32.hip layer2: 16-pixel groups per wave (2: 256-pixel super-groups)
    int det_group = 1;        // plan (fp32): the Detect heads' cv2.i.1 + cv3.i.1 as one grouped 3x3 conv
    int plate_s2d32 = 1;      // fp32 plan: the plate stem on the fp16 space-to-depth canvas (with plate_s2d)
    int face_groups = 2;      // face net as G frame groups on G streams (the tails of one group's launches
                              //   fill with the others'; bit-identical; 0 / 1: one launch over the batch)
    int plate_detect_early = 1; // plan: each YOLO Detect level right after its P level (0: all three at the end)
    int mosaic_early = 1;     // vd_process without MOSAIC_PLATES: the face mosaic runs before the plate branch joins
    int plate_stage = 3;      // plate branch starts after face stage N (0: with the stem; 1-4: after
                              //   layerN; 5: after the whole face net). After layer3 its HBM-bound
                              //   convs overlap the MFMA-bound late face layers: 30.8 -> 30.0 ms/step
    int x6_stream = 1;        // fp32 split: streaming 1x1 kernel for K in {64, 128, 256} (conv_x6_stream.hip)
    int x6_stream_rl = 1;     //   streaming 1x1 with a residual: one input register set refilled per k-step, the
                              //   residual loaded at the top of each pixel group (beside the MFMAs), not in the epilogue
    int x6_stream_silu = 1;   //   fp16 pairs: also SiLU 1x1 convs (YOLO C2f / SPPF) with K in {32..256}
    int x6_stream256 = 2;     //   fp16 pairs, Cout % 256 == 0: 256-channel slices for K = 64 (2: and K = 128;
                              //   each pixel read by half as many workgroups: faces 27.31 -> 26.96 ms/step)
    int x6_small_k = 256;     // fp32 split: K at or below which the small single-stage tile runs
    int x6_small_tiles = 512; //   ... and big-tile grids smaller than this (0 / 0: big tile always)
    int x6_small_k2 = 1 << 20;//   fp16 pairs: K at or below which N <= 64 layers take the small tile
    int x6_bn256 = 1;         // fp16 pairs: 256 x 256 tile for Cout % 256 == 0
    int x6_exact = 1;         // fp16 pairs: one A plane for inputs exact in fp16 (the face stem)
    int x6_mid = 512;         // fp16 pairs: 1x1 Cout-128 convs with K <= this on the 128 x 128 two-stage tile (0: off)
    int x6_mf32 = 0;          // fp16 pairs: 256 x {256,128} tiles on v_mfma_f32_32x32x16_f16 (else 16x16x32)
    int x6_halo = 2;          // fp16 pairs, 3x3 stride-1 convs: input split once per 32-channel chunk
                              //   over the tile's linear halo (conv_x6_halo.hip); 2: three B stages, 1: two
    int x6_halo_narrow = 1;   // ... also for Cout <= 64 (N tiles of 32 / 64)
    int x6_halo_s2 = 1;       // ... also 3x3 stride-2 convs (phase halos; Cout > 32)
    int x6_halo_1b = 1;       // halo tiles with two B stages (wide frames): one barrier per step (0: two)
    int x6_gemm_uni = 2;      // 1x1 GEMM two-stage loop: 2 = the same loads / DMAs every K tile (past the end: the
                              //   last tile again), so the compiler's register waits stay off the next tile, and
                              //   one barrier per K tile; 0 = the general loop (vd_set_option refuses 1)
    int x6_gemm_pf = 1;       // GEMM tiles with wide wave tiles (TN > TM): the same pipelined B-fragment reads
    int x6_halo_pf = 1;       //   halo tiles (128-256 wide): B fragments of block j + 1 read before block j's MFMAs
    int x6_halo_dma = 2;      //   halo tiles: where a K step issues the B DMA two steps ahead (0 after the
                              //   barrier, 1 after the step's MFMAs, 2 one piece between MFMA groups)
    int x6_halo_tr = 2;       // fp32 plan: halo 3x3 tiles with D^T accumulators and the register epilogue
                              //   (1: the 128-256-wide tiles, 2: all; bit-identical)
    int x6_one = 1;           // fp16 pairs, GEMM tiles: 1x1 convs load A at row offset + scalar K offset (no tap stepping)
    int x6_taps = 1;          // fp32 plan: narrow KxK YOLO layers (K <= 288) on the streaming TAPS form
    int x6_gemm1x1 = 1;       // fp16 pairs: GEMM 1x1 convs on the TR tiles (D^T accumulators, register epilogue; 0: off)
    int x6_dbg = 0;           // timing-only (vdt_set_debug / tools/x6bench, never vd_set_option; WRONG results): bit 0 = no
                              //   epilogue; halo tiles: bit 2 = no B DMA past the prologue, 3 = no halo reload, 5 = no
                              //   main-loop barriers
    int face_bands = 1;       // fp32 pairs, ResNet-50: the stem's and layer1's tiles inside the letterbox bands keep
                              //   what an earlier call wrote under the same conditions (0: every tile
                              //   computed in every call; bit-identical)
    int f32_split = 2;        // plan (fp32, at weight load): 2 = operands scaled by powers of two
                              //   and split into fp16 pairs, 3 products on the f16 matrix cores;
                              //   1 = exact 3-term bf16 split, 6 products (conv_x6.hip);
                              //   0 = exact-f32 v_mfma_f32_16x16x4_f32 (conv.hip)
};

// Implicit-GEMM convolution parameters (device side). Activations are NHWC with
// an explicit channel stride (ld) and channel offset (coff) so a conv can read
// a channel slice of a concat buffer and write into one (SSH concat,
// layers.py:64; YOLO C2f/Concat).
struct ConvArgs {
    const void* x;  int xh, xw, ldx, xcoff;     // input  [B][xh][xw][ldx]
    const void* w;                               // packed weights [Npad][Kpad]
    const float* scale; const float* shift;      // BN eval as y = acc*scale + shift (len Npad)
    const void* res; int res_ld, res_coff, res_up;  // residual NHWC; res_up: 1 = nearest 2x source
    int rh, rw;                                  // residual spatial dims
    void* y;  int yh, yw, ldy, ycoff;            // output [B][yh][yw][ldy]
    int B, cin_pad, cout, kpad;                  // cin_pad: channels per tap in the K order
    int kh, kw, stride, pad;
    int M;                                       // B*yh*yw
    int act; float slope; int res_mode; int out_f32;
    int f16;                                     // 16-bit type is fp16 (VD_PREC_FP16), else bf16
    int ntiles_n;                                // ceil(cout / BN)
    // optional second 1x1 conv summed before the activation (bottleneck conv3 +
    // downsample in one pass): y = act(acc*scale + shift + acc2*scale2 + shift2)
    const void* x2; int xh2, xw2, ldx2, xcoff2, stride2;
    const void* w2; const float* scale2; const float* shift2; int cin2_pad, kpad2;
    const VdTune* tune;                          // host-side kernel selection (never read on the device)
    const void* wx3;                             // fp32: split weights (conv_x6.hip: 3 bf16 / 2 fp16 planes), or NULL
    // f32_split = 2 (fp16 pair): per-channel BN scale with the weight rows' 2^-e folded in,
    // the input's running max |x| (device slot, or a static bound when NULL) and the
    // output's slot (atomic max of |y|; NULL: not tracked)
    const float* scale_x;
    int f32_split;                               // the conv's weight format (Conv::split at load)
    const unsigned* xmax; float xbound;
    unsigned* ymax;
    // fp16 pairs, fused downsample (x2): its split weights, rescaled BN scale, input range
    const void* wx3_2; const float* scale2_x;
    const unsigned* x2max; float x2bound;
    int x_exact;                                 // fp16 pairs: input values exact in fp16 (integer canvas)
    // conv_x6 tiles: the schedule selectors of VdTune, filled by vd_launch_conv_x6 (results do not depend on them)
    int one;                                     //   x6_one: 1x1 A loads at row offset + scalar K offset
    int halo_dma;                                //   x6_halo_dma: where a halo step issues the B DMA (0-2)
    int gemm_1b;                                 //   x6_gemm_uni == 2: 1x1 convs on the one-barrier K loop
    int halo_1b;                                 //   x6_halo_1b: two-stage halo tiles with one barrier per step
    int dbg;                                     // timing-only skips (VdTune::x6_dbg bits 0, 2-5; WRONG results; 0 in production)
    int grp_co, grp_ci;                          // grouped conv (fp32 halo tiles): output channels n read input
                                                 //   channels (n / grp_co) * grp_ci + [0, cin); 0: dense
};

// One fused layer1 bottleneck (block.hip): x [B][H][W][cin] -> y [B][H][W][256],
// weights pre-packed by the runtime (Ctx::make_block) from the per-conv bf16 weights.
struct BlockArgs {
    const void* x; void* y;
    int B, H, W, cin, ds;        // ds: identity = bn(downsample(x)) (cin 64), else x (cin 256)
    int tiles_x, tiles_y;        // 16-wide x 8-high output tiles
    const void* w1;              // conv1 MFMA fragments [4 groups of 16 ch][cin/32 k-steps][64 lanes][8]
    const void* w2;              // conv2 fragments [4][18][64][8]
    const void* w3;              // conv3 fragments [8 groups of 32 ch][2 tiles][2 k-steps][64][8]
    const void* wd;              // downsample fragments [8][2][cin/32][64][8] (ds)
    const float* bn;             // s1 t1 s2 t2 (64 each) s3 t3 sd td (256 each)
    unsigned long long* diag;    // optional: per-stage cycle sums of workgroup 0, wave 0 (tools/convbench)
    int mode;                    // experiments (tools/convbench VD_BLOCK_MODE); 0 in production
    int f16;                     // fp16 plan: fp16 operands / activations (else bf16)
};

// Letterbox bands (face_bands.h): the tile rows of one op whose outputs depend on the
// letterbox geometry, the weights and the op's input scale exponents only, and the state that says
// under which of these the rows in the output buffer were last written. on = 0: every tile runs.
constexpr int VD_BAND_FRAMES = 1024;   // frames of one launch with bands on (the kernels' LDS prefix)
struct BandArgs {
    int on;
    int lo, hi;                        // tile rows [0, lo) and [hi, tile rows) are band tiles (lo < hi)
    unsigned epoch;                    // host epoch (nonzero)
    int nchain;                        // input scale exponents in the tag (0: the stem, static bound)
    const unsigned* chain[3];          // max |x| slots of the band ops' inputs up to this op (frame 0 of this call)
    const unsigned long long* tag;     // per frame: the conditions of the band tiles in y (0: none)
    const unsigned* bmax;              // per frame: max |y| over those band tiles
    unsigned* scratch;                 // per frame, zero at the start of the call: max |y| of the band tiles run now
};

// One fused layer1 bottleneck in the fp32 plan (block32.hip): x f32 [B][H][W][cin]
// -> y f32 [B][H][W][256]; weights as fp16 hi / lo planes of the per-conv pair
// packing (row scales folded into the BN scales), per-frame range slots of x / y.
struct Block32Args {
    const void* x; void* y;
    int B, H, W, cin, ds;
    int tiles_x, tiles_y;        // 16-wide x 8-high output tiles
    const void* w1;              // conv1 planes [2][cin/32][64 rows][32] fp16 (LDS image source)
    const void* w2;              // conv2 fragments [4 jn][2 hf][9 taps][2 planes][64 lanes][8] fp16
    const void* w3;              // conv3 fragments [8 waves][2 tiles][2 k-steps][2 planes][64][8] (rows permuted)
    const void* wd;              // downsample fragments, same layout (ds)
    const float* bn;             // s1 h1 s2 h2 (64 each), s3 h3 (256 each), sd hd (256 each, ds)
    const unsigned* xmax;        // x's per-frame max |x| slots (frame 0 of this call)
    unsigned* ymax;              // y's slots (atomic max)
    int xdepth;                  // stage-1 x register sets (option block32_xd: 2, 3, 4)
    int pipe;                    // producer / consumer wave groups on consecutive tiles (option block32_pipe)
    int pipe_ds;                 // ... for cin 64 + downsample (option block32_pipe_ds)
    int dbg;                     // timing-only stage skips (option block32_dbg; wrong results)
    BandArgs band;               // pipelined forms only: letterbox band tiles left alone (on = 0: none)
};

// A bottleneck's conv3 (+ identity, ReLU) and the next bottleneck's conv1 in one
// pass (chain.hip): y = relu(bn3(w3 . t2) + res) [M][512], y2 = relu(bn1'(w1 . y)) [M][128].
struct ChainArgs {
    const void* t2; int ld_t2;            // [M][128] bf16
    const void* res; int ld_res;          // identity [M][512]
    const void* w3; int kpad3;            // conv3 weights [>= 512][kpad3] bf16
    const float* sc3; const float* sh3;   // bn3 folded
    const void* w1; int kpad1;            // next conv1 weights [>= 128][kpad1] bf16
    const float* sc1; const float* sh1;   // next bn1 folded
    void* y; int ld_y;                    // block output [M][512]
    void* y2; int ld_y2;                  // next block's t1 [M][128]
    int M;
    int f16;                              // fp16 plan: fp16 operands / activations (else bf16)
};

// fp32 plan (chain32.hip): layer2 conv3 (+ identity, ReLU) and the next conv1 in one pass,
// fp16-pair weights: y = relu(bn3(w3 . t2) + res) [M][512], y2 = relu(bn1'(w1 . y)) [M][128].
struct Chain32Args {
    const void* t2; int ld_t2;            // [M][128] f32
    const void* res; int ld_res;          // identity [M][512] f32
    const void* w3;                       // conv3 planes [>= 512][4 k-steps][2][32] fp16 (conv_x6 wx3)
    const void* w1;                       // next conv1 planes [>= 128][16][2][32], K permuted per 32-step
    const float* sc3; const float* sh3;   // bn3 (scale times the row's 2^-e)
    const float* sc1; const float* sh1;   // next bn1
    void* y; int ld_y;                    // block output [M][512]
    void* y2; int ld_y2;                  // next block's t1 [M][128]
    int M, B, hw;                         // pixels, frames, pixels per frame
    const unsigned* xmax; float xbound;   // t2's per-frame max |x| slots (frame 0 of this call)
    unsigned* ymax; unsigned* y2max;      // y's / y2's slots (atomic max)
    int gpw;                              // 16-pixel groups per wave (layer2: 1 or 2)
};

// Depthwise 3x3 conv (pad 1) + BN + activation, NHWC (dwconv.hip): MobileNetV1 conv_dw.
struct DwConvArgs {
    const void* x; int xh, xw, ldx, xcoff;
    const void* w;                               // [9 taps][c] (dy-major), compute type
    const float* scale; const float* shift;
    void* y; int yh, yw, ldy, ycoff;
    int B, c, stride, act; float slope;
    unsigned* ymax;                              // fp16-pair plan: per-frame max |y| slots, or NULL
};

// RetinaFace stem conv (space-to-depth form) + maxpool in one kernel (stem.hip):
// x = X' [B][xh][xw][16] -> y = pooled [B][ph][pw][64].
struct StemPoolArgs {
    const void* x; int B, xh, xw;
    void* y; int ph, pw;
    const void* wf;              // MFMA fragments [4 groups of 16 ch, pairs permuted][8 k-steps][64 lanes][8]
                                 //   (fp32 plan: [2 planes: hi, lo] of that, fp16; x = X' in fp16, exact)
    const float* scale; const float* shift;
    unsigned* ymax;              // fp32 plan: per-frame max |y| slots of the pooled map
    int f16;                     // fp16 plan (stem_pool_kernel): fp16 canvas, weights and pooled map
    BandArgs band;               // fp32 plan: letterbox band tiles (6 pool rows each) left alone (on = 0: none)
};

// Device buffers + parameters for one frame batch's detection post-processing.
enum { POST_FACE = 0, POST_YOLO = 1 };
struct PostArgs {
    int mode;                // POST_FACE / POST_YOLO
    const float* heads[3];   // per level NHWC [B][H][W][hstride] f32
    int hstride;             // face: 32 (0..7 bbox, 8..11 cls, 12..31 landm); yolo: 64 DFL | nc cls (padded)
    int lh[3], lw[3];        // level dims
    int loff[3];             // first anchor index per level
    int strides[3];          // yolo: 8/16/32
    const float* anchors;    // face: [A][4] priors
    int A;                   // anchors per frame
    int B;
    int nc;                  // yolo classes
    float conf;
    // weak-detection rescue (include/vdmi.h at vd_rescue): with low_on the candidate test runs at `low`
    // (faces >= low, plates > low), k_all gets the whole keep count and k_count / the caller's arrays the
    // strong prefix (the boxes that pass `conf`); with low_on == 0 nothing below is read
    float low; int low_on;
    int* k_all;              // [B] whole keep list counts (low_on)
    double iou;
    int max_det;             // yolo: 300 (0 = unlimited)
    float max_wh;            // yolo class offset (7680)
    uint64_t* cand_keys;     // [B][A] candidate keys
    int* cand_count;         // [B]
    float4* scratch_box;     // [B][A] decoded box by anchor (candidates only)
    int* scratch_cls;        // [B][A] yolo class by anchor
    float4* scratch_nbox;    // [B][A] NMS boxes for large candidate sets
    float* scratch_area;     // [B][A]
    uint64_t* scratch_keys;  // [B][sort_cap]
    uint8_t* scratch_supp;   // [B][A]
    int sort_cap;            // power of two >= A
    int img_h, img_w;        // source frame size (all frames of a call share it)
    float offx, offy, scx, scy;   // face correction (utils_bbox.py:118-132, float32)
    // tiled face detection (tile_T = 1 + rows * cols > 1; 0: off): net input b is the whole frame
    // when b % tile_T == 0, else a tile of tile_h x tile_w source pixels with its own factors
    int tile_T, tile_h, tile_w;
    float tile_offx, tile_offy, tile_scx, tile_scy;
    int padx, pady; float inv_gain;  // yolo scale_boxes
    int cap;                 // caller's capacity per frame (out_* may all be NULL)
    int kcap;                // complete keep list capacity per frame (>= any keep count)
    int* k_count;            // [B]          complete keep lists (library-owned; the mosaic's input)
    int* k_xyxy;             // [B][kcap][4]
    float* k_xyxy_f;         // [B][kcap][4]
    float* k_score;          // [B][kcap]
    int* k_label;            // [B][kcap]
    int* out_count;          // [B]
    int* out_xyxy;           // [B][cap][4]
    float* out_xyxy_f;       // [B][cap][4]
    float* out_score;        // [B][cap]
    int* out_label;          // [B][cap]
};

enum { LB_COPY = 0, LB_AREA2 = 1, LB_LINEAR = 2 };

struct LetterboxArgs {
    const uint8_t* src; int n, ih, iw; size_t pitch;
    int oh, ow;            // canvas size
    int nh, nw;            // resized size
    int top, left;         // paste offset
    int mode;
    double scale_x, scale_y;   // 1 / inv_scale (resize.cpp)
    float pad_value;       // canvas fill (128 RetinaFace / 114 YOLO)
    float mean[3];         // subtracted per output channel
    float div;             // divisor after mean (1, or 255 for ultralytics' im /= 255)
    int flip;              // 1: output channel c takes source channel 2-c
    void* out; int cpad; int out_f32;
    int out_f16;           // 16-bit canvas in fp16 (VD_PREC_FP16) instead of bf16
    int s2d;               // 1: space-to-depth canvas for the stride-2 stem (bf16, 16 channels):
                           //    out[Y][X][(py*2+px)*4 + c] = canvas[2Y+py-1][2X+px-1][c], 0 off-canvas,
                           //    Y in [0, oh/2], X in [0, ow/2]
    int gx_k, gx_c;        // set by the launcher (pre.hip): gx_k > 0 when the LB_LINEAR column taps are
                           //    an exact gather, source column gx_k * rx + gx_c with weights (1, 0)
    Nv12Src nv;            // nv.on: the frames are NV12 surfaces (nv12.h), converted at the taps
};

// One batch of JPEG frames (jpeg_host.cpp -> jpeg.hip): sparse coefficients per
// block, block order (image, component, block row, block col).
struct JpegArgs {
    int n, h, w, nc, hmax, vmax;
    int bw[3], bh[3], hs[3], vs[3], cblk[3];    // per component: block grid, sampling, first block
    long plane_off[3];
    int blocks_per_image;
    const uint32_t* blk_off;                    // [n * blocks_per_image + 1] into entries
    const uint16_t* quant;                      // [n][3][64] natural order
    const uint32_t* entries;                    // natural index << 16 | int16 quantized value
    uint8_t* planes;                            // [n * blocks_per_image][64] decoded samples
    const int16_t* dense;                       // or (device entropy decode) dense quantized blocks
                                                // [n * blocks_per_image][64] natural order; entries unused
    uint8_t* out; size_t pitch;                 // RGB frames [n][h][pitch]
    int fx[3], fy[3], dw[3], dh[3];             // per component: upsampling factors, downsampled size
                                                // (vd_launch_jpeg fills them)
};

// Device entropy decode (jpeg_dec.hip). JLds: one Huffman table set as the kernels
// hold it in LDS (jpeg_host.cpp build_huff tables): 11-bit lookahead (len << 8 | sym)
// for dc0 dc1 ac0 ac1, the AC fast path (len | run << 8 | (u16)value << 16; run 64 =
// EOB, 16 = ZRL), and the canonical slow path.
struct JLds {
    uint16_t look[4][2048];
    uint32_t fast[2][2048];
    uint32_t fastdc[2][2048];                   // DC code + extra bits in one lookup (len | diff << 16)
    int32_t maxcode[4][18];
    int32_t valoff[4][17];
    uint8_t vals[4][256];
};
struct JdecLaunch {
    int stage;                     // 0 prep, 1 sync pass, 2 scan, 3 write
    int pass, nwg;
    const int* wg_frame; const uint32_t* wg_chunk;   // workgroup -> (frame, first chunk)
    const uint8_t* bytes; const uint32_t* seg_off; const uint32_t* seg_len; const uint32_t* chunk0;
    const uint8_t* tab_of; const JLds* tabs;
    int n, chunk_bytes, bpm;
    int ucomp[6], udc[6], uac[6], ubx[6], uby[6];
    int mcux, total_blocks;
    int cblk[3], bw[3], hs[3], vs[3];
    int blocks_per_image;
    uint32_t* D; uint32_t* S; uint8_t* Su;
    uint32_t* Epos[2]; uint8_t* Eu[2];
    uint32_t* nblk; int* dcs; uint32_t* base; int* dcoff;
    int16_t* dense;
    int* flags;
    int R; uint32_t* Lpos[2]; uint8_t* Lu[2]; int* Ldc[2]; uint8_t* Lcnt[2]; uint8_t* Lsel; uint32_t* own;
};
hipError_t vd_launch_jdec(const JdecLaunch& L, hipStream_t s);

// One batch of RGB frames -> quantized coefficient blocks (jpeg_enc.hip -> jpeg_enc.cpp).
struct JpegEncArgs {
    const uint8_t* src; size_t pitch; int n, h, w;
    int hl, vl;                                 // luma sampling factors (chroma 1x1)
    int bw[3], bh[3];                           // blocks per component (width/height_in_blocks)
    long cblk[3], blocks_per_frame;             // first block of each component within a frame
    const uint16_t* recip; const uint16_t* corr; const uint8_t* shift;   // [2 tables][64], natural order
    int16_t* coef;                              // [n][blocks_per_frame][64] natural order
};

// Device entropy stage (jpeg_enc.hip, after jpeg_fdct_kernel): one thread per
// scan unit (a block in MCU order, dummy blocks included) sizes, then writes, its
// Huffman code; a per-frame scan gives the bit offsets; a stuffing pass emits the
// entropy-coded segment with 0xFF 0x00 and the 1-bit padding.
struct JpegHuffArgs {
    const int16_t* coef; long blocks_per_frame; int n;
    int hl, vl, bw[3], bh[3]; long cblk[3];
    int mcux, units;                            // MCUs per row; scan units per frame
    const uint16_t* code; const uint8_t* size;  // [4][256]: DC luma, DC chroma, AC luma, AC chroma
    unsigned* bits;                             // [n][units] code length, then exclusive bit offset
    unsigned* total;                            // [n] bits per frame
    unsigned* words; long wcap;                 // [n][wcap] MSB-first bit buffer (zeroed)
    uint8_t* seg; long segcap; unsigned* segsize;   // stuffed segments packed frame after frame; lengths
    unsigned* ffcnt; int nchunk;                // [n][nchunk] 0xFF bytes per 4-KB chunk, then output offsets
    unsigned long long* segbase;                // [n + 1] frame offsets in seg (exclusive scan; [n] = total)
};

// Dispatch record: the kernel family that took the calling thread's last conv, written by
// each launcher where its choice is final and read back by the test hook vdt_run_op. Host
// side only (runtime.cpp holds the thread_local): it changes no decision and no kernel
// argument and is never read on the device.
enum VdConvFam {
    VD_FAM_NONE = 0,
    VD_FAM_GEMM,          // conv.hip conv_igemm_kernel: the 16-bit plans' implicit GEMM, the exact-f32 MFMA form
    VD_FAM_STREAM,        // conv1x1.hip streaming 1x1
    VD_FAM_DUAL,          //   ... with the fused second 1x1 conv
    VD_FAM_TAPS,          //   ... streaming taps
    VD_FAM_BIG,           // conv_big.hip phased 256 x 256 tiles
    VD_FAM_X6_TILE,       // conv_x6.hip GEMM tiles (LDS epilogue)
    VD_FAM_X6_TR,         //   ... TR tiles (D^T accumulators, register epilogue)
    VD_FAM_X6_HALO,       // conv_x6_halo.hip 3x3 stride 1 (dense or grouped)
    VD_FAM_X6_HALO_S2,    //   ... stride 2 (phase halos)
    VD_FAM_X6_STREAM,     // conv_x6_stream.hip streaming 1x1 slices
    VD_FAM_X6_TAPS,       //   ... streaming taps
    VD_FAM_X6_DUAL,       //   ... with the fused second 1x1 conv
    VD_FAM_COUNT
};
static inline const char* vd_conv_fam_name(int f) {
    static const char* const names[VD_FAM_COUNT] = {"", "gemm", "stream", "dual", "taps", "conv_big", "x6_tile", "x6_tr",
                                                    "x6_halo", "x6_halo_s2", "x6_stream", "x6_taps", "x6_dual"};
    return f >= 0 && f < VD_FAM_COUNT ? names[f] : "";
}
void vd_conv_fam_set(int fam);
int vd_conv_fam_get();

// ---- kernel launchers (one translation unit each) ----
hipError_t vd_launch_jpeg_fdct(const JpegEncArgs& a, hipStream_t s);
hipError_t vd_launch_jpeg_huff(const JpegHuffArgs& a, hipStream_t s);          // codes -> words, bit totals
hipError_t vd_launch_jpeg_stuff(const JpegHuffArgs& a, hipStream_t s);         // words -> packed segments
hipError_t vd_launch_amax_merge(unsigned* dst, const unsigned* src, int n, hipStream_t s);
bool vd_conv1x1_stream_ok(const ConvArgs& a);
bool vd_conv_big_ok(const ConvArgs& a);
hipError_t vd_launch_conv_big(const ConvArgs& a, hipStream_t s);
hipError_t vd_launch_conv1x1_stream(const ConvArgs& a, hipStream_t s);
bool vd_conv_taps_ok(const ConvArgs& a);
bool vd_conv1x1_dual_ok(const ConvArgs& a);
hipError_t vd_launch_conv_taps(const ConvArgs& a, hipStream_t s);
hipError_t vd_launch_conv(const ConvArgs& a, bool f32, hipStream_t s);
bool vd_conv_x6_ok(const ConvArgs& a);
bool vd_conv1x1_x6_dual_ok(const ConvArgs& a);   // conv_x6_stream.hip; launched through vd_launch_conv_x6 (a.x2)
hipError_t vd_launch_conv_x6(const ConvArgs& a, hipStream_t s);   // a.tune set; the family's own entries: conv_x6.h
void vd_pack_x6(const float* w, int npad, int kpad, uint16_t* out);   // host: f32 [npad][kpad] -> split planes
void vd_pack_x3h(const float* w, int npad, int kpad, uint16_t* out, float* row_inv);   // ... fp16 pairs
bool vd_block_ok(int cin, bool ds, int h, int w);
bool vd_block32_ok(int cin, bool ds, int h, int w);
hipError_t vd_launch_block32(const Block32Args& a, hipStream_t s);
// After the last band op of a forward (bands.hip): per op and frame of the call, a tag that differs
// from the current conditions is replaced, with the band maximum the call's kernels left in scratch.
struct BandPublishArgs {
    BandArgs op[4];                    // as the kernels got them (on = 0: op without band tiles)
    unsigned long long* tag[4];        // the writable tags / maxima behind op[k].tag / op[k].bmax
    unsigned* bmax[4];
    unsigned* stats;                   // [4][2] per op: frames that matched, frames that did not
    int n;
};
hipError_t vd_launch_band_publish(const BandPublishArgs& a, hipStream_t s);
bool vd_stem_pool_ok(int xh, int xw, int ph, int pw);
hipError_t vd_launch_dwconv(const DwConvArgs& a, bool f32, bool f16, hipStream_t s);
hipError_t vd_launch_stem_pool(const StemPoolArgs& a, hipStream_t s);
hipError_t vd_launch_stem_pool32(const StemPoolArgs& a, hipStream_t s);   // fp16-pair plan, f32 pooled map
hipError_t vd_launch_block(const BlockArgs& a, hipStream_t s);
bool vd_chain_ok(int cmid, int cout, int kpad3, int kpad1, int ld_t2, int ld_res, int ld_y, int ld_y2, long M);
hipError_t vd_launch_chain(const ChainArgs& a, hipStream_t s);
bool vd_chain32_ok(int cmid, int cout, int kpad3, int kpad1, int ld_t2, int ld_res, int ld_y, int ld_y2, long M,
                   int frames);
hipError_t vd_launch_chain32(const Chain32Args& a, hipStream_t s);
hipError_t vd_launch_letterbox(const LetterboxArgs& a, hipStream_t s);
bool vd_letterbox_pair_ok(const LetterboxArgs& a, const LetterboxArgs& b);
hipError_t vd_launch_letterbox_pair(const LetterboxArgs& a, const LetterboxArgs& b, hipStream_t s);
hipError_t vd_launch_maxpool(bool f32, bool f16, const void* x, int n, int xh, int xw, int ldx, int xcoff,
                             void* y, int yh, int yw, int ldy, int ycoff, int c, int k, int st, int p,
                             hipStream_t s);
hipError_t vd_launch_upsample2x(bool f32, const void* x, int n, int xh, int xw, int ldx, int xcoff,
                                void* y, int ldy, int ycoff, int c, hipStream_t s);
hipError_t vd_launch_post(const PostArgs& p, hipStream_t s);
hipError_t vd_launch_jpeg(const JpegArgs& a, hipStream_t s);
hipError_t vd_launch_mosaic(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
                            const int* cnt0, const int* xy0, int cap0,
                            const int* cnt1, const int* xy1, int cap1, int level, void* table,
                            int stages, int map_on, int cell_blocks, hipStream_t s, int cells = 0);   // stages: 1 = cell table, 2 = output pass, 4 = copy; cells: vd_cells (0 = off)
size_t vd_mosaic_table_bytes(int n, int tcap);
// Pixelation of 4:2:0 frames (nv12.hip; include/vdmi.h at vd_nv12 and vd_yuv420): one launch, every
// plane. Luma at in / out, U at + *_uv bytes, V at + *_v, chroma rows of *_cp bytes, samples *_step
// apart (NV12: *_v = *_uv + 1, *_cp = *_pitch, *_step = 2), frame f at + f * *_stride; lists as
// vd_launch_mosaic takes them (none: the launch is the copy in -> out between the two layouts).
struct Nv12MosaicArgs {
    const uint8_t* in; uint8_t* out; int n, h, w;
    size_t in_pitch, in_uv, in_stride, out_pitch, out_uv, out_stride;
    size_t in_v, in_cp, out_v, out_cp;
    int in_step, out_step;
    void set(const Yuv420Dev& i, const Yuv420Dev& o) {
        in = i.base; in_pitch = i.pitch; in_uv = i.u; in_v = i.v; in_cp = i.cpitch; in_stride = i.stride; in_step = i.step;
        out = o.base; out_pitch = o.pitch; out_uv = o.u; out_v = o.v; out_cp = o.cpitch; out_stride = o.stride; out_step = o.step;
    }
    Yuv420Dev src() const { return Yuv420Dev{(uint8_t*)in, in_pitch, in_uv, in_v, in_cp, in_stride, in_step}; }
    Yuv420Dev dst() const { return Yuv420Dev{out, out_pitch, out_uv, out_v, out_cp, out_stride, out_step}; }
    bool nv12() const { return src().nv12() && dst().nv12(); }   // the NV12-only kernels serve the call
    const int* cnt0; const int* xy0; int cap0;
    const int* cnt1; const int* xy1; int cap1;
    int level, cells;
};
// depth != 0: both sides hold 16-bit words (include/vdmi.h at vd_yuv420_16) -- the sizes above stay in
// bytes, the steps in samples -- and the launch is the kernel for words (a copy needs no more than that)
hipError_t vd_launch_mosaic_nv12(const Nv12MosaicArgs& a, hipStream_t s, int depth = 0);
// The look-ahead ring push of NV12 surfaces (nv12.hip): [0, w) of every row of both planes of n
// surfaces, src layout -> dst layout, one launch. No alignment is assumed of either layout.
struct Nv12PackArgs {
    const uint8_t* src; uint8_t* dst; int n, h, w;
    size_t src_pitch, src_uv, src_stride, dst_pitch, dst_uv, dst_stride;
};
hipError_t vd_launch_nv12_pack(const Nv12PackArgs& a, hipStream_t s);
// The same push from any layout of vd_yuv420 / vd_yuv420_16 (src.depth != 0: 16-bit words, copied whole)
// into the ring's layout: `ring` is interleaved, U first, of src's sample size. One launch; an NV12
// source runs the kernel of vd_launch_nv12_pack. Nothing is assumed of src beyond its descriptor's
// checks; of ring, that its pairs are aligned to their size.
hipError_t vd_launch_yuv420_pack(const Yuv420Dev& src, const Yuv420Dev& ring, int n, int h, int w, hipStream_t s);
// Box-scaled strength (include/vdmi.h at vd_cells): the cell level L of a box of unclipped size
// W x H under the base level and the cells setting. cells == 0 or an empty box: the base level;
// otherwise max(level, min(32768, ceil(max(W, H) / cells))). The one routine of the kernels
// (mosaic.hip, smooth.hip) and of the host call vd_cell_level.
__host__ __device__ inline int vd_cell_level_hd(long long W, long long H, int level, int cells) {
    if (cells == 0 || W <= 0 || H <= 0) return level;
    const long long m = W > H ? W : H;
    // int32 coordinates: m < 2^32. Past 32768 * cells the clamp binds, below it 32 bits do
    const int q = m > 32768LL * cells ? 32768 : (int)(((unsigned)m + (unsigned)cells - 1u) / (unsigned)cells);
    return q > level ? q : level;
}
// Scaled smooth blur of box lists (smooth.hip). stage 0: the copy in -> out; stage 1: the box
// pass (reads `in`, writes the boxes' pixels of `out`; after stage 0 on the same stream).
// h, w <= 32768, 1 <= level <= 32768, cells in [VD_CELLS_MIN, VD_CELLS_MAX].
hipError_t vd_launch_smooth(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
                            const int* cnt0, const int* xy0, int cap0,
                            const int* cnt1, const int* xy1, int cap1, int level, int cells, int stage,
                            hipStream_t s);
// ... of NV12 frames, both planes (smooth.hip; include/vdmi.h at vd_nv12): stage 0 copies [0, w) of
// every row of both planes, stage 1 is the box pass of both planes in one launch. Even h, w <= 32768.
// depth != 0: 16-bit words whose value is (word >> shift) & (2^depth - 1), depth <= 12
hipError_t vd_launch_smooth_nv12(const Nv12MosaicArgs& a, int stage, hipStream_t s, int depth = 0, int shift = 0);
size_t vd_smooth_lds_bytes(int cells);   // dynamic LDS of either box pass (RGB cells^2 * 3, chroma (cells + 1)^2 * 2 sums)
// Gaussian blur of box lists (blur.hip): plan + band pass + dependent-box pass on `s`.
// q: the ksize Q20 weights of vd_blur_weights; table: vd_blur_table_bytes(n, h, pitch, tcap) bytes.
hipError_t vd_launch_blur(const uint8_t* in, uint8_t* out, int n, int h, int w, size_t pitch,
                          const int* cnt0, const int* xy0, int cap0,
                          const int* cnt1, const int* xy1, int cap1, int ksize, const uint32_t* q,
                          void* table, hipStream_t s);
size_t vd_blur_table_bytes(int n, int h, size_t pitch, int tcap);
int vd_blur_weights(int ksize, float sigma, uint32_t* q);   // host; 0, or -1 for a refused ksize / sigma

// Box hold (hold.hip): frame f's blur list B = D ++ H in merged rows, and the next history.
// Lists 0 / 1 as the mosaic takes them (list 1 optional); xy pointers 16-B aligned.
struct HoldArgs {
    int n, h, w, K, P;                               // frames, frame size, hold_frames, hold_iou_pct
    int motion;                                      // vd_hold_motion mode; history depth = K + motion slots
    const int* cnt0; const int* xy0; int cap0;       // this call's D lists: list 0 (faces)
    const int* cnt1; const int* xy1; int cap1;       //   list 1 (plates, optional)
    const int* hist_cnt; const int* hist_xy;         // history read: [depth], [depth][hcap][4] (hold_state.h)
    int* next_cnt; int* next_xy;                     // history written: the other buffer
    int hcap, hn;                                    // history row capacity (>= cap0 + cap1), valid slots
    int* m_xy; int* m_age; int* m_count; int* m_own; // merged rows [n][mcap][4], ages [n][mcap], |B| [n], |D| [n]
    int mcap;                                        // (K + 1) * hcap: D plus K complete older lists always fit
};
hipError_t vd_launch_hold(const HoldArgs& a, hipStream_t s);
// Rows of merged lists into caller-shaped arrays [n][cap] (count complete, arrays truncated at cap,
// scalar stores: no alignment assumed); held_only: H alone (skip each row's own |D| boxes).
hipError_t vd_launch_hold_gather(const HoldArgs& a, int n, int held_only, int* out_count, int* out_xyxy,
                                 int* out_label, int cap, hipStream_t s);

// Weak-detection rescue (rescue.hip; include/vdmi.h at vd_rescue): E = D ++ R in merged rows with `since`,
// and the next history. Lists 0 / 1 as the mosaic takes them (list 1 optional); xy pointers 16-B aligned.
// split == 0: the weak boxes of list i are its row's entries [cnt_i, all_i) (all_i NULL: none);
// split == 1: list 0 holds the strong boxes and (wcnt, wxy, wcap) the weak ones (vd_rescue_lists).
#define VD_RESCUE_LDS_BOXES 2048                     // clipped reference boxes a workgroup stages in LDS
struct RescueArgs {
    int n, h, w, W, P, S;                            // frames, frame size, window, hold_iou_pct, span
    int split;
    const int* cnt0; const int* all0; const int* xy0; int cap0;
    const int* cnt1; const int* all1; const int* xy1; int cap1;
    const int* wcnt; const int* wxy; int wcap;
    const int* hist_cnt; const int* hist_xy; const int* hist_since;   // history read: [W], [W][hcap][4], [W][hcap]
    int* next_cnt; int* next_xy; int* next_since;    // history written: the other buffer
    int hcap, hn;                                    // history row capacity (>= ecap), valid slots
    int* e_xy; int* e_since; int* e_count; int* e_own; int* e_nr0;   // E rows [n][ecap][4], since [n][ecap], |E|, |D|,
    int ecap;                                        //   rescued boxes of list 0 [n]; ecap >= every |D| + |W|
    int* w_since; int wtot;                          // per weak box (list 0's, then list 1's): since, 0 = not rescued
};
hipError_t vd_launch_rescue(const RescueArgs& a, hipStream_t s);
// Weak or rescued boxes of one list into caller-shaped arrays [n][cap] (count complete, arrays cut at cap,
// scalar stores). which 1: the weak tail [cnt, all) of the keep rows as stored; which 0: its rescued boxes
// (w_since row entries [woff, woff + weak count) > 0) in order, label = since.
struct RescueReadArgs {
    int which, list;                                 // list 1: the weak index starts behind list 0's weak boxes
    const int* cnt; const int* all; int kcap;        // the list's keep rows
    const int* xy; const float* xy_f; const float* score; const int* label;
    const int* cnt_o; const int* all_o; int kcap_o;  // the other list (list 1's offset), or NULL
    const int* w_since; int wtot;
    int cap; int* out_count; int* out_xyxy; float* out_xyxy_f; float* out_score; int* out_label;
};
hipError_t vd_launch_rescue_read(const RescueReadArgs& a, int n, hipStream_t s);

// Look-ahead hold (lead.hip): the emitted frames' blur lists B = D ++ H ++ A in merged rows, and
// the next pending ring (lead_state.h: window W = ring ++ call). Lists 0 / 1 as the mosaic takes
// them (list 1 optional); xy pointers 16-B aligned.
// A ring buffer, in ints: D counts [slots], D ++ H counts [slots], |D| [slots], padded to
// VD_LEAD_RING_HEAD; then D lists [slots][hcap][4], D ++ H rows [slots][rcap][4], ages [slots][rcap].
#define VD_LEAD_RING_HEAD 32
struct LeadArgs {
    int n, m, pend, keep;                            // frames pushed, emitted, pending before / after (m + keep = pend + n)
    int h, w, J, P, motion;                          // frame size, lead frames, hold_iou_pct, vd_lead motion mode
    const int* cnt0; const int* xy0; int cap0;       // this call's D lists: list 0 (faces)
    const int* cnt1; const int* xy1; int cap1;       //   list 1 (plates, optional)
    const int* dh_xy; const int* dh_age;             // this call's D ++ H rows (the hold launch's merged rows);
    const int* dh_count; const int* dh_own; int dh_cap;   //   dh_xy null without hold: the D lists are the rows
    const int* ring; int* next;                      // pending ring read / written (the other buffer)
    int hcap, rcap, slots;                           // D capacity (>= cap0 + cap1), D ++ H capacity, slots = delay
    int* m_xy; int* m_age; int* m_count;             // merged rows [m][mcap][4], labels [m][mcap] (0, +a, -a), |B| [m]
    int* m_own; int* m_dh;                           // |D| [m], |D ++ H| [m]
    int mcap;                                        // rcap + J * hcap: the row plus J complete newer lists always fit
};
size_t vd_lead_ring_ints(int slots, int hcap, int rcap);
hipError_t vd_launch_lead(const LeadArgs& a, hipStream_t s);

// Mask shaping (mask.hip). Grow: lists 0 / 1 as the mosaic takes them (list 1 optional, scalar
// reads: no alignment assumed) -> merged rows of grown boxes. Restore (VD_MASK_ELLIPSE, after the
// rectangular pass on the same stream): pixels of the rows' clipped boxes outside every ellipse
// are copied in -> out.
struct MaskArgs {
    const uint8_t* in; uint8_t* out; int n, h, w; size_t pitch;   // restore only
    const int* cnt0; const int* xy0; int cap0;       // grow only: list 0 (faces)
    const int* cnt1; const int* xy1; int cap1;       //   list 1 (plates, optional)
    int g;                                           // grow percentage in [0, VD_MASK_GROW_MAX]
    int zero_tail;                                   // grow: entries past the count are zeroed (vd_mask_boxes)
    int* m_cnt; int* m_xy;                           // merged rows: counts [n], boxes [n][mcap][4], 16-B aligned
    int mcap;                                        // row capacity >= cap0 + cap1
};
hipError_t vd_launch_mask_grow(const MaskArgs& a, hipStream_t s);
hipError_t vd_launch_mask_restore(const MaskArgs& a, hipStream_t s);
// Restore on NV12 frames (include/vdmi.h at vd_nv12, "ellipse"), after the rectangular NV12 pass on the
// same stream: luma bytes of the rows' clipped boxes outside every ellipse, and chroma pairs of
// their chroma rectangles none of whose four luma pixels lies in an ellipse, are copied in -> out.
struct MaskNv12Args {
    const uint8_t* in; uint8_t* out; int n, h, w;
    size_t in_pitch, in_uv, in_stride, out_pitch, out_uv, out_stride;   // U at + *_uv, V at + *_v, as Nv12MosaicArgs
    size_t in_v, in_cp, out_v, out_cp;
    int in_step, out_step;
    const int* m_cnt; const int* m_xy; int mcap;     // the grown merged rows (MaskArgs)
};
// es: bytes per sample -- 1, or 2 for surfaces of 16-bit words (vd_yuv420_16: whole words are copied)
hipError_t vd_launch_mask_restore_nv12(const MaskNv12Args& a, hipStream_t s, int es = 1);

// Tiled face detection (include/vdmi.h at vd_tiles). T = 1 + rows * cols net inputs per frame:
// input 0 the whole frame, input 1 + r * cols + c tile (r, c); every tile is tw x th pixels.
#ifndef VD_TILES_MAX
#define VD_TILES_MAX 4   // include/vdmi.h: rows, cols in [1, VD_TILES_MAX]
#endif
constexpr int VD_TILE_INPUTS_MAX = 1 + VD_TILES_MAX * VD_TILES_MAX;
struct TileGrid {
    int T, th, tw;
    int x0[VD_TILE_INPUTS_MAX], y0[VD_TILE_INPUTS_MAX];   // origin of input t in the frame ([0] = 0)
};
// host, integers: xywh[1 + rows * cols][4] of an h x w frame; 0, or -1 outside the ranges
int vd_tile_rects_host(int h, int w, int rows, int cols, int overlap_pct, int32_t* xywh, int* count);
// The n * T canvases of n frames in one launch (pre.hip): canvas f * T + t is what
// vd_launch_letterbox writes for a frame holding input t's rectangle. `whole` / `tile`: the
// letterbox geometry of the frame / of a tile as a frame of its own (src, n, pitch, out from
// `whole`; both of one canvas form).
hipError_t vd_launch_letterbox_tiles(const LetterboxArgs& whole, const LetterboxArgs& tile, const TileGrid& g,
                                     hipStream_t s);
// The tile canvases alone (tiled plate detection: the whole-frame canvas can differ in size, so it
// is written by vd_launch_letterbox): canvas f * (T - 1) + (t - 1) is frame f's tile t, n frames of
// fh x fw pixels at tile.src / tile.pitch; `tile`: the geometry of a tile as a frame of its own.
hipError_t vd_launch_letterbox_tile_inputs(const LetterboxArgs& tile, const TileGrid& g, int n, int fh, int fw,
                                           hipStream_t s);
// Cross-tile merge (tiles.hip): per frame, the T keep lists -> one list in merged rows.
struct TileMergeArgs {
    int n; TileGrid g;
    int A;                                           // the net's anchor count: label = t * A + label_in
    double iou;
    const int* cnt; const float* xyxy_f; const float* score; const int* label;   // [n * T] rows of icap (label optional)
    int icap;
    uint64_t* s_keys; float4* s_box; float* s_area; uint8_t* s_supp;   // per-frame spill scratch: [n][sort_cap], [n][mcap] x 3
    int sort_cap;                                    // power of two >= mcap
    int mcap;                                        // merged row capacity >= T * icap
    int* m_count; int* m_xyxy; float* m_xyxy_f; float* m_score; int* m_label;   // merged rows [n][mcap]
    int cap;                                         // caller's capacity per frame (out_* may all be NULL)
    int* out_count; int* out_xyxy; float* out_xyxy_f; float* out_score; int* out_label;
    // tiled plate detection (include/vdmi.h at vd_tiles_nets): the class-aware form. label_in is the
    // box's class, a kept box suppresses boxes of its own class only, label = the class (A unused)
    int plate;
    int split;                                       // plate: frame f's input 0 at row f, input t > 0 at row
                                                     //   n + f * (T - 1) + (t - 1) (two forwards); 0: row f * T + t
    int* s_cls;                                      // plate: spill scratch [n][mcap]
    // rescue on a tiled net (include/vdmi.h at vd_rescue_tiles): the input lists are the lists at `low`, the
    // merged rows hold the whole merged list and m_all its count; m_count / out_count get the length of the
    // strong prefix (score >= thr, plates score > thr) and the caller's out_* arrays the strong boxes only.
    // low_on == 0: nothing below is read (appended last: the fields above keep their offsets)
    int low_on; float thr;
    int* m_all;                                      // [n] whole merged counts (low_on)
};
hipError_t vd_launch_tiles_merge(const TileMergeArgs& a, hipStream_t s);

#define VD_CHECK_HIP(expr)                                                   \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            vd_set_error(VD_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__,      \
                         #expr, hipGetErrorString(_e));                        \
            return VD_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

int vd_set_error(int code, const char* fmt, ...);
