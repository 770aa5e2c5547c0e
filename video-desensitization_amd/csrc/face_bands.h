// face_bands.h — which output rows of the face stem and layer1 depend on the letterbox bands
// only (pure host arithmetic).
//
// A frame letterboxed into the canvas with left = 0 leaves canvas rows [0, top) and
// [top + nh, canvas_h) at the pad colour minus the mean. An output row of a k x k, stride s,
// pad p step reads input rows s y - p .. s y - p + k - 1 clipped to the map; it is a band row when
// all of them are band rows of its input (of the top band, or of the bottom band: the two differ
// at the map's edges, so a row never mixes them). Band rows hold values that depend on the
// weights, the geometry and the op's operand scales, not on the frame.
#pragma once

struct BandRows {   // rows [0, top_end) and [bot_begin, h) of an h-row map are band rows
    int top_end, bot_begin, h;
};

// one k x k, stride s, pad p step onto a map of out_h rows
static inline BandRows vd_band_step(BandRows in, int out_h, int k, int s, int p) {
    BandRows o{0, out_h, out_h};
    for (int y = 0; y < out_h; ++y) {             // leading rows whose last input row is a top band row
        const int last = s * y - p + k - 1 < in.h - 1 ? s * y - p + k - 1 : in.h - 1;
        if (last >= in.top_end) break;
        o.top_end = y + 1;
    }
    for (int y = out_h - 1; y >= o.top_end; --y) {   // trailing rows whose first input row is a bottom band row
        const int first = s * y - p > 0 ? s * y - p : 0;
        if (first < in.bot_begin) break;
        o.bot_begin = y;
    }
    return o;
}

enum { VD_BAND_OPS = 4 };   // the fused stem + pool, layer1.0, layer1.1, layer1.2

struct FaceBandPlan {
    BandRows rows[VD_BAND_OPS];                   // band rows of each op's output map
    int tile_rows[VD_BAND_OPS];                   // tile rows of the op (6 pool rows in the stem, 8 rows in block32)
    int lo[VD_BAND_OPS], hi[VD_BAND_OPS];         // tile rows [0, lo) and [hi, tile_rows) hold band rows only
};

// The ResNet-50 face plan on a canvas of canvas_h rows (a multiple of 4) whose image rows are
// [top, top + nh). Bands that are columns (left != 0) or absent give lo = 0, hi = tile_rows: no band tiles.
static inline FaceBandPlan vd_face_band_plan(int canvas_h, int top, int nh, int left) {
    FaceBandPlan P{};
    BandRows r{top, top + nh, canvas_h};
    if (left != 0 || nh <= 0 || top < 0 || top + nh > canvas_h) r = BandRows{0, canvas_h, canvas_h};
    r = vd_band_step(r, canvas_h / 2, 7, 2, 3);   // conv1 7x7 / 2, pad 3
    r = vd_band_step(r, canvas_h / 4, 3, 2, 1);   // maxpool 3x3 / 2, pad 1
    for (int k = 0; k < VD_BAND_OPS; ++k) {
        if (k) r = vd_band_step(r, r.h, 3, 1, 1); // the bottleneck's 3x3, pad 1 (its 1x1 convs keep rows)
        const int th = k ? 8 : 6;
        P.rows[k] = r;
        P.tile_rows[k] = (r.h + th - 1) / th;
        P.lo[k] = r.top_end / th;
        P.hi[k] = (r.bot_begin + th - 1) / th;
        if (P.hi[k] > P.tile_rows[k]) P.hi[k] = P.tile_rows[k];
        if (P.lo[k] >= P.hi[k]) { P.lo[k] = 0; P.hi[k] = P.tile_rows[k]; }   // no image tile row left: not a case to save on
    }
    return P;
}
