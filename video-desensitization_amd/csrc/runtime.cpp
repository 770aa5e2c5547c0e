// runtime.cpp — libvdmi.so: context, weights, network plans and their execution, and the
// context entries of the C-ABI (frames.cpp, process.cpp, track.cpp and testhooks.cpp hold the rest).
//
// Host side of the MI355X detect-and-blur path. One vd_ctx = one GPU + one HIP
// stream + device-resident weights and workspace sized for cfg.max_batch
// frames (replaces the reference's nn.DataParallel replicate-per-forward,
// detect_face/face.py:55-56: weights are uploaded once, workspace is
// allocated once, nothing is allocated on the per-batch path).
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

static thread_local std::string g_err;

int vd_set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// the dispatch record (vd_common.h VdConvFam)
static thread_local int g_conv_fam = VD_FAM_NONE;
void vd_conv_fam_set(int fam) { g_conv_fam = fam; }
int vd_conv_fam_get() { return g_conv_fam; }

// ----------------------------------------------------------------------------
// weights container
// ----------------------------------------------------------------------------
int vd_parse_vdw1(const void* blob, size_t bytes, WMap& out) {
    const uint8_t* p = (const uint8_t*)blob;
    const uint8_t* end = p + bytes;
    auto need = [&](size_t k) { return (size_t)(end - p) >= k; };
    if (!need(8) || memcmp(p, "VDW1", 4) != 0) return vd_set_error(VD_ERR_WEIGHTS, "weights: bad magic");
    uint32_t count;
    memcpy(&count, p + 4, 4);
    p += 8;
    for (uint32_t i = 0; i < count; ++i) {
        if (!need(2)) return vd_set_error(VD_ERR_WEIGHTS, "weights: truncated header %u", i);
        uint16_t nl;
        memcpy(&nl, p, 2);
        p += 2;
        if (!need(nl + 2)) return vd_set_error(VD_ERR_WEIGHTS, "weights: truncated name %u", i);
        std::string name((const char*)p, nl);
        p += nl;
        uint8_t dtype = p[0], ndim = p[1];
        p += 2;
        if (dtype != 0 || ndim > 8 || !need(4u * ndim))
            return vd_set_error(VD_ERR_WEIGHTS, "weights: bad tensor header for %s", name.c_str());
        HT t;
        size_t numel = 1;
        for (int d = 0; d < ndim; ++d) {
            uint32_t v;
            memcpy(&v, p, 4);
            p += 4;
            t.shape.push_back((int)v);
            numel *= v;
        }
        if (!need(numel * 4)) return vd_set_error(VD_ERR_WEIGHTS, "weights: truncated data for %s", name.c_str());
        t.data.resize(numel);
        memcpy(t.data.data(), p, numel * 4);
        p += numel * 4;
        out[name] = std::move(t);
    }
    return VD_OK;
}

// ----------------------------------------------------------------------------
// device memory helpers
// ----------------------------------------------------------------------------
int Ctx::dalloc(void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return vd_set_error(VD_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    allocs.push_back(*p);
    return VD_OK;
}

int Ctx::act(Act& a, int h, int w, int c, bool f32out, bool half) {
    a.h = h; a.w = w; a.c = c;
    a.f32 = !half && (f32out || f32);
    size_t bytes = (size_t)cfg.max_batch * h * w * c * (a.f32 ? 4 : 2);
    int rc = dalloc(&a.p, bytes);
    if (rc) return rc;
    hipMemset(a.p, 0, bytes);
    a.amax = nullptr;
    a.bound = 0.f;
    if (f32 && tune.f32_split == 2) {
        if (!amax_pool && (rc = dalloc((void**)&amax_pool, 2 * amax_region_bytes()))) return rc;
        if (amax_next[amax_owner] >= kAmaxActs) return vd_set_error(VD_ERR_NOMEM, "activation range slots exhausted");
        a.amax = amax_region(amax_owner) + (size_t)amax_next[amax_owner]++ * cfg.max_batch;
    }
    return VD_OK;
}

int Ctx::amax_begin(int owner) {
    amax_owner = owner;
    amax_next[owner] = 0;
    return VD_OK;
}

int Ctx::ensure_pinned(void** p, size_t* have, size_t need) {
    if (*have >= need) return VD_OK;
    if (*p) { (void)hipEventSynchronize(jpeg_ev); hipHostFree(*p); }
    *p = nullptr;
    *have = 0;
    need += need / 4;                             // grow with headroom: batches vary in size
    hipError_t e = hipHostMalloc(p, need, hipHostMallocDefault);
    if (e != hipSuccess) return vd_set_error(VD_ERR_NOMEM, "hipHostMalloc(%zu) failed", need);
    *have = need;
    return VD_OK;
}

int Ctx::ensure_staging(void** p, size_t* have, size_t need) {
    if (*have >= need) return VD_OK;
    if (*p) hipFree(*p);
    *p = nullptr;
    *have = 0;
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) return vd_set_error(VD_ERR_NOMEM, "hipMalloc(%zu) failed", need);
    *have = need;
    return VD_OK;
}

// ----------------------------------------------------------------------------
// conv construction: OIHW f32 -> packed [npad][kpad] in the compute type with
// k = (kh*KW + kw)*cin_pad + c; BN(eval) -> per-channel scale/shift.
// ----------------------------------------------------------------------------
int Ctx::upload_conv(Conv& cv, const std::vector<float>& w_oihw, const std::vector<float>& scale,
                     const std::vector<float>& shift) {
    const int vec = f32 ? 4 : 8;
    const int bke = 8 * vec;
    cv.cin_pad = (cv.cin + vec - 1) / vec * vec;
    cv.npad = (cv.cout + 127) / 128 * 128;
    const int K = cv.kh * cv.kw * cv.cin_pad;
    cv.kpad = (K + bke - 1) / bke * bke;
    std::vector<float> packed((size_t)cv.npad * cv.kpad, 0.f);
    for (int n = 0; n < cv.cout; ++n)
        for (int c = 0; c < cv.cin; ++c)
            for (int y = 0; y < cv.kh; ++y)
                for (int x = 0; x < cv.kw; ++x)
                    packed[(size_t)n * cv.kpad + (y * cv.kw + x) * cv.cin_pad + c] =
                        w_oihw[(((size_t)n * cv.cin + c) * cv.kh + y) * cv.kw + x];
    int rc;
    if (f32) {
        rc = dalloc(&cv.w, packed.size() * 4);
        if (rc) return rc;
        VD_CHECK_HIP(hipMemcpy(cv.w, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        if (tune.f32_split == 2) {   // scaled fp16 pairs (conv_x6.hip, 3 products)
            std::vector<uint16_t> sp(packed.size() * 2);
            std::vector<float> row_inv(cv.npad), sx(cv.npad, 0.f);
            vd_pack_x3h(packed.data(), cv.npad, cv.kpad, sp.data(), row_inv.data());
            for (int n = 0; n < cv.cout; ++n) sx[n] = scale[n] * row_inv[n];
            if ((rc = dalloc(&cv.wx3, sp.size() * 2)) || (rc = dalloc((void**)&cv.scale_x, cv.npad * 4))) return rc;
            VD_CHECK_HIP(hipMemcpy(cv.wx3, sp.data(), sp.size() * 2, hipMemcpyHostToDevice));
            VD_CHECK_HIP(hipMemcpy(cv.scale_x, sx.data(), cv.npad * 4, hipMemcpyHostToDevice));
            cv.split = 2;
        } else if (tune.f32_split) {   // the same weights as three exact bf16 planes for conv_x6.hip
            std::vector<uint16_t> sp(packed.size() * 3);
            vd_pack_x6(packed.data(), cv.npad, cv.kpad, sp.data());
            if ((rc = dalloc(&cv.wx3, sp.size() * 2))) return rc;
            VD_CHECK_HIP(hipMemcpy(cv.wx3, sp.data(), sp.size() * 2, hipMemcpyHostToDevice));
            cv.split = 1;
        }
    } else {
        std::vector<uint16_t> h(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) h[i] = to_half(f16, packed[i]);
        rc = dalloc(&cv.w, h.size() * 2);
        if (rc) return rc;
        VD_CHECK_HIP(hipMemcpy(cv.w, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    std::vector<float> sc(cv.npad, 0.f), sh(cv.npad, 0.f);
    for (int n = 0; n < cv.cout; ++n) { sc[n] = scale[n]; sh[n] = shift[n]; }
    rc = dalloc((void**)&cv.scale, cv.npad * 4);
    if (rc) return rc;
    rc = dalloc((void**)&cv.shift, cv.npad * 4);
    if (rc) return rc;
    VD_CHECK_HIP(hipMemcpy(cv.scale, sc.data(), cv.npad * 4, hipMemcpyHostToDevice));
    VD_CHECK_HIP(hipMemcpy(cv.shift, sh.data(), cv.npad * 4, hipMemcpyHostToDevice));
    cv.flops_per_px = 2.0 * cv.cout * cv.kh * cv.kw * cv.cin;
    return VD_OK;
}

const HT* find_t(const WMap& W, const std::string& k) {
    auto it = W.find(k);
    return it == W.end() ? nullptr : &it->second;
}

// conv weight `wkey` [cout][cin][kh][kw] + BatchNorm at `bn` (eval: alpha =
// gamma/sqrt(var+eps), beta = bias - mean*alpha, as torch's CPU inference kernel).
int Ctx::make_conv_bn(const WMap& W, const std::string& wkey, const std::string& bn, float eps, int stride,
                      int pad, int act, float slope, int* out_idx) {
    return make_conv_bn_cat(W, {{wkey, bn}}, eps, stride, pad, act, slope, out_idx);
}

// Several conv+BN pairs reading the same input, stacked along Cout in the given
// order (the SSH conv5X5_1 + conv3X3 pair of face_net.cpp): one GEMM, per-channel
// scale/shift, so every output channel is computed exactly as by its own conv.
int Ctx::make_conv_bn_cat(const WMap& W, const std::vector<std::pair<std::string, std::string>>& parts, float eps,
                          int stride, int pad, int act, float slope, int* out_idx) {
    Conv cv{};
    std::vector<float> wall, sc, sh;
    for (size_t i = 0; i < parts.size(); ++i) {
        const std::string& wkey = parts[i].first;
        const std::string& bn = parts[i].second;
        const HT* w = find_t(W, wkey);
        if (!w || w->shape.size() != 4) return vd_set_error(VD_ERR_WEIGHTS, "missing/bad conv weight %s", wkey.c_str());
        if (i == 0) { cv.cin = w->shape[1]; cv.kh = w->shape[2]; cv.kw = w->shape[3]; }
        if (w->shape[1] != cv.cin || w->shape[2] != cv.kh || w->shape[3] != cv.kw)
            return vd_set_error(VD_ERR_WEIGHTS, "conv shape mismatch at %s", wkey.c_str());
        const int co = w->shape[0];
        wall.insert(wall.end(), w->data.begin(), w->data.end());
        if (bn.empty()) {
            sc.insert(sc.end(), co, 1.f);
            sh.insert(sh.end(), co, 0.f);
        } else {
            const HT* g = find_t(W, bn + ".weight");
            const HT* b = find_t(W, bn + ".bias");
            const HT* m = find_t(W, bn + ".running_mean");
            const HT* v = find_t(W, bn + ".running_var");
            if (!g || !b || !m || !v) return vd_set_error(VD_ERR_WEIGHTS, "missing BatchNorm tensors under %s", bn.c_str());
            for (int n = 0; n < co; ++n) {
                const float alpha = g->data[n] / std::sqrt(v->data[n] + eps);
                sc.push_back(alpha);
                sh.push_back(b->data[n] - m->data[n] * alpha);
            }
        }
        cv.cout += co;
    }
    cv.stride = stride; cv.pad = pad; cv.act = act; cv.slope = slope;
    int rc = upload_conv(cv, wall, sc, sh);
    if (rc) return rc;
    convs.push_back(cv);
    *out_idx = (int)convs.size() - 1;
    return VD_OK;
}

// Depthwise 3x3 conv [c][1][3][3] + BatchNorm at `bn` (mobilenet025.py:10-14), weights
// stored tap-major [9][c] in the compute type (dwconv.hip reads 16 B of channels per tap).
int Ctx::make_dwconv_bn(const WMap& W, const std::string& wkey, const std::string& bn, float eps, int stride,
                        int act, float slope, int* idx) {
    const HT* w = find_t(W, wkey);
    if (!w || w->shape.size() != 4 || w->shape[1] != 1 || w->shape[2] != 3 || w->shape[3] != 3)
        return vd_set_error(VD_ERR_WEIGHTS, "missing/bad depthwise weight %s", wkey.c_str());
    const HT* g = find_t(W, bn + ".weight");
    const HT* b = find_t(W, bn + ".bias");
    const HT* m = find_t(W, bn + ".running_mean");
    const HT* v = find_t(W, bn + ".running_var");
    if (!g || !b || !m || !v) return vd_set_error(VD_ERR_WEIGHTS, "missing BatchNorm tensors under %s", bn.c_str());
    DwConv d;
    d.c = w->shape[0]; d.stride = stride; d.act = act; d.slope = slope;
    if (d.c % (f32 ? 4 : 8)) return vd_set_error(VD_ERR_WEIGHTS, "depthwise %s: %d channels", wkey.c_str(), d.c);
    std::vector<float> wt((size_t)9 * d.c), sc(d.c), sh(d.c);
    for (int c = 0; c < d.c; ++c) {
        for (int t = 0; t < 9; ++t) wt[(size_t)t * d.c + c] = w->data[(size_t)c * 9 + t];
        const float alpha = g->data[c] / std::sqrt(v->data[c] + eps);
        sc[c] = alpha;
        sh[c] = b->data[c] - m->data[c] * alpha;
    }
    int rc;
    if (f32) {
        if ((rc = dalloc(&d.w, wt.size() * 4))) return rc;
        VD_CHECK_HIP(hipMemcpy(d.w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> h(wt.size());
        for (size_t i = 0; i < wt.size(); ++i) h[i] = to_half(f16, wt[i]);
        if ((rc = dalloc(&d.w, h.size() * 2))) return rc;
        VD_CHECK_HIP(hipMemcpy(d.w, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    if ((rc = dalloc((void**)&d.scale, d.c * 4)) || (rc = dalloc((void**)&d.shift, d.c * 4))) return rc;
    VD_CHECK_HIP(hipMemcpy(d.scale, sc.data(), d.c * 4, hipMemcpyHostToDevice));
    VD_CHECK_HIP(hipMemcpy(d.shift, sh.data(), d.c * 4, hipMemcpyHostToDevice));
    dwconvs.push_back(d);
    *idx = (int)dwconvs.size() - 1;
    return VD_OK;
}

int Ctx::add_dwconv(Net& net, int di, const Act& x, Act& y) {
    const DwConv& d = dwconvs[di];
    if (x.c < d.c || y.c < d.c || y.h != (x.h - 1) / d.stride + 1 || y.w != (x.w - 1) / d.stride + 1)
        return vd_set_error(VD_ERR_ARG, "depthwise conv plan shape mismatch");
    Op op{};
    op.kind = OP_DWCONV;
    op.conv = di;
    op.x = x;
    op.y = y;
    net.ops.push_back(op);
    return VD_OK;
}

// Several 1x1 conv heads with bias fused along Cout (retinaface.py:90-92,140-142).
// cin_perm (1x1 heads): input channel i of the packed conv reads the tensors' channel
// cin_perm[i] (a concat laid out in another block order)
int Ctx::make_conv_cat(const WMap& W, const std::vector<std::string>& wkeys, const std::vector<std::string>& bkeys,
                       int act, int* out_idx, const std::vector<int>* cin_perm) {
    Conv cv{};
    std::vector<float> wall, sc, sh;
    for (size_t i = 0; i < wkeys.size(); ++i) {
        const HT* w = find_t(W, wkeys[i]);
        const HT* b = bkeys[i].empty() ? nullptr : find_t(W, bkeys[i]);
        if (!w || w->shape.size() != 4 || (!bkeys[i].empty() && !b))
            return vd_set_error(VD_ERR_WEIGHTS, "missing head tensor %s", wkeys[i].c_str());
        if (i == 0) { cv.cin = w->shape[1]; cv.kh = w->shape[2]; cv.kw = w->shape[3]; }
        if (w->shape[1] != cv.cin || w->shape[2] != cv.kh || w->shape[3] != cv.kw)
            return vd_set_error(VD_ERR_WEIGHTS, "head shape mismatch at %s", wkeys[i].c_str());
        wall.insert(wall.end(), w->data.begin(), w->data.end());
        for (int n = 0; n < w->shape[0]; ++n) { sc.push_back(1.f); sh.push_back(b ? b->data[n] : 0.f); }
        cv.cout += w->shape[0];
    }
    if (cin_perm) {
        if ((int)cin_perm->size() != cv.cin || cv.kh != 1 || cv.kw != 1)
            return vd_set_error(VD_ERR_STATE, "internal: head channel permutation");
        std::vector<float> pw(wall.size());
        for (int o = 0; o < cv.cout; ++o)
            for (int i = 0; i < cv.cin; ++i) pw[(size_t)o * cv.cin + i] = wall[(size_t)o * cv.cin + (*cin_perm)[i]];
        wall.swap(pw);
    }
    cv.stride = 1; cv.pad = cv.kh / 2; cv.act = act; cv.slope = 0.f;
    int rc = upload_conv(cv, wall, sc, sh);
    if (rc) return rc;
    convs.push_back(cv);
    *out_idx = (int)convs.size() - 1;
    return VD_OK;
}

// Bottleneck conv3 (ci on x) + downsample (c2 on x2, strided 1x1) in one op.
bool Ctx::dual_ok(int ci, int c2, const Act& y) const {
    const Conv& a = convs[ci];
    const Conv& b = convs[c2];
    if (f32) {   // fp16-pair plan: conv1x1_x6_dual_kernel
        if (!tune.conv_dual || a.split != 2 || b.split != 2 || b.cout != a.cout || b.act != VD_ACT_NONE) return false;
        ConvArgs t{};
        t.kh = a.kh; t.kw = a.kw; t.pad = a.pad; t.stride = a.stride; t.cin_pad = a.cin_pad; t.kpad = a.kpad;
        t.cout = a.cout; t.act = a.act; t.res_mode = VD_RES_NONE; t.ldx = a.cin_pad; t.ldy = y.c;
        t.ldx2 = b.cin_pad; t.cin2_pad = b.cin_pad; t.kpad2 = b.kpad; t.f32_split = 2;
        t.wx3 = a.wx3; t.wx3_2 = b.wx3; t.scale_x = a.scale_x; t.scale2_x = b.scale_x;
        return b.kh == 1 && b.kw == 1 && b.pad == 0 && vd_conv1x1_x6_dual_ok(t);
    }
    ConvArgs t{};
    t.kh = a.kh; t.kw = a.kw; t.pad = a.pad; t.stride = a.stride; t.cin_pad = a.cin_pad; t.kpad = a.kpad;
    t.cout = a.cout; t.act = a.act; t.res_mode = VD_RES_NONE; t.ldx = a.cin_pad; t.ldy = y.c; t.x2 = (const void*)1;
    t.cin2_pad = b.cin_pad; t.kpad2 = b.kpad; t.ldx2 = b.cin_pad; t.tune = &tune;
    return b.kh == 1 && b.kw == 1 && b.pad == 0 && b.cout == a.cout && b.act == VD_ACT_NONE && vd_conv1x1_dual_ok(t);
}

int Ctx::add_conv_dual(Net& net, int ci, const Act& x, int c2, const Act& x2, Act& y) {
    int rc = add_conv(net, ci, x, 0, y, 0);
    if (rc) return rc;
    const Conv& b = convs[c2];
    if ((x2.h - 1) / b.stride + 1 != y.h || (x2.w - 1) / b.stride + 1 != y.w || b.cin_pad > x2.c)
        return vd_set_error(VD_ERR_ARG, "dual conv plan shape mismatch");
    net.ops.back().conv2 = c2;
    net.ops.back().x2 = x2;
    return VD_OK;
}

int Ctx::add_conv(Net& net, int ci, const Act& x, int xcoff, Act& y, int ycoff, const Act* res, int rcoff, int rmode,
                  int rup) {
    const Conv& cv = convs[ci];
    Op op{};
    op.kind = OP_CONV;
    op.conv = ci;
    op.x = x; op.xcoff = xcoff;
    op.y = y; op.ycoff = ycoff;
    if (res) { op.r = *res; op.rcoff = rcoff; op.rmode = rmode; op.rup = rup; }
    const int oh = (x.h + 2 * cv.pad - cv.kh) / cv.stride + 1;
    const int ow = (x.w + 2 * cv.pad - cv.kw) / cv.stride + 1;
    const int xspan = cv.grp_co ? (cv.cout / cv.grp_co - 1) * cv.grp_ci + cv.cin_pad : cv.cin_pad;
    if (oh != y.h || ow != y.w || ycoff + cv.cout > y.c || xcoff + xspan > x.c)
        return vd_set_error(VD_ERR_ARG, "conv plan shape mismatch (%dx%d vs %dx%d)", oh, ow, y.h, y.w);
    net.ops.push_back(op);
    return VD_OK;
}

// ----------------------------------------------------------------------------
// plan execution
// ----------------------------------------------------------------------------
void Ctx::t_begin(int fam, double work) {
    if (!timing) return;
    if (ev_used == ev_pool.size()) {
        TimedEv t{};
        hipEventCreate(&t.a);
        hipEventCreate(&t.b);
        ev_pool.push_back(t);
    }
    TimedEv& t = ev_pool[ev_used];
    t.fam = fam;
    t.work = work;
    hipEventRecord(t.a, stream);
}

void Ctx::t_end() {
    if (!timing) return;
    hipEventRecord(ev_pool[ev_used].b, stream);
    ++ev_used;
}

static inline const void* foff(const Act& a, int f0) {
    return a.p ? (const char*)a.p + (size_t)f0 * a.h * a.w * a.c * (a.f32 ? 4 : 2) : nullptr;
}

int Ctx::run_conv_op(const Op& op, int f0, int n, int fam) {
    const Conv& cv = convs[op.conv];
    ConvArgs a{};
    a.x = foff(op.x, f0); a.xh = op.x.h; a.xw = op.x.w; a.ldx = op.x.c; a.xcoff = op.xcoff;
    a.w = cv.w; a.scale = cv.scale; a.shift = cv.shift;
    a.res = foff(op.r, f0); a.res_ld = op.r.c; a.res_coff = op.rcoff; a.res_up = op.rup; a.rh = op.r.h; a.rw = op.r.w;
    a.res_mode = op.r.p ? op.rmode : VD_RES_NONE;
    a.y = (void*)foff(op.y, f0); a.yh = op.y.h; a.yw = op.y.w; a.ldy = op.y.c; a.ycoff = op.ycoff;
    a.B = n; a.cin_pad = cv.cin_pad; a.cout = cv.cout; a.kpad = cv.kpad;
    a.kh = cv.kh; a.kw = cv.kw; a.stride = cv.stride; a.pad = cv.pad;
    a.M = n * op.y.h * op.y.w;
    a.act = cv.act; a.slope = cv.slope; a.out_f32 = op.y.f32 ? 1 : 0;
    a.f16 = f16 ? 1 : 0;
    a.tune = &tune;
    a.wx3 = cv.wx3;
    a.scale_x = cv.scale_x;
    a.f32_split = cv.split;
    a.xmax = op.x.amax ? op.x.amax + f0 : nullptr;
    a.xbound = op.x.bound;
    a.x_exact = (op.x.exact16 && cv.split == 2 && tune.x6_exact) ? 1 : 0;
    a.ymax = op.y.amax ? op.y.amax + f0 : nullptr;
    a.grp_co = cv.grp_co; a.grp_ci = cv.grp_ci;
    if (cv.split == 2 && !a.xmax && !(a.xbound > 0.f))
        return vd_set_error(VD_ERR_ARG, "internal: conv input without a range (fp16-pair plan)");
    if (a.xmax && op.x.amax == op.y.amax) {
        // input and output are channel slices of one buffer (the SSH concat): the kernel
        // reads the input's per-frame range while its epilogue raises the same slots, so
        // it reads a copy frozen before the launch (one array per conv: the frame groups
        // run the same conv concurrently on disjoint frames)
        unsigned*& snap = amax_snaps[op.conv];
        if (!snap) {
            int rc = dalloc((void**)&snap, (size_t)cfg.max_batch * 4);
            if (rc) return rc;
        }
        VD_CHECK_HIP(hipMemcpyAsync(snap + f0, a.xmax, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
        a.xmax = snap + f0;
    }
    double flops = cv.flops_per_px * a.M;
    if (op.conv2 >= 0) {
        const Conv& c2 = convs[op.conv2];
        a.x2 = foff(op.x2, f0); a.xh2 = op.x2.h; a.xw2 = op.x2.w; a.ldx2 = op.x2.c; a.xcoff2 = 0;
        a.stride2 = c2.stride; a.w2 = c2.w; a.scale2 = c2.scale; a.shift2 = c2.shift;
        a.cin2_pad = c2.cin_pad; a.kpad2 = c2.kpad;
        a.wx3_2 = c2.wx3; a.scale2_x = c2.scale_x;
        a.x2max = op.x2.amax ? op.x2.amax + f0 : nullptr;
        a.x2bound = op.x2.bound;
        flops += c2.flops_per_px * a.M;
    }
    t_begin(fam, flops);
    hipError_t e = vd_launch_conv(a, f32, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "conv launch: %s", hipGetErrorString(e));
    return VD_OK;
}

// conv3 (+ identity) of one bottleneck and conv1 of the next in one pass (chain.hip)
int Ctx::run_chain_op(const Op& op, int f0, int n, int fam) {
    const Conv& c3 = convs[op.conv];
    const Conv& c1 = convs[op.conv2];
    if (f32) {   // fp16-pair plan (chain32.hip)
        Chain32Args a{};
        a.t2 = foff(op.x, f0); a.ld_t2 = op.x.c;
        a.res = foff(op.r, f0); a.ld_res = op.r.c;
        a.w3 = c3.wx3; a.w1 = c1.wx3_chain;
        a.sc3 = c3.scale_x; a.sh3 = c3.shift; a.sc1 = c1.scale_x; a.sh1 = c1.shift;
        a.y = (void*)foff(op.y, f0); a.ld_y = op.y.c;
        a.y2 = (void*)foff(op.y2, f0); a.ld_y2 = op.y2.c;
        a.hw = op.y.h * op.y.w;
        a.M = n * a.hw;
        a.B = n;
        a.xmax = op.x.amax ? op.x.amax + f0 : nullptr; a.xbound = op.x.bound;
        a.ymax = op.y.amax ? op.y.amax + f0 : nullptr;
        a.y2max = op.y2.amax ? op.y2.amax + f0 : nullptr;
        a.gpw = tune.chain_gpw;
        t_begin(fam, (c3.flops_per_px + c1.flops_per_px) * a.M);
        hipError_t e = vd_launch_chain32(a, stream);
        t_end();
        if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "chain32 launch: %s", hipGetErrorString(e));
        return VD_OK;
    }
    ChainArgs a{};
    a.t2 = foff(op.x, f0); a.ld_t2 = op.x.c;
    a.res = foff(op.r, f0); a.ld_res = op.r.c;
    a.w3 = c3.w; a.kpad3 = c3.kpad; a.sc3 = c3.scale; a.sh3 = c3.shift;
    a.w1 = c1.w; a.kpad1 = c1.kpad; a.sc1 = c1.scale; a.sh1 = c1.shift;
    a.y = (void*)foff(op.y, f0); a.ld_y = op.y.c;
    a.y2 = (void*)foff(op.y2, f0); a.ld_y2 = op.y2.c;
    a.M = n * op.y.h * op.y.w;
    a.f16 = f16 ? 1 : 0;
    t_begin(fam, (c3.flops_per_px + c1.flops_per_px) * a.M);
    hipError_t e = vd_launch_chain(a, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "chain launch: %s", hipGetErrorString(e));
    return VD_OK;
}

// Peephole over ops [begin, end) of a bf16 / fp16 plan: a bottleneck conv3 (1x1, + identity
// before the ReLU) immediately followed by a 1x1 conv that reads exactly its output
// (the next bottleneck's conv1) becomes one OP_CHAIN where chain.hip covers the shape.
// fp32 plan (chain32.hip): the same peephole on the layer2 shape with fp16-pair weights;
// conv1's planes are copied with K permuted inside each 32-channel step (position 8q + e
// <- channel 4q + e, 8q + 4 + e <- 16 + 4q + e) so conv3's accumulator lanes are its B
// fragments.
int Ctx::chain32_weights(Conv& c1) {
    if (c1.wx3_chain) return VD_OK;
    const size_t rows = (size_t)c1.npad, nk = (size_t)c1.kpad / 32, bytes = rows * nk * 2 * 64;
    std::vector<uint16_t> src(bytes / 2), dst(bytes / 2);
    VD_CHECK_HIP(hipMemcpy(src.data(), c1.wx3, bytes, hipMemcpyDeviceToHost));
    for (size_t blk = 0; blk < rows * nk * 2; ++blk)       // one 32-entry plane of one k-step of one row
        for (int qq = 0; qq < 4; ++qq)
            for (int e = 0; e < 4; ++e) {
                dst[blk * 32 + 8 * qq + e] = src[blk * 32 + 4 * qq + e];
                dst[blk * 32 + 8 * qq + 4 + e] = src[blk * 32 + 16 + 4 * qq + e];
            }
    int rc = dalloc(&c1.wx3_chain, bytes);
    if (rc) return rc;
    VD_CHECK_HIP(hipMemcpy(c1.wx3_chain, dst.data(), bytes, hipMemcpyHostToDevice));
    return VD_OK;
}

void Ctx::fuse_chains(Net& net, size_t begin) {
    if (f32) {
        fuse_chains32(net, begin);
        return;
    }
    std::vector<Op> out(net.ops.begin(), net.ops.begin() + begin);
    for (size_t i = begin; i < net.ops.size(); ++i) {
        const Op& a = net.ops[i];
        if (i + 1 < net.ops.size() && a.kind == OP_CONV && net.ops[i + 1].kind == OP_CONV && a.conv2 < 0) {
            const Op& b = net.ops[i + 1];
            const Conv& c3 = convs[a.conv];
            const Conv& c1 = convs[b.conv];
            const bool shape = c3.kh == 1 && c3.kw == 1 && c3.stride == 1 && c3.pad == 0 && c3.act == VD_ACT_RELU &&
                               c1.kh == 1 && c1.kw == 1 && c1.stride == 1 && c1.pad == 0 && c1.act == VD_ACT_RELU &&
                               a.r.p && a.rmode == VD_RES_PRE_ACT && !a.rup && a.rcoff == 0 && a.xcoff == 0 &&
                               a.ycoff == 0 && b.conv2 < 0 && !b.r.p && b.x.p == a.y.p && b.xcoff == 0 &&
                               b.ycoff == 0 && !a.y.f32 && !b.y.f32 && c3.cin_pad == a.x.c &&
                               c1.cin_pad == c3.cout && a.r.h == a.y.h && a.r.w == a.y.w;
            const long M = (long)cfg.max_batch * a.y.h * a.y.w;
            if (shape && tune.chain && vd_chain_ok(c3.cin_pad, c3.cout, c3.kpad, c1.kpad, a.x.c, a.r.c, a.y.c, b.y.c, M)) {
                Op op = a;
                op.kind = OP_CHAIN;
                op.conv2 = b.conv;
                op.y2 = b.y;
                out.push_back(op);
                ++i;
                continue;
            }
        }
        out.push_back(a);
    }
    net.ops.swap(out);
}

void Ctx::fuse_chains32(Net& net, size_t begin) {
    if (!tune.chain) return;
    std::vector<Op> out(net.ops.begin(), net.ops.begin() + begin);
    for (size_t i = begin; i < net.ops.size(); ++i) {
        const Op& a = net.ops[i];
        if (i + 1 < net.ops.size() && a.kind == OP_CONV && net.ops[i + 1].kind == OP_CONV && a.conv2 < 0) {
            const Op& b = net.ops[i + 1];
            const Conv& c3 = convs[a.conv];
            Conv& c1 = convs[b.conv];
            const bool shape = c3.kh == 1 && c3.kw == 1 && c3.stride == 1 && c3.pad == 0 && c3.act == VD_ACT_RELU &&
                               c1.kh == 1 && c1.kw == 1 && c1.stride == 1 && c1.pad == 0 && c1.act == VD_ACT_RELU &&
                               c3.split == 2 && c1.split == 2 && c3.wx3 && c1.wx3 && c3.scale_x && c1.scale_x &&
                               a.r.p && a.rmode == VD_RES_PRE_ACT && !a.rup && a.rcoff == 0 && a.xcoff == 0 &&
                               a.ycoff == 0 && b.conv2 < 0 && !b.r.p && b.x.p == a.y.p && b.xcoff == 0 &&
                               b.ycoff == 0 && a.x.f32 && a.y.f32 && b.y.f32 && a.r.f32 && c3.cin_pad == a.x.c &&
                               c1.cin_pad == c3.cout && a.r.h == a.y.h && a.r.w == a.y.w;
            const long M = (long)cfg.max_batch * a.y.h * a.y.w;
            const bool take = tune.chain == 1 || c3.cin_pad == 128;   // option chain=2 (default): layer2 only
            if (shape && take && vd_chain32_ok(c3.cin_pad, c3.cout, c3.kpad, c1.kpad, a.x.c, a.r.c, a.y.c, b.y.c, M,
                                       cfg.max_batch) &&
                chain32_weights(c1) == VD_OK) {
                Op op = a;
                op.kind = OP_CHAIN;
                op.conv2 = b.conv;
                op.y2 = b.y;
                out.push_back(op);
                ++i;
                continue;
            }
        }
        out.push_back(a);
    }
    net.ops.swap(out);
}

int Ctx::run_dwconv_op(const Op& op, int f0, int n) {
    const DwConv& d = dwconvs[op.conv];
    DwConvArgs a{};
    a.x = foff(op.x, f0); a.xh = op.x.h; a.xw = op.x.w; a.ldx = op.x.c; a.xcoff = 0;
    a.w = d.w; a.scale = d.scale; a.shift = d.shift;
    a.y = (void*)foff(op.y, f0); a.yh = op.y.h; a.yw = op.y.w; a.ldy = op.y.c; a.ycoff = 0;
    a.B = n; a.c = d.c; a.stride = d.stride; a.act = d.act; a.slope = d.slope;
    a.ymax = op.y.amax ? op.y.amax + f0 : nullptr;
    t_begin(4, 0);
    hipError_t e = vd_launch_dwconv(a, f32, f16, stream);
    t_end();
    if (e != hipSuccess) return vd_set_error(VD_ERR_HIP, "depthwise conv: %s", hipGetErrorString(e));
    return VD_OK;
}

// max-pool / upsample: the output's per-frame range is within the input's
static hipError_t amax_follow_impl(const Op& op, int f0, int n, hipStream_t s) {
    if (!op.y.amax || op.y.amax == op.x.amax) return hipSuccess;   // in-place slices: already covered
    if (!op.x.amax) return op.x.bound > 0.f ? hipErrorInvalidValue : hipSuccess;
    return vd_launch_amax_merge(op.y.amax + f0, op.x.amax + f0, n, s);
}

int Ctx::run_ops(const Net& net, int b, int e, int f0, int n) {
    // two lanes (face net, option ssh_side): lane-1 ops run on stream_side; an op with
    // dep >= 0 waits for that op's completion event first (recorded below on the
    // producer's lane); after the net's last op the main lane waits for the side lane
    const bool lanes = &net == &face.net && !lane_ev.empty();
    hipStream_t main = stream;
    bool side_used = false;
    for (int i = b; i < e; ++i) {
        const Op& op = net.ops[i];
        int rc = VD_OK;
        if (lanes) {
            stream = op.lane ? stream_side : main;
            side_used |= op.lane != 0;
            if (op.dep >= 0) VD_CHECK_HIP(hipStreamWaitEvent(stream, lane_ev[op.dep], 0));
        }
        if (op.kind == OP_CONV) {
            rc = run_conv_op(op, f0, n, net.conv_fam);
        } else if (op.kind == OP_BLOCK) {
            rc = run_block_op(op, f0, n, net.conv_fam);
        } else if (op.kind == OP_CHAIN) {
            rc = run_chain_op(op, f0, n, net.conv_fam);
        } else if (op.kind == OP_STEMPOOL) {
            rc = run_stem_pool_op(op, f0, n, net.conv_fam);
        } else if (op.kind == OP_DWCONV) {
            rc = run_dwconv_op(op, f0, n);
        } else if (op.kind == OP_MAXPOOL) {
            t_begin(4, 0);
            hipError_t er = vd_launch_maxpool(f32, f16, foff(op.x, f0), n, op.x.h, op.x.w, op.x.c, op.xcoff,
                                              (void*)foff(op.y, f0), op.y.h, op.y.w, op.y.c, op.ycoff, op.ch, op.k,
                                              op.s, op.p, stream);
            t_end();
            if (er == hipSuccess) er = amax_follow_impl(op, f0, n, stream);
            if (er != hipSuccess) rc = vd_set_error(VD_ERR_HIP, "maxpool: %s", hipGetErrorString(er));
        } else if (op.kind == OP_UPSAMPLE) {
            t_begin(4, 0);
            hipError_t er = vd_launch_upsample2x(f32, foff(op.x, f0), n, op.x.h, op.x.w, op.x.c, op.xcoff,
                                                 (void*)foff(op.y, f0), op.y.c, op.ycoff, op.ch, stream);
            t_end();
            if (er == hipSuccess) er = amax_follow_impl(op, f0, n, stream);
            if (er != hipSuccess) rc = vd_set_error(VD_ERR_HIP, "upsample: %s", hipGetErrorString(er));
        }
        if (lanes && lane_ev[i]) VD_CHECK_HIP(hipEventRecord(lane_ev[i], stream));
        if (lanes) stream = main;
        if (rc) return rc;
        if (&net == &face.net && i + 1 == fork_at) VD_CHECK_HIP(hipEventRecord(ev_fork, stream));
    }
    if (lanes && side_used) {
        VD_CHECK_HIP(hipEventRecord(ev_side, stream_side));
        VD_CHECK_HIP(hipStreamWaitEvent(stream, ev_side, 0));
    }
    return VD_OK;
}

// The face net's op list as built (FPN o3 o2 m2 o1 m1, then SSH + heads of levels 0, 1,
// 2) reordered into two lanes: level 2's chain right after o3 and level 1's after m2,
// both on the side stream, so they fill the CUs that FPN merge1 and the level-0 SSH
// convs (6x the pixels) leave idle in their last partial rounds. Same kernels and
// operands: results are bit-identical to the one-lane order.
int Ctx::face_lanes(const int (&fpn)[5], const int (&ssh_b)[3], const int (&ssh_e)[3]) {
    Net& net = face.net;
    std::vector<Op> out(net.ops.begin(), net.ops.begin() + fpn[0]);
    auto take = [&](int b, int e, int lane, int dep) {
        for (int i = b; i < e; ++i) {
            Op op = net.ops[i];
            op.lane = lane;
            op.dep = i == b ? dep : -1;
            out.push_back(op);
        }
    };
    take(fpn[0], fpn[0] + 1, 0, -1);                      // o3
    const int p_o3 = (int)out.size() - 1;
    take(ssh_b[2], ssh_e[2], 1, p_o3);                     // level 2 (reads o3)
    take(fpn[1], fpn[2] + 1, 0, -1);                       // o2, m2
    const int p_m2 = (int)out.size() - 1;
    take(ssh_b[1], ssh_e[1], 1, p_m2);                     // level 1 (reads m2)
    take(fpn[3], fpn[4] + 1, 0, -1);                       // o1, m1
    take(ssh_b[0], ssh_e[0], 0, -1);                       // level 0
    if (out.size() != net.ops.size()) return vd_set_error(VD_ERR_STATE, "internal: face lanes lost ops");
    net.ops.swap(out);
    if (!stream_side) {
        VD_CHECK_HIP(hipStreamCreateWithFlags(&stream_side, hipStreamNonBlocking));
        VD_CHECK_HIP(hipEventCreateWithFlags(&ev_side, hipEventDisableTiming));
    }
    for (hipEvent_t ev : lane_ev)
        if (ev) hipEventDestroy(ev);
    lane_ev.assign(net.ops.size(), nullptr);
    for (int i : {p_o3, p_m2}) VD_CHECK_HIP(hipEventCreateWithFlags(&lane_ev[i], hipEventDisableTiming));
    return VD_OK;
}

// Depth-first over micro-batches of `mb` frames for ops [0, split) -- each
// micro-batch's stem/layer1/layer2 intermediates (~100-200 MB) then stay in the
// 256 MiB Infinity Cache between producer and consumer -- then ops [split, end)
// over the whole batch (the small late layers need the whole batch to fill 256 CUs).
int Ctx::run_net(const Net& net, int n, int mb, int split) {
    const int ne = (int)net.ops.size();
    if (net.amax) VD_CHECK_HIP(hipMemsetAsync(net.amax, 0, net.amax_bytes, stream));
    if (mb <= 0 || mb >= n || split <= 0) return run_ops(net, 0, ne, 0, n);
    for (int f0 = 0; f0 < n; f0 += mb) {
        int rc = run_ops(net, 0, split, f0, std::min(mb, n - f0));
        if (rc) return rc;
    }
    return run_ops(net, split, ne, 0, n);
}

extern "C" {

int vd_abi_version(void) { return VDMI_ABI_VERSION; }
const char* vd_last_error(void) { return g_err.c_str(); }

int vd_default_cfg(vd_cfg* c) {
    if (!c) return vd_set_error(VD_ERR_ARG, "null cfg");
    memset(c, 0, sizeof *c);
    c->input_h = 640; c->input_w = 640;     // combine_detect.py:860
    c->max_batch = 64;                      // config.ini:35
    c->max_frame_h = 2160; c->max_frame_w = 3840;
    c->precision = VD_PREC_BF16;
    c->max_boxes = 256;
    c->confidence = 0.5f;                   // combine_detect.py:861
    c->nms_iou = 0.4;                       // combine_detect.py:862
    c->mosaic_level = 8;                    // combine_detect.py:249
    c->plate_imgsz = 640;
    c->plate_nc = 1;
    c->plate_conf = 0.5f;                   // combine_detect.py:217
    c->plate_iou = 0.7;                     // ultralytics default [ext]
    c->plate_max_det = 300;                 // ultralytics default [ext]
    return VD_OK;
}

int vd_create(const vd_cfg* cfg, int device, vd_ctx** out) {
    if (!out) return vd_set_error(VD_ERR_ARG, "null out");
    *out = nullptr;
    vd_cfg c;
    if (cfg) c = *cfg; else vd_default_cfg(&c);
    if (c.max_batch <= 0 || c.input_h % 32 || c.input_w % 32 || c.input_h <= 0 || c.input_w <= 0)
        return vd_set_error(VD_ERR_ARG, "cfg: max_batch>0 and input dims multiple of 32 required");
    if (c.precision != VD_PREC_BF16 && c.precision != VD_PREC_FP32 && c.precision != VD_PREC_FP16)
        return vd_set_error(VD_ERR_ARG, "cfg: bad precision");
    if (c.mosaic_level <= 0) c.mosaic_level = 8;
    if (c.blur_mode != VD_BLUR_PIXELATE && c.blur_mode != VD_BLUR_GAUSSIAN)
        return vd_set_error(VD_ERR_ARG, "cfg: bad blur_mode %d", c.blur_mode);
    if (c.blur_mode == VD_BLUR_GAUSSIAN) {
        if (c.blur_ksize == 0) c.blur_ksize = 31;
        uint32_t q[VD_BLUR_KSIZE_MAX];
        if (vd_blur_weights(c.blur_ksize, c.blur_sigma, q))
            return vd_set_error(VD_ERR_ARG, "cfg: blur_ksize must be odd in [3, %d] (got %d) and blur_sigma finite",
                                VD_BLUR_KSIZE_MAX, c.blur_ksize);
    }
    if (c.hold_frames < 0 || c.hold_frames > VD_HOLD_MAX || c.hold_iou_pct < 0 || c.hold_iou_pct > 100)
        return vd_set_error(VD_ERR_ARG, "cfg: hold_frames in [0, %d] and hold_iou_pct in [0, 100] required (got %d, %d)",
                            VD_HOLD_MAX, c.hold_frames, c.hold_iou_pct);
    if (c.hold_iou_pct == 0) c.hold_iou_pct = 30;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return vd_set_error(VD_ERR_HIP, "no HIP device %d (count %d)", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return vd_set_error(VD_ERR_HIP, "hipSetDevice(%d)", device);
    Ctx* ctx = new Ctx();
    ctx->cfg = c;
    ctx->device = device;
    ctx->f32 = c.precision == VD_PREC_FP32;
    ctx->f16 = c.precision == VD_PREC_FP16;
    ctx->hold.K = c.hold_frames;
    ctx->hold.P = c.hold_iou_pct;
    ctx->rescue_hs.K = std::max(1, c.hold_frames);   // the rescue window W
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return vd_set_error(VD_ERR_HIP, "hipStreamCreate failed");
    }
    ctx->stream = ctx->own_stream;
    {
        const unsigned hw = std::thread::hardware_concurrency();
        ctx->jpeg_threads = (int)std::max(1u, std::min(16u, hw ? hw : 4u));   // one GPU's host share
    }
    if (hipEventCreateWithFlags(&ctx->jpeg_ev, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return vd_set_error(VD_ERR_HIP, "stream/event creation failed");
    }
    *out = (vd_ctx*)ctx;
    return VD_OK;
}

int vd_destroy(vd_ctx* h) {
    Ctx* ctx = (Ctx*)h;
    if (!ctx) return VD_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (void* p : ctx->allocs) hipFree(p);
    if (ctx->stage_in) hipFree(ctx->stage_in);
    if (ctx->stage_out) hipFree(ctx->stage_out);
    if (ctx->stage_box) hipFree(ctx->stage_box);
    if (ctx->stage_box2) hipFree(ctx->stage_box2);
    if (ctx->mosaic_table) hipFree(ctx->mosaic_table);
    if (ctx->blur_table) hipFree(ctx->blur_table);
    if (ctx->hold_rows) hipFree(ctx->hold_rows);
    if (ctx->lead_rows) hipFree(ctx->lead_rows);
    ctx->lead_free();
    if (ctx->mask_rows) hipFree(ctx->mask_rows);
    if (ctx->tiles_buf) hipFree(ctx->tiles_buf);
    if (ctx->ptiles_buf) hipFree(ctx->ptiles_buf);
    if (ctx->tiles_in) hipFree(ctx->tiles_in);
    for (int* p : ctx->hold_hist)
        if (p) hipFree(p);
    if (ctx->rescue_rows) hipFree(ctx->rescue_rows);
    for (int* p : ctx->rescue_hist)
        if (p) hipFree(p);
    if (ctx->jpeg_dev) hipFree(ctx->jpeg_dev);
    if (ctx->jpeg_planes) hipFree(ctx->jpeg_planes);
    if (ctx->jpeg_host) hipHostFree(ctx->jpeg_host);
    if (ctx->jdec_host) hipHostFree(ctx->jdec_host);
    if (ctx->jdec_dev) hipFree(ctx->jdec_dev);
    if (ctx->jdec_work) hipFree(ctx->jdec_work);
    if (ctx->jenc_dev) hipFree(ctx->jenc_dev);
    if (ctx->jhuf_dev) hipFree(ctx->jhuf_dev);
    if (ctx->jseg_host) hipHostFree(ctx->jseg_host);
    if (ctx->jenc_host) hipHostFree(ctx->jenc_host);
    if (ctx->jpeg_ev) hipEventDestroy(ctx->jpeg_ev);
    for (auto& t : ctx->ev_pool) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
    hipStreamSynchronize(ctx->stream2);
    if (ctx->stream_side) {
        hipStreamSynchronize(ctx->stream_side);
        hipStreamDestroy(ctx->stream_side);
        hipEventDestroy(ctx->ev_side);
    }
    for (hipEvent_t ev : ctx->lane_ev)
        if (ev) hipEventDestroy(ev);
    hipEventDestroy(ctx->ev_fork);
    hipEventDestroy(ctx->ev_join);
    if (ctx->ev_half) hipEventDestroy(ctx->ev_half);
    for (size_t g = 0; g < ctx->group_streams.size(); ++g) {
        hipStreamSynchronize(ctx->group_streams[g]);
        hipStreamDestroy(ctx->group_streams[g]);
        hipEventDestroy(ctx->group_events[g]);
    }
    hipStreamDestroy(ctx->stream2);
    hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return VD_OK;
}

int vd_load_weights(vd_ctx* h, int net, const void* blob, size_t bytes, int fmt) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (fmt != VD_WEIGHTS_VDW1) return vd_set_error(VD_ERR_ARG, "unknown weight format %d", fmt);
    if (!blob) return vd_set_error(VD_ERR_ARG, "null weight blob");
    WMap W;
    int rc = vd_parse_vdw1(blob, bytes, W);
    if (rc) return rc;
    ctx->bands.forget();                          // letterbox bands: nothing written before a load is kept
    if (net == VD_NET_RETINAFACE) {
        if (ctx->face.loaded) return vd_set_error(VD_ERR_STATE, "RetinaFace weights already loaded");
        return vd_build_face(*ctx, W);
    }
    if (net == VD_NET_YOLOV8N) {
        if (ctx->plate.loaded) return vd_set_error(VD_ERR_STATE, "plate weights already loaded");
        return vd_build_plate(*ctx, W);
    }
    return vd_set_error(VD_ERR_ARG, "unknown net %d", net);
}

int vd_set_option(vd_ctx* h, const char* name, int value) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    if (!name) return vd_set_error(VD_ERR_ARG, "null option name");
    struct Opt { const char* n; int VdTune::*f; };
    static const Opt opts[] = {
        {"conv_stream", &VdTune::conv_stream}, {"conv_stream512", &VdTune::conv_stream512},
        {"conv_dual", &VdTune::conv_dual}, {"conv_taps", &VdTune::conv_taps}, {"conv_n192", &VdTune::conv_n192},
        {"conv_small", &VdTune::conv_small}, {"conv_big", &VdTune::conv_big},
        {"conv_big_kmin", &VdTune::conv_big_kmin}, {"stream_ntt", &VdTune::stream_ntt},
        {"lb_pair", &VdTune::lb_pair}, {"mosaic_map", &VdTune::mosaic_map}, {"mosaic_nt", &VdTune::mosaic_nt},
        {"mosaic_cells", &VdTune::mosaic_cells}, {"mosaic_fused", &VdTune::mosaic_fused},
        {"mosaic_rows", &VdTune::mosaic_rows}, {"mosaic_gather", &VdTune::mosaic_gather},
        {"block_fuse", &VdTune::block_fuse}, {"block_fuse32", &VdTune::block_fuse32},
        {"block32_xd", &VdTune::block32_xd}, {"block32_pipe", &VdTune::block32_pipe},
        {"block32_pipe_ds", &VdTune::block32_pipe_ds}, {"chain", &VdTune::chain},
        {"chain_gpw", &VdTune::chain_gpw}, {"stem_pool", &VdTune::stem_pool}, {"ssh_fuse", &VdTune::ssh_fuse},
        {"ssh_side", &VdTune::ssh_side},
        {"plate_s2d", &VdTune::plate_s2d}, {"plate_s2d32", &VdTune::plate_s2d32},
        {"plate_stage", &VdTune::plate_stage}, {"plate_detect_early", &VdTune::plate_detect_early},
        {"mosaic_early", &VdTune::mosaic_early}, {"face_groups", &VdTune::face_groups},
        {"det_group", &VdTune::det_group}, {"f32_split", &VdTune::f32_split}, {"face_bands", &VdTune::face_bands},
        {"x6_small_k", &VdTune::x6_small_k}, {"x6_small_k2", &VdTune::x6_small_k2},
        {"x6_small_tiles", &VdTune::x6_small_tiles}, {"x6_bn256", &VdTune::x6_bn256},
        {"x6_exact", &VdTune::x6_exact}, {"x6_mid", &VdTune::x6_mid}, {"x6_mf32", &VdTune::x6_mf32},
        {"x6_one", &VdTune::x6_one},
        {"x6_stream", &VdTune::x6_stream}, {"x6_stream_silu", &VdTune::x6_stream_silu},
        {"x6_stream_rl", &VdTune::x6_stream_rl}, {"x6_stream256", &VdTune::x6_stream256},
        {"x6_taps", &VdTune::x6_taps},
        {"x6_gemm1x1", &VdTune::x6_gemm1x1}, {"x6_gemm_uni", &VdTune::x6_gemm_uni},
        {"x6_gemm_pf", &VdTune::x6_gemm_pf},
        {"x6_halo", &VdTune::x6_halo}, {"x6_halo_narrow", &VdTune::x6_halo_narrow},
        {"x6_halo_s2", &VdTune::x6_halo_s2}, {"x6_halo_tr", &VdTune::x6_halo_tr},
        {"x6_halo_dma", &VdTune::x6_halo_dma}, {"x6_halo_pf", &VdTune::x6_halo_pf},
        {"x6_halo_1b", &VdTune::x6_halo_1b},
        {"jenc_gpu", &VdTune::jenc_gpu}, {"jdec_gpu", &VdTune::jdec_gpu}, {"jdec_chunk", &VdTune::jdec_chunk},
        {"jdec_sync", &VdTune::jdec_sync}, {"jdec_group", &VdTune::jdec_group},
    };
    for (const Opt& o : opts)
        if (strcmp(o.n, name) == 0) {
            if (!strcmp(name, "stream_ntt") && value != 8 && value != 16)
                return vd_set_error(VD_ERR_ARG, "stream_ntt must be 8 or 16");
            if (!strcmp(name, "x6_gemm_uni") && value != 0 && value != 2)
                return vd_set_error(VD_ERR_ARG, "x6_gemm_uni must be 0 or 2");
            ctx->tune.*(o.f) = value;
            ctx->bands.forget();                  // letterbox bands: a switch may change what a kernel writes
            return VD_OK;
        }
    return vd_set_error(VD_ERR_ARG, "unknown option '%s'", name);
}

int vd_set_stream(vd_ctx* h, void* s) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
    return VD_OK;
}

void* vd_get_stream(vd_ctx* h) { return h ? (void*)((Ctx*)h)->stream : nullptr; }

int vd_sync(vd_ctx* h) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return VD_OK;
}

int vd_timing_enable(vd_ctx* h, int on) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    ctx->timing = on != 0;
    return VD_OK;
}

int vd_timing_reset(vd_ctx* h) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->ev_used = 0;
    return VD_OK;
}

int vd_timing_read(vd_ctx* h, int fam, double* ms, int64_t* launches, double* work) {
    Ctx* ctx = (Ctx*)h;
    VD_ENTRY(ctx);
    VD_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    double tot = 0, wk = 0;
    int64_t cnt = 0;
    for (size_t i = 0; i < ctx->ev_used; ++i) {
        const TimedEv& t = ctx->ev_pool[i];
        if (t.fam != fam) continue;
        float e = 0.f;
        VD_CHECK_HIP(hipEventElapsedTime(&e, t.a, t.b));
        tot += e;
        wk += t.work;
        ++cnt;
    }
    if (ms) *ms = tot;
    if (launches) *launches = cnt;
    if (work) *work = wk;
    return VD_OK;
}

}  // extern "C"
