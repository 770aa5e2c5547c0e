"""float64 references of the plan ops on whole NHWC buffers, the integer-input generators and
the case tables of tests/test_gpu_layouts.py (checked on the CPU by tests/test_layout_ref.py).

The ops are written in plain numpy (tap loops and matmuls), independent of torch: a conv reads a
channel slice [xcoff, xcoff + cin) of a buffer with channel stride ldx and writes a slice of the y
buffer; everything else of the y buffer is carried over. An output slice inside the x buffer
(in-place concat) and a residual inside the y buffer read the PRIOR contents, which is what the
plans rely on (the slices are disjoint)."""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
SLOPE = 0.5          # leaky slope of the integer legs (exact on multiples of 1/4)
FSLOPE = 0.1         # leaky slope of the random-float legs


# ------------------------------------------------------------------ ops
def act64(v, act, slope):
    return {0: lambda t: t, 1: lambda t: np.maximum(t, 0), 2: lambda t: np.where(t > 0, t, slope * t),
            3: lambda t: t / (1 + np.exp(-t))}[act](np.asarray(v, np.float64))


def conv64(x, w, stride=1, pad=0):
    """x [n,h,w,cin], w [cout,cin,kh,kw] -> [n,oh,ow,cout], float64, zero padding."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, h, wd, cin = x.shape
    cout, cin_w, kh, kw = w.shape
    assert cin == cin_w
    oh, ow = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, cin))
    xp[:, pad:pad + h, pad:pad + wd] = x
    y = np.zeros((n, oh, ow, cout))
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]
            y += patch @ w[:, :, ky, kx].T
    return y


def conv_op(xbuf, ybuf, *, w, scale, shift, xcoff=0, ycoff=0, stride=1, pad=0, act=0, slope=0.0, res=None,
            res_coff=0, res_mode=0, res_up=False, x2=None, w2=None, scale2=None, shift2=None, stride2=1,
            grp_co=0, grp_ci=0, f0=0, n=None):
    """The conv op on whole buffers. Returns (y buffer after the op, pre-activation v of the run
    frames). Row r of a grouped conv reads input channels xcoff + (r // grp_co) * grp_ci + [0, cin);
    res_up: the residual of output pixel (oy, ox) is res[b, oy >> 1, ox >> 1]; the second conv
    (x2: whole buffer, channels [0, cin2), 1x1 at stride2) is summed before the activation."""
    xbuf, out = np.asarray(xbuf, np.float64), np.array(ybuf, np.float64)
    n = xbuf.shape[0] - f0 if n is None else n
    fr = slice(f0, f0 + n)
    cout, cin = w.shape[:2]
    if grp_co:
        v = np.concatenate([conv64(xbuf[fr, :, :, xcoff + g * grp_ci:xcoff + g * grp_ci + cin],
                                   w[g * grp_co:(g + 1) * grp_co], stride, pad) for g in range(cout // grp_co)], -1)
    else:
        v = conv64(xbuf[fr, :, :, xcoff:xcoff + cin], w, stride, pad)
    v = v * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if x2 is not None:
        v2 = conv64(np.asarray(x2, np.float64)[fr, :, :, :w2.shape[1]], w2, stride2, 0)
        v = v + (v2 * np.asarray(scale2, np.float64) + np.asarray(shift2, np.float64))
    oh, ow = v.shape[1:3]
    assert out.shape[1:3] == (oh, ow)
    r = None
    if res_mode:
        r = np.asarray(res, np.float64)[fr, :, :, res_coff:res_coff + cout]
        if res_up:
            r = r[:, np.arange(oh) >> 1][:, :, np.arange(ow) >> 1]
        assert r.shape == v.shape
    if res_mode == 1:
        v = v + r
    t = act64(v, act, slope)
    if res_mode == 2:
        t = t + r
    out[fr, :, :, ycoff:ycoff + cout] = t
    return out, v


def maxpool_op(xbuf, ybuf, *, ch, k, s, p, xcoff=0, ycoff=0, f0=0, n=None):
    """Max-pool of channels [xcoff, xcoff + ch); padded taps are ignored (-inf)."""
    xbuf, out = np.asarray(xbuf, np.float64), np.array(ybuf, np.float64)
    n = xbuf.shape[0] - f0 if n is None else n
    x = xbuf[f0:f0 + n, :, :, xcoff:xcoff + ch]
    h, w = x.shape[1:3]
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    xp = np.full((n, h + 2 * p, w + 2 * p, ch), -np.inf)
    xp[:, p:p + h, p:p + w] = x
    y = np.full((n, oh, ow, ch), -np.inf)
    for ky in range(k):
        for kx in range(k):
            y = np.maximum(y, xp[:, ky:ky + s * (oh - 1) + 1:s, kx:kx + s * (ow - 1) + 1:s])
    out[f0:f0 + n, :, :, ycoff:ycoff + ch] = y
    return out


def upsample_op(xbuf, ybuf, *, ch, xcoff=0, ycoff=0, f0=0, n=None):
    """Nearest 2x: y[b, oy, ox] = x[b, oy >> 1, ox >> 1]."""
    xbuf, out = np.asarray(xbuf, np.float64), np.array(ybuf, np.float64)
    n = xbuf.shape[0] - f0 if n is None else n
    x = xbuf[f0:f0 + n, :, :, xcoff:xcoff + ch]
    out[f0:f0 + n, :, :, ycoff:ycoff + ch] = np.repeat(np.repeat(x, 2, 1), 2, 2)
    return out


def dwconv_op(xbuf, ybuf, *, w, scale, shift, stride=1, act=0, slope=0.0, f0=0, n=None):
    """Depthwise 3x3, pad 1, w [c,3,3], channels [0, c) of both buffers. Returns (y buffer, v)."""
    xbuf, out = np.asarray(xbuf, np.float64), np.array(ybuf, np.float64)
    n = xbuf.shape[0] - f0 if n is None else n
    c = w.shape[0]
    w = np.asarray(w, np.float64).reshape(c, 3, 3)
    x = xbuf[f0:f0 + n, :, :, :c]
    h, wd = x.shape[1:3]
    oh, ow = (h - 1) // stride + 1, (wd - 1) // stride + 1
    xp = np.zeros((n, h + 2, wd + 2, c))
    xp[:, 1:1 + h, 1:1 + wd] = x
    v = np.zeros((n, oh, ow, c))
    for ky in range(3):
        for kx in range(3):
            v += xp[:, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride] * w[:, ky, kx]
    v = v * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    out[f0:f0 + n, :, :, :c] = act64(v, act, slope)
    return out, v


def round16(a, prec):
    """float32 array rounded (RNE) to the 16-bit type of a bf16 / fp16 context; fp32: unchanged."""
    a = np.array(a, F32)
    if prec == "fp32":
        return a
    import torch
    return torch.from_numpy(a).to(torch.bfloat16 if prec == "bf16" else torch.float16).float().numpy()


# ------------------------------------------------------------------ buffer patterns
def guard(shape):
    """Guard pattern of a y buffer: small integers |g| <= 64 that differ between neighbours."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((i * 37) % 129 - 64).astype(F32).reshape(shape)


def background(shape, amp=64):
    """Nonzero integers in [-amp, amp] for the channels of an x buffer outside the slice."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    v = (i * 29) % (2 * amp) - amp
    v[v == 0] = amp
    return v.astype(F32).reshape(shape)


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class ConvCase:
    """shape = (n, h, w, cin, cout, k, stride, pad, act, res_mode); n frames are run, starting at
    f0, in buffers of `frames` frames (default n). ld* None: the plain layout (ld = the slice)."""
    name: str
    shape: tuple
    ldx: int = None
    xcoff: int = 0
    ldy: int = None
    ycoff: int = 0
    res_ld: int = None
    res_coff: int = 0
    res_up: bool = False
    r_is_y: bool = False
    y_is_x: bool = False
    x2: tuple = None            # (cin2, stride2, ldx2, h2, w2)
    grp: tuple = None           # (grp_co, grp_ci)
    frames: int = None
    f0: int = 0
    bg: int = 64                # amplitude of the x buffer's background

    @property
    def dims(self):
        n, h, w, cin, cout, k, s, p, act, rm = self.shape
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        span = cin if not self.grp else (cout // self.grp[0] - 1) * self.grp[1] + cin
        ldx = self.ldx or span
        ldy = ldx if self.y_is_x else (self.ldy or cout)
        frames = self.frames or n
        return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, s=s, p=p, act=act, rm=rm, oh=oh, ow=ow, span=span,
                    ldx=ldx, ldy=ldy, frames=frames, res_ld=self.res_ld or cout,
                    rh=(oh + 1) // 2 if self.res_up else oh, rw=(ow + 1) // 2 if self.res_up else ow)


_PROBLEMS = {}


def conv_problem(case, mode):
    """Seeded inputs of a conv case. mode "int": x in -3..3, weights in {-1, 0, 1} with one all-zero
    row, scales in {0.5, 1, 2}, integer shifts and residuals in -8..8. "silu": the sparse rows
    (4 / scale nonzeros of +-1: |v| <= 16) and the non-negative residual of the SiLU legs.
    "bf16" / "fp16" / "fp32": random operands rounded to that type. Buffers outside the slices hold
    the background / guard patterns. Computed once and shared read-only."""
    key = (case.name, mode)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    d = case.dims
    n, cin, cout, k, K = d["n"], d["cin"], d["cout"], d["k"], d["cin"] * d["k"] ** 2
    fr = d["frames"]
    integer = mode in ("int", "silu")
    rng = np.random.default_rng([ord(c) for c in case.name] + [integer, mode == "silu"])
    rnd = (lambda shape, lo=-3, hi=3: rng.integers(lo, hi + 1, shape).astype(F32)) if integer else \
        (lambda shape, lo=0, hi=0: round16(rng.standard_normal(shape).astype(F32), mode))
    pr = {}
    x = background((fr, d["h"], d["w"], d["ldx"]), case.bg) if integer else rnd((fr, d["h"], d["w"], d["ldx"]))
    x[..., case.xcoff:case.xcoff + d["span"]] = rnd((fr, d["h"], d["w"], d["span"]))
    pr["x"] = x
    if not case.y_is_x:
        pr["y0"] = guard((fr, d["oh"], d["ow"], d["ldy"]))
        if case.r_is_y:
            pr["y0"][..., case.res_coff:case.res_coff + cout] = rnd((fr, d["oh"], d["ow"], cout),
                                                                    0 if mode == "silu" else -8, 8)
    if d["rm"] and not case.r_is_y:
        pr["res"] = rnd((fr, d["rh"], d["rw"], d["res_ld"]), 0 if mode == "silu" else -8, 8)
    if integer:
        scale = rng.choice(np.array([0.5, 1.0, 2.0], F32), cout)
        shift = rng.integers(-4, 5, cout).astype(F32)
        if mode == "silu":
            wt = np.zeros((cout, K), F32)
            for co in range(cout):
                nnz = min(K, int(4 / scale[co]))
                wt[co, rng.choice(K, nnz, replace=False)] = rng.choice(np.array([-1.0, 1.0], F32), nnz)
            wt = wt.reshape(cout, cin, k, k)
        else:
            wt = rng.integers(-1, 2, (cout, cin, k, k)).astype(F32)
        wt[cout // 3] = 0
    else:
        wt = round16((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / K)).astype(F32), mode)
        scale = rng.uniform(0.5, 1.5, cout).astype(F32)
        shift = rng.standard_normal(cout).astype(F32) * F32(0.1)
    pr.update(w=wt, scale=scale, shift=shift)
    if case.x2:
        cin2, stride2, ldx2, h2, w2 = case.x2
        x2 = background((fr, h2, w2, ldx2), case.bg) if integer else rnd((fr, h2, w2, ldx2))
        x2[..., :cin2] = rnd((fr, h2, w2, cin2))
        if integer:
            pr.update(w2=rng.integers(-1, 2, (cout, cin2, 1, 1)).astype(F32),
                      scale2=rng.choice(np.array([0.5, 1.0, 2.0], F32), cout),
                      shift2=rng.integers(-4, 5, cout).astype(F32))
        else:
            pr.update(w2=round16((rng.standard_normal((cout, cin2, 1, 1)) * np.sqrt(2.0 / cin2)).astype(F32), mode),
                      scale2=rng.uniform(0.5, 1.5, cout).astype(F32),
                      shift2=rng.standard_normal(cout).astype(F32) * F32(0.1))
        pr["x2"] = x2
    for a in pr.values():
        a.setflags(write=False)
    _PROBLEMS[key] = pr
    return pr


def conv_kwargs(case, pr, act, slope):
    """The arguments of a case that conv_op and Context.run_op share."""
    d = case.dims
    kw = dict(w=pr["w"], scale=pr["scale"], shift=pr["shift"], xcoff=case.xcoff, ycoff=case.ycoff, stride=d["s"],
              pad=d["p"], act=act, slope=slope, res_coff=case.res_coff, res_mode=d["rm"], res_up=case.res_up,
              f0=case.f0, n=d["n"])
    if case.grp:
        kw.update(grp_co=case.grp[0], grp_ci=case.grp[1])
    if case.x2:
        kw.update(x2=pr["x2"], w2=pr["w2"], scale2=pr["scale2"], shift2=pr["shift2"], stride2=case.x2[1])
    return kw


_REFS = {}


def conv_reference(case, mode, act, slope):
    """(y buffer after the op, pre-activation v), float64, computed once per (case, mode, act)."""
    key = (case.name, mode, act, slope)
    if key not in _REFS:
        pr = conv_problem(case, mode)
        kw = conv_kwargs(case, pr, act, slope)
        ybuf = pr["x"] if case.y_is_x else pr["y0"]
        if case.dims["rm"]:
            kw["res"] = ybuf if case.r_is_y else pr["res"]
        out, v = conv_op(pr["x"], ybuf, **kw)
        out.setflags(write=False)
        v.setflags(write=False)
        _REFS[key] = (out, v)
    return _REFS[key]


BIG_CASES = [(2, 20, 24, 128, 256, 3, 1, 1, 1, 1), (1, 26, 30, 64, 256, 3, 2, 1, 1, 0),
             (1, 33, 31, 256, 512, 1, 1, 0, 0, 2), (2, 9, 11, 512, 256, 3, 1, 1, 2, 0)]   # test_gpu_kernels.BIG_CASES

_FPN = dict(res_up=True, res_ld=320, res_coff=64, ldy=384, ycoff=128, ldx=200, xcoff=72)
_SSH = dict(y_is_x=True, ldx=320, xcoff=192, ycoff=256)
L1 = [ConvCase(f"L1.{i}", c) for i, c in enumerate(BIG_CASES)]
L2 = ConvCase("L2", (2, 12, 20, 128, 256, 1, 1, 0, 2, 2), **_FPN)
L3 = [ConvCase("L3.mnet", (2, 12, 20, 128, 64, 1, 1, 0, 1, 2), res_up=True, res_ld=72, res_coff=8, ldy=136, ycoff=72,
               ldx=136, xcoff=8),
      ConvCase("L3.k512", (1, 8, 10, 512, 256, 1, 1, 0, 1, 2), res_up=True, res_ld=264, res_coff=8, ldy=328, ycoff=72,
               ldx=520, xcoff=8),
      # the issue's act = 2 (leaky) rows: mode_ok (conv1x1.hip) takes no leaky conv, they run the GEMM
      ConvCase("L3.mnet.leaky", (2, 12, 20, 128, 64, 1, 1, 0, 2, 2), res_up=True, res_ld=72, res_coff=8, ldy=136,
               ycoff=72, ldx=136, xcoff=8),
      ConvCase("L3.k512.leaky", (1, 8, 10, 512, 256, 1, 1, 0, 2, 2), res_up=True, res_ld=264, res_coff=8, ldy=328,
               ycoff=72, ldx=520, xcoff=8)]
L4 = [ConvCase("L4.layer1", (2, 9, 11, 64, 256, 1, 1, 0, 1, 0), x2=(64, 1, 64, 9, 11)),
      ConvCase("L4.layer2", (2, 9, 11, 128, 512, 1, 1, 0, 1, 0), x2=(256, 2, 264, 17, 21))]
# C2f: C [2,14,18,4 cc], m.cv1 reads C at cc -> T, m.cv2 reads T -> C at 2 cc with the shortcut C at cc
L5 = [ConvCase("L5.cv1.cc16", (2, 14, 18, 16, 16, 3, 1, 1, 3, 0), ldx=64, xcoff=16),
      ConvCase("L5.cv2.cc16", (2, 14, 18, 16, 16, 3, 1, 1, 3, 2), ldy=64, ycoff=32, res_coff=16, r_is_y=True),
      ConvCase("L5.cv1.cc32", (2, 14, 18, 32, 32, 3, 1, 1, 3, 0), ldx=128, xcoff=32),
      ConvCase("L5.cv2.cc32", (2, 14, 18, 32, 32, 3, 1, 1, 3, 2), ldy=128, ycoff=64, res_coff=32, r_is_y=True)]
L6 = ConvCase("L6", (1, 9, 11, 64, 24, 3, 1, 1, 2, 2), ldy=44, ycoff=12, res_ld=36, res_coff=4, res_up=True)
L7 = [ConvCase("L7.ssh", (2, 7, 9, 64, 64, 3, 1, 1, 2, 0), **_SSH),
      # MobileNet SSH conv7x7_3 (ReLU: the post-concat one): cat = [t5 16 | c3 32 | c7 16 | c5 16 | t7 16]
      ConvCase("L7.mnet", (2, 7, 9, 16, 16, 3, 1, 1, 1, 0), y_is_x=True, ldx=96, xcoff=80, ycoff=48)]
P1 = [L7[0], ConvCase("P1.bg96", (2, 7, 9, 64, 64, 3, 1, 1, 2, 0), bg=96, **_SSH)]
P2 = ConvCase("P2", (2, 6, 10, 64, 128, 3, 1, 1, 3, 0), ldx=136, xcoff=4, ldy=144, ycoff=8, grp=(64, 64))
P2_HALVES = [ConvCase(f"P2.half{g}", (2, 6, 10, 64, 64, 3, 1, 1, 3, 0), ldx=136, xcoff=4 + 64 * g, ldy=144,
                      ycoff=8 + 64 * g) for g in range(2)]
_P3 = dict(res_up=True, res_ld=320, ldy=384, ycoff=128, ldx=1032, xcoff=8)
P3 = [ConvCase("P3", (2, 12, 20, 1024, 256, 1, 1, 0, 2, 2), res_coff=64, **_P3),
      ConvCase("P3.rc4", (2, 12, 20, 1024, 256, 1, 1, 0, 2, 2), res_coff=4, **_P3)]
_P4 = dict(ldx=200, xcoff=72, ldy=384, ycoff=128, res_ld=264, res_coff=8)
P4 = [ConvCase("P4", (2, 9, 11, 128, 256, 1, 1, 0, 1, 1), **_P4),
      ConvCase("P4.up", (2, 9, 11, 128, 256, 1, 1, 0, 1, 1), res_up=True, **_P4)]
P8 = [ConvCase("P8.ssh", (2, 7, 9, 64, 64, 3, 1, 1, 2, 0), frames=6, f0=3, **_SSH),
      ConvCase("P8.fpn", (2, 12, 20, 128, 256, 1, 1, 0, 2, 2), frames=6, f0=3, **_FPN)]
CONV_CASES = L1 + [L2] + L3 + L4 + L5 + [L6] + L7 + P1[1:] + [P2] + P2_HALVES + P3 + P4 + P8


@dataclass(frozen=True)
class PoolCase:
    """Max-pool (k > 0) or nearest 2x upsample (k = 0) of `ch` channels: x [n,h,w,ldx] at xcoff ->
    y at ycoff (y_is_x: of the same buffer)."""
    name: str
    n: int
    h: int
    w: int
    ch: int
    ldx: int
    xcoff: int
    ldy: int
    ycoff: int
    k: int = 0
    s: int = 0
    p: int = 0
    y_is_x: bool = False

    @property
    def out_hw(self):
        if not self.k:
            return 2 * self.h, 2 * self.w
        return (self.h + 2 * self.p - self.k) // self.s + 1, (self.w + 2 * self.p - self.k) // self.s + 1


L8 = [PoolCase("L8.sppf", 2, 7, 9, 32, 128, 0, 128, 32, 5, 1, 2, y_is_x=True),
      PoolCase("L8.stem", 1, 15, 17, 64, 64, 0, 64, 0, 3, 2, 1)]
L9 = PoolCase("L9", 2, 5, 7, 64, 72, 8, 192, 128)
P7_POOL = [PoolCase("P7.pool", 2, 7, 9, 12, 20, 4, 24, 4, 3, 2, 1),
           PoolCase("P7.sppf", 2, 7, 9, 12, 32, 4, 32, 16, 5, 1, 2, y_is_x=True),
           PoolCase("P7.up", 2, 5, 7, 12, 20, 4, 24, 8)]
POOL_CASES = L8 + [L9] + P7_POOL


def pool_problem(case, prec):
    """Random values of the type (pool and upsample are exact on any value); frame 0 of a max-pool
    is all negative, so a zero-padded border would show. The y buffer holds the guard pattern."""
    key = (case.name, prec)
    if key not in _PROBLEMS:
        rng = np.random.default_rng([ord(c) for c in case.name])
        x = rng.standard_normal((case.n, case.h, case.w, case.ldx)).astype(F32) * F32(4)
        if case.k:
            x[0] = -np.abs(x[0]) - F32(0.5)
        x = round16(x, prec)
        pr = dict(x=x)
        if not case.y_is_x:
            pr["y0"] = guard((case.n,) + case.out_hw + (case.ldy,))
        for a in pr.values():
            a.setflags(write=False)
        _PROBLEMS[key] = pr
    return _PROBLEMS[key]


def pool_reference(case, pr):
    ybuf = pr["x"] if case.y_is_x else pr["y0"]
    if case.k:
        return maxpool_op(pr["x"], ybuf, ch=case.ch, k=case.k, s=case.s, p=case.p, xcoff=case.xcoff, ycoff=case.ycoff)
    return upsample_op(pr["x"], ybuf, ch=case.ch, xcoff=case.xcoff, ycoff=case.ycoff)


@dataclass(frozen=True)
class DwCase:
    """Depthwise 3x3 (pad 1, leaky) of channels [0, c) of buffers with channel stride c + extra."""
    name: str
    n: int
    h: int
    w: int
    c: int
    stride: int
    extra: int = 0

    @property
    def out_hw(self):
        return (self.h - 1) // self.stride + 1, (self.w - 1) // self.stride + 1


L10 = [DwCase("L10.s1", 2, 9, 11, 64, 1), DwCase("L10.s1.ld", 2, 9, 11, 64, 1, 8),
       DwCase("L10.s2", 1, 10, 13, 32, 2), DwCase("L10.s2.ld", 1, 10, 13, 32, 2, 8)]
P7_DW = [DwCase("P7.dw.s1", 2, 9, 11, 12, 1, 4), DwCase("P7.dw.s2", 1, 10, 13, 12, 2, 4)]
DW_CASES = L10 + P7_DW


def dw_problem(case, mode):
    """mode "int": x in -3..3, weights in {-1, 0, 1} with one all-zero channel, scales in
    {0.5, 1, 2}, integer shifts; else random operands rounded to the type `mode`."""
    key = (case.name, mode)
    if key not in _PROBLEMS:
        rng = np.random.default_rng([ord(c) for c in case.name] + [mode == "int"])
        ld = case.c + case.extra
        if mode == "int":
            x = background((case.n, case.h, case.w, ld))
            x[..., :case.c] = rng.integers(-3, 4, (case.n, case.h, case.w, case.c))
            w = rng.integers(-1, 2, (case.c, 3, 3)).astype(F32)
            w[case.c // 3] = 0
            scale = rng.choice(np.array([0.5, 1.0, 2.0], F32), case.c)
            shift = rng.integers(-4, 5, case.c).astype(F32)
        else:
            x = round16(rng.standard_normal((case.n, case.h, case.w, ld)).astype(F32), mode)
            w = round16((rng.standard_normal((case.c, 3, 3)) * np.sqrt(2.0 / 9)).astype(F32), mode)
            scale = rng.uniform(0.5, 1.5, case.c).astype(F32)
            shift = rng.standard_normal(case.c).astype(F32) * F32(0.1)
        pr = dict(x=x, y0=guard((case.n,) + case.out_hw + (ld,)), w=w, scale=scale, shift=shift)
        for a in pr.values():
            a.setflags(write=False)
        _PROBLEMS[key] = pr
    return _PROBLEMS[key]


def dw_reference(case, pr, slope):
    return dwconv_op(pr["x"], pr["y0"], w=pr["w"], scale=pr["scale"], shift=pr["shift"], stride=case.stride, act=2,
                     slope=slope)
