"""Bit-exact checks of the conv and bottleneck kernels (through the C-ABI test hooks).

test_gpu_kernels.py holds the 16-bit paths to 2e-2 of max|y| and draws every frame of a
batch from one distribution, so a dropped K element, a dropped channel or a per-frame
scale taken from the wrong frame passes there. Here the arithmetic is made exact, so no
tolerance is needed:

A / B. Integer-valued operands. Small integer activations, weights in {-1, 0, 1},
   power-of-two BN scales, integer shifts and residuals: every product and every partial
   sum is an integer (times 1/4 at most) below 2^24, exact in bf16, in fp16, in the
   exact-f32 MFMA, in the 3-term bf16 split and in the fp16 pair (hi exact, lo zero;
   vd_pack_x3h and act_scale_exp_of scale by powers of two only), in every summation
   order. The result equals the float64 reference bit for bit.
C. A frame scaled by 2^j. Scaling commutes with every rounding of every path while
   nothing under- or overflows, and in the pair path the exponent follows the frame's
   own max, so the fp16 bit patterns do not move. With zero BN shift and a positively
   homogeneous activation, frame b of a batch of mixed magnitudes equals
   ldexp(the unscaled frame run alone, j[b]) bit for bit. The hook's own check of the
   per-frame output max slots then sees a different value in every slot.

Which kernel a case reaches was read from the launchers (vd_launch_conv in conv.hip,
launch_terms in conv_x6.hip, vd_conv1x1_stream_ok / vd_conv_taps_ok in conv1x1.hip,
vd_conv_big_ok in conv_big.hip) and is noted at the cases.

The phased 256 x 256 kernel (conv_big.hip) is NOT reached by any case here or in
test_conv_big_matches_torch: vdt_conv2d asks for the f32 accumulator (out_f32 = 1) and
vd_conv_big_ok refuses out_f32, so the BIG_CASES options (conv_big = 1, conv_big_kmin = 0,
conv_stream = 0) leave those shapes on the bf16 implicit GEMM of conv.hip. The legs are
kept (they are GEMM coverage at K up to 4608) under that name. Their sibling
test_gpu_layouts.py runs the same shapes and options through vdt_run_op with the 16-bit
output of the plans, reaches conv_big.hip and asserts so (the dispatch record); it also
takes this file's method to channel slices, res_up, the fused second conv, grouped rows,
in-place concats and frame offsets."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import (BIG_CASES, BLOCK_CASES, CONV_CASES, CONV_PRECS, CONV_TOL, S2_CASES, TR_CASES,
                              conv_plan)

pytestmark = pytest.mark.gpu
F32 = np.float32
SLOPE = 0.5

# the existing tests run these at workload size; the reference alone would take too long here
_TOO_BIG = {(4, 224, 224, 32, 256, 3, 2, 1, 1, 0), (2, 45, 47, 512, 2048, 1, 1, 0, 1, 1),
            (1, 77, 79, 1024, 2048, 1, 1, 0, 1, 1)}
BIG_OPTIONS = dict(conv_big=1, conv_big_kmin=0, conv_stream=0)


def _conv64(x, wt, s, p):
    """NHWC float64 convolution (torch CPU, float64 throughout)."""
    y = torch.nn.functional.conv2d(torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2),
                                   torch.from_numpy(np.asarray(wt, np.float64)), stride=s, padding=p)
    return y.permute(0, 2, 3, 1).numpy()


def _act64(v, act, slope):
    return {0: lambda t: t, 1: lambda t: np.maximum(t, 0), 2: lambda t: np.where(t > 0, t, slope * t),
            3: lambda t: t / (1 + np.exp(-t))}[act](v)


# ------------------------------------------------------------------ A. integer-exact conv
_INT_REF = {}


def _int_problem(case, silu):
    """Seeded integer inputs of a case and its exact reference, computed once and shared by
    the prec legs (read-only). silu: the sparse weights and non-negative residual of the
    SiLU legs (see test_conv_integer_exact)."""
    key = (case, silu)
    if key in _INT_REF:
        return _INT_REF[key]
    n, h, w, cin, cout, k, s, p, act, res_mode = case
    rng = np.random.default_rng([n, h, w, cin, cout, k, s, p, res_mode, int(silu)])
    x = rng.integers(-3, 4, (n, h, w, cin)).astype(F32)
    scale = rng.choice(np.array([0.5, 1.0, 2.0], F32), cout)
    shift = rng.integers(-4, 5, cout).astype(F32)
    K = cin * k * k
    if silu:
        # 4 / scale nonzeros of +-1 per row: |v| <= scale * 3 * nnz + 4 = 16
        wt = np.zeros((cout, K), F32)
        for co in range(cout):
            nnz = min(K, int(4 / scale[co]))
            wt[co, rng.choice(K, nnz, replace=False)] = rng.choice(np.array([-1.0, 1.0], F32), nnz)
        wt = wt.reshape(cout, cin, k, k)
    else:
        wt = rng.integers(-1, 2, (cout, cin, k, k)).astype(F32)
    wt[cout // 3] = 0          # row max 0: vd_pack_x3h takes e = 0, the output is act(shift (+ res))
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    res = rng.integers(0 if silu else -8, 9, (n, oh, ow, cout)).astype(F32) if res_mode else None
    v = _conv64(x, wt, s, p) * scale + shift
    if res_mode == 1:
        v = v + res
    # conditions on the inputs (not tolerances): multiples of 1/4 below 2^24 / 4, exact in f32
    assert np.array_equal(v * 4, np.round(v * 4))
    assert np.abs(v).max() <= 2 * 3 * K + 12 and (2 * 3 * K + 12) * 4 < 2 ** 24
    if silu:
        assert np.abs(v).max() <= 16
    prob = dict(x=x, wt=wt, scale=scale, shift=shift, res=res, v=v)
    for a in prob.values():
        if a is not None:
            a.setflags(write=False)
    _INT_REF[key] = prob
    return prob


def _run(ctx, case, pr, act):
    n, h, w, cin, cout, k, s, p, _, res_mode = case
    return ctx.conv2d(pr["x"], pr["wt"], s, p, pr["scale"], pr["shift"], act, SLOPE, pr["res"], res_mode)


def _check_integer_exact(face_ctx_factory, prec, case, options=None):
    """Assertion 1 on the legs with act in {none, ReLU, leaky}; the SiLU cases run twice:
    with ReLU in SiLU's place on the dense inputs (bit-equal), and with SiLU on the sparse
    ones against float64 SiLU of the exact pre-activation v under
        |got - ref| <= 2^-24 (8 + |v|) |ref|.
    act_apply computes v / (1 + __expf(-v)): t = RN(-v log2e) moves the exponent by at most
    |t| 2^-24, i.e. exp(-v) by a relative |v| ln2 log2e 2^-24 = |v| 2^-24 (plus 0.22 |v| 2^-24
    for log2e's own f32 rounding); v_exp_f32 is good to 1 ulp = 2 x 2^-24; the add and the
    divide round once each, 2^-24 together with the exponential's weight e / (1 + e) <= 1.
    That is (1.22 |v| + 4) 2^-24 <= (8 + |v|) 2^-24 for |v| <= 16, which the inputs keep
    (asserted on the reference). Where the residual is added after the activation its sign
    is kept non-negative on this leg, so |ref| >= |SiLU(v)| (SiLU > -0.28, res an integer
    >= 0; asserted) and the bound on the sum is no looser than the one on SiLU itself; the
    last add's rounding (2^-24 |ref|) fits the slack for |v| <= 13 and is within it in
    practice: the largest observed ratio is printed.

    Does the activation change the kernel family? Read from the launchers: not in the
    bf16 / fp16 plans (mode_ok in conv1x1.hip takes ReLU wherever it takes SiLU, at both
    residual modes these cases use; vd_conv_big_ok and the GEMM do not look at it), not in
    the exact-f32 MFMA and not in the 3-term split (launch_terms<3>). It DOES in the
    fp16-pair plan: launch_taps_x6 and the x6_stream_silu branch of launch_terms<2> take
    SiLU only, so under the fp32 pair names the ReLU leg of a SiLU case runs the GEMM /
    halo / streaming form that takes the shape over, and the SiLU leg is the one that
    reaches the streaming-taps and SiLU-streaming kernels (its bound, ~1e-6 of |ref|, is
    far below the 1/4 a dropped or misplaced term moves v by)."""
    cprec, opts = conv_plan(prec, options)
    ctx = face_ctx_factory(cprec, 8, options=tuple(sorted(opts.items())))
    act, res_mode = case[8], case[9]
    pr = _int_problem(case, False)
    got = _run(ctx, case, pr, 1 if act == 3 else act)
    ref = _act64(pr["v"], 1 if act == 3 else act, SLOPE)
    if res_mode == 2:
        ref = ref + pr["res"]
    assert got.shape == ref.shape
    assert np.array_equal(got, ref.astype(F32)), _diff(got, ref)
    if act != 3:
        return
    pr = _int_problem(case, True)
    got = _run(ctx, case, pr, 3).astype(np.float64)
    v = pr["v"]
    silu = _act64(v, 3, SLOPE)
    ref = silu + pr["res"] if res_mode == 2 else silu
    assert np.all(np.abs(ref) >= np.abs(silu))
    bound = 2.0 ** -24 * (8 + np.abs(v)) * np.abs(ref)
    err = np.abs(got - ref)
    nz = bound > 0
    print(f"SiLU {prec} {case}: max |got - ref| / bound = {(err[nz] / bound[nz]).max():.3f}")
    assert np.all(err <= bound), _diff(got, ref)


def _diff(got, ref):
    bad = np.argwhere(got != ref.astype(got.dtype))
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return f"{len(bad)} of {got.size} differ, first at {i}: got {got[i]!r}, ref {ref[i]!r}; channels {sorted(set(bad[:, -1]))[:8]}"


@pytest.mark.parametrize("prec", CONV_PRECS)
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_integer_exact(gpu, face_ctx_factory, prec, case):
    """Every plan name of test_conv_matches_torch on every CONV_CASES shape, integer
    operands, equal to the float64 reference bit for bit (_check_integer_exact)."""
    _check_integer_exact(face_ctx_factory, prec, case)


@pytest.mark.parametrize("case", BIG_CASES)
def test_conv_big_options_integer_exact(gpu, face_ctx_factory, case):
    """BIG_CASES under the options of test_conv_big_matches_torch, bf16. Through the hook
    these run conv.hip's implicit GEMM, not conv_big.hip (module docstring);
    test_gpu_layouts.py::test_conv_layout_16bit[L1.*] is the leg that does."""
    _check_integer_exact(face_ctx_factory, "bf16", case, BIG_OPTIONS)


@pytest.mark.parametrize("s2", [1, 0])
@pytest.mark.parametrize("case", [c for c in S2_CASES if c not in _TOO_BIG])
def test_conv_halo_s2_integer_exact(gpu, face_ctx_factory, case, s2):
    """Stride-2 3x3 convs on the phase halos (x6_halo_s2 = 1: conv_x6_halo_kernel<.., S2>)
    and on the tap-major tiles they replace (0)."""
    _check_integer_exact(face_ctx_factory, "fp32", case, dict(x6_halo_s2=s2))


@pytest.mark.parametrize("uni", [2, 0])
@pytest.mark.parametrize("tr", [1, 0])
@pytest.mark.parametrize("case", [c for c in TR_CASES if c not in _TOO_BIG])
def test_conv_tr_tiles_integer_exact(gpu, face_ctx_factory, case, tr, uni):
    """1x1 convs on the TR tiles (x6_gemm1x1 = 1) and the untransposed ones (0), with the
    one-barrier K loop (x6_gemm_uni = 2) and the general loop (0); streaming form off."""
    _check_integer_exact(face_ctx_factory, "fp32", case, dict(x6_gemm1x1=tr, x6_gemm_uni=uni, x6_stream=0))


# ------------------------------------------------------------------ B. integer-exact bottleneck
def _sparse_rows(rng, co, ci, k):
    """Every row: exactly four nonzeros of +-1 at random positions."""
    wt = np.zeros((co, ci * k * k), F32)
    for r in range(co):
        wt[r, rng.choice(ci * k * k, 4, replace=False)] = rng.choice(np.array([-1.0, 1.0], F32), 4)
    return wt.reshape(co, ci, k, k)


def _bottleneck64(x, w1, b1, w2, b2, w3, b3, wd, bd):
    """float64 bottleneck; returns (t1, t2, out), NHWC."""
    aff = lambda v, b: v * b[:len(b) // 2].astype(np.float64) + b[len(b) // 2:].astype(np.float64)
    t1 = np.maximum(aff(_conv64(x, w1, 1, 0), b1), 0)
    t2 = np.maximum(aff(_conv64(t1, w2, 1, 1), b2), 0)
    idt = aff(_conv64(x, wd, 1, 0), bd) if wd is not None else np.asarray(x, np.float64)
    return t1, t2, np.maximum(aff(_conv64(t2, w3, 1, 0), b3) + idt, 0)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("case", [c for c in BLOCK_CASES if c != (8, 96, 160, 256, False)])
def test_bottleneck_integer_exact(gpu, face_ctx_factory, prec, case):
    """block.hip (bf16) / block32.hip (fp32), the conv-by-conv chain and the float64
    reference agree bit for bit on integer operands: x in [0, 3], four +-1 per weight row,
    BN scale 1, shifts in [-2, 2], so t1 <= 14, t2 <= 58, out <= 248: integers below 2^8,
    exact in bf16 (t1, t2 and the bf16 plan's output are stored in it) and in block32's
    per-tile-scaled pairs (a tile whose t1 or t2 is all zero takes exponent 0).

    vdt_bottleneck never falls back: with fused = 1 it returns an error unless
    Ctx::block_ok holds, and vd_block_ok / vd_block32_ok accept (cin 256, no downsample) and
    (cin 64, downsample) at any h, w below 2 GiB per frame, which is every BLOCK_CASES
    shape: all five cases here run the fused kernel. The hook refuses fp16 contexts
    ("bf16 or fp32 (fp16-pair) contexts only"), so there is no fp16 leg."""
    n, h, w, cin, ds = case
    ctx = face_ctx_factory(prec, 8)
    rng = np.random.default_rng([n, h, w, cin, int(ds)])
    x = rng.integers(0, 4, (n, h, w, cin)).astype(F32)
    bn = lambda c: np.concatenate([np.ones(c), rng.integers(-2, 3, c)]).astype(F32)
    w1, w2, w3 = _sparse_rows(rng, 64, cin, 1), _sparse_rows(rng, 64, 64, 3), _sparse_rows(rng, 256, 64, 1)
    b1, b2, b3 = bn(64), bn(64), bn(256)
    wd, bd = (_sparse_rows(rng, 256, cin, 1), bn(256)) if ds else (None, None)
    t1, t2, ref = _bottleneck64(x, w1, b1, w2, b2, w3, b3, wd, bd)
    assert t1.max() <= 256 and t2.max() <= 256 and ref.max() <= 256 and ref.max() > 0
    fused = ctx.bottleneck(x, w1, b1, w2, b2, w3, b3, wd, bd, fused=True)
    chain = ctx.bottleneck(x, w1, b1, w2, b2, w3, b3, wd, bd, fused=False)
    assert np.array_equal(chain, ref.astype(F32)), "chain: " + _diff(chain, ref)
    assert np.array_equal(fused, ref.astype(F32)), "fused: " + _diff(fused, ref)


# ------------------------------------------------------------------ C. per-frame scale
# exponents of the four frames (None: an all-zero frame); the 16-bit contexts keep within
# their type's range
J32 = (0, -40, 40, None)
J16 = (0, 3, 6, None)

# (case, [(prec name, extra options)]) -- the kernel each leg reaches, from the launchers:
SCALE_CASES = [
    # conv_x6_kernel, the 128-row one-stage (fp32-small: <128, 64, 256, 1>) and 256-row two-stage
    # (fp32-big: <256, 64, 512, 2>) GEMM tiles; M = 140, so one tile holds all four frames. 16-bit:
    # leaky is not a streaming mode (mode_ok), so the implicit GEMM of conv.hip.
    ((4, 5, 7, 64, 64, 1, 1, 0, 2, 1), [("fp32-small", {}), ("fp32-big", {}), ("fp32-exact", {}), ("fp32-x6", {})]),
    # conv1x1_x6_kernel, K = 128, RL form (ReLU + residual): 128-channel slices <4, 8> (fp32-s128) and
    # 256-channel ones <4, 16> (fp32-s256); 16-row pixel groups straddle the 30-row frames.
    # 16-bit: conv1x1.hip launch_mode<4, 16>.
    ((4, 5, 6, 128, 256, 1, 1, 0, 1, 1), [("fp32-s128", {}), ("fp32-s256", {}), ("fp32-x6", {})]),
    # TR tiles: launch_tr -> conv_x6_kernel<256, 128, 512, 2, 2, 16, true> (t256 < 192, Cout 256), one-barrier
    # and general K loops; M = 168. 16-bit: the streaming kernel at K = 512, launch_mode<16, 8>.
    ((4, 6, 7, 512, 256, 1, 1, 0, 1, 2), [("fp32", dict(x6_gemm1x1=1, x6_stream=0, x6_gemm_uni=2)),
                                          ("fp32", dict(x6_gemm1x1=1, x6_stream=0, x6_gemm_uni=0))]),
    # halo form, stride 1: x6_halo_narrow -> conv_x6_halo_kernel<32, 3, ...> (default) and <32, 2, ...>
    # (fp32-halo1); M = 252: one tile, whose halo indexes xmax for four frames. 16-bit: GEMM <64, 32>.
    ((4, 7, 9, 64, 32, 3, 1, 1, 2, 1), [("fp32", {}), ("fp32-halo1", {}), ("fp32-exact", {})]),
    # phase halo, stride 2: conv_x6_halo_kernel<64, 3, .., S2> (x6_halo_s2 = 1), else the small GEMM tile
    # <128, 64, 256, 1>. 16-bit: streaming taps (kpad 320, launch_taps_n<10>).
    ((4, 9, 9, 32, 64, 3, 2, 1, 1, 0), [("fp32", dict(x6_halo_s2=1)), ("fp32", dict(x6_halo_s2=0))]),
    # stem loader: cin_pad 4, kpad 224: conv_x6_kernel<128, 64, 256, 1> with the generic tap loader.
    # 16-bit: cin_pad 8, not dense, kpad 448: the GEMM's generic loader.
    ((4, 12, 10, 3, 64, 7, 2, 3, 1, 0), [("fp32", {})]),
    # streaming taps: the 16-bit legs reach conv1x1.hip's taps kernel (kpad 192, launch_taps_n<6>, ReLU with the
    # residual after it). The fp32 plan's taps form takes SiLU only (launch_taps_x6), which is not homogeneous:
    # with ReLU this shape runs conv_x6_kernel<128, 32, 256, 1>; test_conv_taps_silu_frame_alone covers the form.
    ((4, 6, 8, 16, 32, 3, 1, 1, 1, 2), [("fp32", {})]),
    # tile seams inside frames: conv_x6_halo_kernel<128, ...>, M = 1200 in five tiles over 400-row frames
    # (three frames: exponents -40, +40 and the zero frame). 16-bit: GEMM <64, 128>.
    ((3, 20, 20, 64, 128, 3, 1, 1, 0, 0), [("fp32", {}), ("fp32-big", {})]),
    # the BIG_CASES options, bf16 only: conv.hip's GEMM (module docstring), K = 1152
    ((4, 6, 6, 128, 256, 3, 1, 1, 1, 1), [("bf16", BIG_OPTIONS)]),
]
# the 16-bit default dispatch and the forced GEMMs on every shape
_SCALE_LEGS = [(case, prec, opts) for case, legs in SCALE_CASES for prec, opts in
               legs + ([] if legs[0][0] == "bf16" else [("bf16", {}), ("fp16", {}), ("bf16-gemm64", {}),
                                                        ("bf16-gemm128", {})])]


def _round16(a, cprec):
    """Round to the context's 16-bit type (fp32: unchanged); fp16 subnormals are dropped so
    that the scaled and the unscaled frame meet the same (normal) values."""
    if cprec == "fp32":
        return a
    dt = torch.bfloat16 if cprec == "bf16" else torch.float16
    r = torch.from_numpy(np.ascontiguousarray(a, F32)).to(dt).float().numpy()
    if cprec == "fp16":
        r[np.abs(r) < 2.0 ** -14] = 0
    return r


def _mixed(base, js):
    """frame b = base[b] * 2^j[b] (exact), or zeros."""
    out = np.zeros_like(base)
    for b, j in enumerate(js):
        if j is not None:
            out[b] = np.ldexp(base[b], j)
    return out


@pytest.mark.parametrize("case,prec,opts", _SCALE_LEGS,
                         ids=[f"{'x'.join(map(str, c))}-{p}-{'-'.join(f'{k}{v}' for k, v in sorted(o.items()))}"
                              for c, p, o in _SCALE_LEGS])
def test_conv_frame_scale(gpu, face_ctx_factory, case, prec, opts):
    """Four frames of one batch at 2^0, 2^-40 (2^3), 2^+40 (2^6) and all zero: frame b of
    the batch equals ldexp(the base frame run alone, j[b]) bit for bit, the zero frame's
    output is zero, and the frame run alone is within the existing tolerance (CONV_TOL)
    of the float64 convolution. Zero BN shift; the residual carries its frame's factor."""
    n, h, w, cin, cout, k, s, p, act, res_mode = case
    cprec, opts = conv_plan(prec, opts)
    ctx = face_ctx_factory(cprec, 8, options=tuple(sorted(opts.items())))
    js = (J32 if cprec == "fp32" else J16)[-n:]
    rng = np.random.default_rng([n, h, w, cin, cout, k])
    x = _round16(rng.standard_normal((n, h, w, cin)).astype(F32), cprec)
    wt = _round16((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(F32), cprec)
    scale = rng.uniform(0.5, 1.5, cout).astype(F32)
    shift = np.zeros(cout, F32)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    res = _round16(rng.standard_normal((n, oh, ow, cout)).astype(F32), cprec) if res_mode else None
    full = ctx.conv2d(_mixed(x, js), wt, s, p, scale, shift, act, SLOPE, None if res is None else _mixed(res, js),
                      res_mode)
    y = _conv64(x, wt, s, p) * scale
    if res_mode == 1:
        y = y + res
    y = _act64(y, act, SLOPE)
    if res_mode == 2:
        y = y + res
    for b, j in enumerate(js):
        if j is None:
            assert not full[b].any(), f"frame {b} (zero input) has nonzero output"
            continue
        alone = ctx.conv2d(x[b:b + 1], wt, s, p, scale, shift, act, SLOPE, None if res is None else res[b:b + 1],
                           res_mode)[0]
        assert np.abs(alone - y[b]).max() / np.abs(y[b]).max() < CONV_TOL[cprec]
        assert np.array_equal(full[b], np.ldexp(alone, j)), f"frame {b} (2^{j}): " + _diff(full[b], np.ldexp(alone, j))


@pytest.mark.parametrize("prec", ["fp32", "fp32-big"])
def test_conv_taps_silu_frame_alone(gpu, face_ctx_factory, prec):
    """The fp32 plan's streaming-taps form (launch_taps_x6: SiLU only; ks = 5, Cout 32 ->
    conv1x1_x6_kernel<5, 2, SILU, POST_ACT, 2, TAPS>) cannot take the ldexp check, SiLU
    not being homogeneous. Its per-frame exponents are checked the other way round: every
    frame of the mixed-magnitude batch equals the same (scaled) frame run alone."""
    n, h, w, cin, cout, k, s, p = 4, 6, 8, 16, 32, 3, 1, 1
    cprec, opts = conv_plan(prec)
    ctx = face_ctx_factory(cprec, 8, options=tuple(sorted(opts.items())))
    rng = np.random.default_rng(168)
    x = _mixed(rng.standard_normal((n, h, w, cin)).astype(F32), J32)
    wt = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(F32)
    scale = rng.uniform(0.5, 1.5, cout).astype(F32)
    shift = rng.standard_normal(cout).astype(F32) * F32(0.1)
    res = _mixed(rng.standard_normal((n, h, w, cout)).astype(F32), J32)
    full = ctx.conv2d(x, wt, s, p, scale, shift, 3, 0.0, res, 2)
    for b in range(n):
        alone = ctx.conv2d(x[b:b + 1], wt, s, p, scale, shift, 3, 0.0, res[b:b + 1], 2)[0]
        assert np.array_equal(full[b], alone), f"frame {b}: " + _diff(full[b], alone)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [(4, 13, 18, 64, True), (4, 21, 37, 256, False)])
def test_bottleneck_frame_scale(gpu, face_ctx_factory, prec, case):
    """The four-frame construction through ctx.bottleneck, zero BN shifts: the fused kernel
    (block32.hip / block.hip) and the conv-by-conv chain are each bit-equal to ldexp of the
    frame run alone in the same mode. The unfused fp32 chain hands each conv's ymax slots
    to the next conv as xmax (the only kernel-level check of that hand-over)."""
    n, h, w, cin, ds = case
    ctx = face_ctx_factory(prec, 8)
    js = J32 if prec == "fp32" else J16
    rng = np.random.default_rng([n, h, w, cin, 3])
    he = lambda co, ci, k: (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(F32)
    bn = lambda c: np.concatenate([rng.uniform(0.5, 1.5, c), np.zeros(c)]).astype(F32)
    x = _round16(np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(F32), prec)
    args = [he(64, cin, 1), bn(64), he(64, 64, 3), bn(64), he(256, 64, 1), bn(256)]
    args += [he(256, cin, 1), bn(256)] if ds else [None, None]
    for fused in (True, False):
        full = ctx.bottleneck(_mixed(x, js), *args, fused=fused)
        for b, j in enumerate(js):
            if j is None:
                assert not full[b].any(), f"fused={fused}: frame {b} (zero input) has nonzero output"
                continue
            alone = ctx.bottleneck(x[b:b + 1], *args, fused=fused)[0]
            assert alone.any()
            assert np.array_equal(full[b], np.ldexp(alone, j)), \
                f"fused={fused} frame {b} (2^{j}): " + _diff(full[b], np.ldexp(alone, j))
