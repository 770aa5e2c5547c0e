"""Kernel tests on the argument blocks the networks really use: channel slices of wider buffers,
16-bit outputs, res_up, the fused second conv, grouped rows, in-place concats and a frame offset.

Every case goes through vdt_run_op (Context.run_op), which places ONE op in a one-op plan and runs
Ctx::run_ops on it: the argument filling, the range-slot snapshot of an in-place concat, the slot
merge of pool / upsample and the frame offset are the production code. Checked per case:

(a) the output slice of the run frames equals the float64 reference (tests/layout_ref.py) bit for
    bit on integer operands (test_gpu_exact.py's method); with a 16-bit output, the reference
    rounded once to that type. SiLU cases run with ReLU in SiLU's place (bit-equal) and with SiLU
    on the sparse inputs under test_gpu_exact.py's bound 2^-24 (8 + |v|) |ref|; with a 16-bit
    output `got` must lie in [RNE16(RNE32(ref - bound)), RNE16(RNE32(ref + bound))]: the kernel's
    f32 value t is within the bound of ref, t is an f32, and both roundings are monotone.
(b) every other element of the y buffer (other channels, frames outside [f0, f0 + n)) comes back
    bit-identical to the guard pattern it held.
(c) the dispatch record (vd_common.h VdConvFam) names the family the case is written for.
(d) fp16-pair plan: the range slots. A distinct output's slot = max |y slice| of its frame; an
    in-place output's slot = max(x buffer max, |y slice| max); pool / upsample: max(prior slot, x
    slot); slots of frames not run are unchanged.
(e) a random-float leg (operands rounded to the plan's type) against float64, relative to max |y|:
    CONV_TOL[prec] of test_gpu_kernels.py, plus the unit roundoff u of the one extra rounding for a
    16-bit output (2^-8 bf16, 2^-11 fp16). The observed errors are printed.

Final table (family per plan; "a / b": ReLU leg / SiLU leg; "refused": the launcher has no kernel
for the form and the hook returns an error, as a plan with that op would). Read from the launchers
(vd_launch_conv in conv.hip, vd_conv1x1_stream_ok / vd_conv_taps_ok / vd_conv1x1_dual_ok in
conv1x1.hip, vd_conv_big_ok, launch_terms in conv_x6.hip, stream_terms in conv_x6_stream.hip):

bf16 and fp16 contexts, 16-bit output:
  L1   conv_big   the four BIG_CASES, conv_big=1 conv_big_kmin=0 conv_stream=0, plain layout
  L2   conv_big   FPN add (res_up, slices everywhere), conv_big=1 conv_big_kmin=0; M = 480
  L3   stream     ReLU (the ResNet FPN's activation: mode_ok in conv1x1.hip takes no leaky conv, so
                  the issue's act = 2 rows were moved to act = 1); the leaky rows are kept: gemm
  L4   dual       layer1.0 and layer2.0 forms
  L5   taps       C2f m.cv1 / m.cv2 in place (residual = another slice of the y buffer), cc 16 / 32
  L6   gemm       scalar epilogue (ldy 44, ycoff 12, res_coff 4, res_up); also bf16-gemm64 / -gemm128,
                  and with the f32 output of the heads (out16 = 0)
  L7   gemm       SSH conv7x7_3 in place in a 320-wide buffer; MobileNet form (16 -> 16, ReLU as in
                  the plan: the post-concat one) taps
  L8 / L9 / L10   max-pool (SPPF in place, stem), upsample, depthwise (ld = c and c + 8)
fp32 contexts (fp32 | fp32-exact | fp32-x6 | fp32-big | fp32-small):
  P1   x6_halo | gemm | x6_tile | x6_tile | x6_tile     L7's SSH case, and with background +-96
  P2   x6_halo (fp32 only)  grouped rows against groups = 2 and against its two halves
  P3   x6_tr | gemm | x6_tile | x6_tr | x6_tr; x6_gemm1x1=0: x6_tile; res_coff 4: x6_tile (gemm)
  P4   x6_stream | gemm | x6_stream | x6_tr | x6_tr     with and without res_up
  P5   layer1.0: x6_dual | refused | refused | x6_dual | x6_dual; layer2.0: refused everywhere
       (vd_conv1x1_x6_dual_ok takes K 64 + 64 only; the plans run that pair as two convs)
  P6   cc 16: x6_tile / x6_taps | gemm | x6_tile | x6_tile / x6_taps | x6_tile / x6_taps
       cc 32: x6_halo | gemm | x6_tile | x6_tile | x6_tile
  P7   pool / upsample / depthwise on 12 channels at offset 4, with the slot check
  P8   frames [3, 5) of 6-frame buffers: P1's case under the fp32 plans, L2's under bf16 / fp16
       (conv_big) and fp32 (x6_tr)
Depthwise convs have no channel offset in a plan (run_dwconv_op passes 0), so L10 / P7 vary the
channel stride only."""
import numpy as np
import pytest
import torch

import layout_ref as R
from test_gpu_kernels import CONV_TOL, conv_plan

pytestmark = pytest.mark.gpu
F32 = np.float32
HALF = ["bf16", "fp16"]
FP32_PLANS = ["fp32", "fp32-exact", "fp32-x6", "fp32-big", "fp32-small"]
BIG = dict(conv_big=1, conv_big_kmin=0, conv_stream=0)
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
REFUSED = "refused"


def _ctx(factory, prec, options=None):
    cprec, opts = conv_plan(prec, options)
    return cprec, factory(cprec, 8, options=tuple(sorted(opts.items())))


def _rne16(a, cprec, out16=True):
    """float64 -> f32 (exact for the integer legs) -> the output's 16-bit type, as float32."""
    a32 = np.asarray(a, np.float64).astype(F32)
    if cprec == "fp32" or not out16:
        return a32
    return torch.from_numpy(a32).to(torch.bfloat16 if cprec == "bf16" else torch.float16).float().numpy()


def _diff(got, exp):
    bad = np.argwhere(got != exp)
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    return (f"{len(bad)} of {got.size} differ, first at {i}: got {got[i]!r}, expected {exp[i]!r}; "
            f"frames {sorted(set(bad[:, 0]))}, channels {sorted(set(bad[:, -1]))[:12]}")


def _run_conv(ctx, case, pr, act, slope, out16=True):
    kw = R.conv_kwargs(case, pr, act, slope)
    rm = case.dims["rm"]
    if rm and not case.r_is_y:
        kw["res"] = pr["res"]
    return ctx.run_op("conv", pr["x"], None if case.y_is_x else pr["y0"], y_is_x=case.y_is_x,
                      r_is_y=bool(rm and case.r_is_y), out16=out16, **kw)


def _slice_mask(case, shape):
    d = case.dims
    m = np.zeros(shape, bool)
    m[case.f0:case.f0 + d["n"], :, :, case.ycoff:case.ycoff + d["cout"]] = True
    return m


def _check_slots(case, pr, r, what):
    """(d), pair plan only."""
    if r["xslots"] is None:
        return
    d = case.dims
    got = r["y"]
    run = range(case.f0, case.f0 + d["n"])
    xmax = np.abs(pr["x"]).reshape(d["frames"], -1).max(1)
    ymax = np.abs(got[..., case.ycoff:case.ycoff + d["cout"]]).reshape(d["frames"], -1).max(1)
    if case.y_is_x:
        exp = np.array([max(xmax[f], ymax[f]) if f in run else xmax[f] for f in range(d["frames"])], F32)
        assert np.array_equal(r["xslots"], exp), f"{what}: in-place slots {r['xslots']} != {exp}"
        assert np.array_equal(r["yslots"], exp), f"{what}: y view of the in-place slots"
    else:
        exp = np.array([ymax[f] if f in run else 0 for f in range(d["frames"])], F32)
        assert np.array_equal(r["xslots"], xmax.astype(F32)), f"{what}: x slots changed"
        assert np.array_equal(r["yslots"], exp), f"{what}: y slots {r['yslots']} != {exp}"


def _check_conv(ctx, cprec, case, family, out16=True, float_leg=True):
    """(a) - (e) of one conv case in one context. family: a name, (ReLU leg, SiLU leg), or REFUSED."""
    from vdmi import _lib
    d = case.dims
    act = d["act"]
    fams = family if isinstance(family, tuple) else (family, family)
    what = f"{case.name} {cprec}"
    if family == REFUSED:
        with pytest.raises(_lib.VdError):
            _run_conv(ctx, case, R.conv_problem(case, "int"), act, R.SLOPE, out16)
        return
    # integer leg: bit-equal (SiLU cases with ReLU in its place)
    ia = 1 if act == 3 else act
    pr = R.conv_problem(case, "int")
    ref, _ = R.conv_reference(case, "int", ia, R.SLOPE)
    r = _run_conv(ctx, case, pr, ia, R.SLOPE, out16)
    exp = _rne16(ref, cprec, out16)
    mask = _slice_mask(case, exp.shape)
    print(f"{what}: family {r['family']!r} (expected {fams[0]!r})")
    assert np.array_equal(r["y"][mask], exp[mask]), f"{what} (a): " + _diff(np.where(mask, r["y"], 0), np.where(mask, exp, 0))
    assert np.array_equal(r["y"][~mask], exp[~mask]), f"{what} (b): " + _diff(np.where(mask, 0, r["y"]), np.where(mask, 0, exp))
    assert r["family"] == fams[0], f"{what} (c): dispatched to {r['family']!r}, written for {fams[0]!r}"
    _check_slots(case, pr, r, what)
    if act == 3:   # SiLU leg on the sparse inputs, under the derived bound
        pr = R.conv_problem(case, "silu")
        ref, v = R.conv_reference(case, "silu", 3, 0.0)
        r = _run_conv(ctx, case, pr, 3, 0.0, out16)
        sl = (slice(case.f0, case.f0 + d["n"]), slice(None), slice(None), slice(case.ycoff, case.ycoff + d["cout"]))
        bound = 2.0 ** -24 * (8 + np.abs(v)) * np.abs(ref[sl])
        lo, hi = _rne16(ref[sl] - bound, cprec, out16), _rne16(ref[sl] + bound, cprec, out16)
        g = r["y"][sl]
        nz = bound > 0
        if cprec == "fp32" or not out16:
            print(f"{what}: SiLU family {r['family']!r}, max |got - ref| / bound = "
                  f"{(np.abs(g - ref[sl])[nz] / bound[nz]).max():.3f}")
        else:
            print(f"{what}: SiLU family {r['family']!r}, {int((g != _rne16(ref[sl], cprec)).sum())} of {g.size} "
                  f"outputs differ from RNE16(ref) (all within the rounded bound interval or the leg fails)")
        assert np.all((g >= lo) & (g <= hi)), f"{what} SiLU (a): " + _diff(np.clip(g, lo, hi), g)
        e2 = _rne16(ref, cprec, out16)
        assert np.array_equal(r["y"][~mask], e2[~mask]), f"{what} SiLU (b): " + _diff(np.where(mask, 0, r["y"]), np.where(mask, 0, e2))
        assert r["family"] == fams[1], f"{what} SiLU (c): dispatched to {r['family']!r}, written for {fams[1]!r}"
        _check_slots(case, pr, r, what + " SiLU")
    if not float_leg:
        return
    # random-float leg
    pr = R.conv_problem(case, cprec)
    ref, _ = R.conv_reference(case, cprec, act, R.FSLOPE)
    r = _run_conv(ctx, case, pr, act, R.FSLOPE, out16)
    tol = CONV_TOL[cprec] + (U16[cprec] if cprec != "fp32" and out16 else 0.0)
    err = np.abs(r["y"][mask] - ref[mask]).max() / np.abs(ref[mask]).max()
    print(f"{what}: float leg rel err {err:.3e} (tol {tol:.3e})")
    assert err < tol, f"{what} (e): rel err {err} >= {tol}"
    assert np.array_equal(r["y"][~mask], ref[~mask].astype(F32)), f"{what} float (b): " + _diff(
        np.where(mask, 0, r["y"]), np.where(mask, 0, ref.astype(F32)))
    _check_slots(case, pr, r, what + " float")


def _ids(rows):
    return [f"{c.name}-{p}" + ("".join(f"-{k}{v}" for k, v in sorted(o.items())) if o else "") for c, p, o, *_ in rows]


# ------------------------------------------------------------------ bf16 / fp16 contexts
_HALF_ROWS = []
for _p in HALF:
    _HALF_ROWS += [(c, _p, BIG, "conv_big") for c in R.L1]
    _HALF_ROWS += [(R.L2, _p, dict(conv_big=1, conv_big_kmin=0), "conv_big")]
    _HALF_ROWS += [(c, _p, {}, "gemm" if c.name.endswith("leaky") else "stream") for c in R.L3]
    _HALF_ROWS += [(c, _p, {}, "dual") for c in R.L4]
    _HALF_ROWS += [(c, _p, {}, "taps") for c in R.L5]
    _HALF_ROWS += [(R.L6, _p, {}, "gemm"), (R.L7[0], _p, {}, "gemm"), (R.L7[1], _p, {}, "taps")]
    _HALF_ROWS += [(R.P8[1], _p, dict(conv_big=1, conv_big_kmin=0), "conv_big"), (R.P8[0], _p, {}, "gemm")]
_HALF_ROWS += [(R.L6, "bf16-gemm64", {}, "gemm"), (R.L6, "bf16-gemm128", {}, "gemm")]


@pytest.mark.parametrize("case,prec,opts,family", _HALF_ROWS, ids=_ids(_HALF_ROWS))
def test_conv_layout_16bit(gpu, face_ctx_factory, case, prec, opts, family):
    """L1 - L7 (and the frame-offset forms of L2 / L7) with the 16-bit output of the plans."""
    cprec, ctx = _ctx(face_ctx_factory, prec, opts)
    _check_conv(ctx, cprec, case, family)


@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("case,family", [(R.L6, "gemm"), (R.L3[0], "stream")], ids=["L6", "L3.mnet"])
def test_conv_layout_f32_output_of_16bit_plan(gpu, face_ctx_factory, case, family, prec):
    """The same slices with the f32 output the head convs have (out16 = 0): the other arm of
    `if (a.out_f32)` at the strides the 16-bit arm was checked at."""
    cprec, ctx = _ctx(face_ctx_factory, prec)
    _check_conv(ctx, cprec, case, family, out16=False)


def test_run_op_refuses_f32_output_in_a_16bit_buffer(gpu, face_ctx_factory):
    from vdmi import _lib
    _, ctx = _ctx(face_ctx_factory, "bf16")
    for case in (R.L7[0], R.L5[1]):
        with pytest.raises(_lib.VdError, match="out16"):
            _run_conv(ctx, case, R.conv_problem(case, "int"), 1, 0.0, out16=False)


# ------------------------------------------------------------------ fp32 contexts
def _per_plan(cases, fams):
    return [(c, p, {}, f) for c in cases for p, f in zip(FP32_PLANS, fams)]


_TAPS16 = ("x6_tile", "x6_taps")
_FP32_ROWS = (
    _per_plan(R.P1, ["x6_halo", "gemm", "x6_tile", "x6_tile", "x6_tile"])
    + [(R.P2, "fp32", {}, "x6_halo")] + [(c, "fp32", {}, "x6_halo") for c in R.P2_HALVES]
    + _per_plan(R.P3[:1], ["x6_tr", "gemm", "x6_tile", "x6_tr", "x6_tr"])
    + [(R.P3[0], "fp32", dict(x6_gemm1x1=0), "x6_tile")]
    + _per_plan(R.P3[1:], ["x6_tile", "gemm", "x6_tile", "x6_tile", "x6_tile"])
    + _per_plan(R.P4, ["x6_stream", "gemm", "x6_stream", "x6_tr", "x6_tr"])
    + _per_plan(R.L4[:1], ["x6_dual", REFUSED, REFUSED, "x6_dual", "x6_dual"])
    + _per_plan(R.L4[1:], [REFUSED] * 5)
    + _per_plan(R.L5[:2], [_TAPS16, "gemm", "x6_tile", _TAPS16, _TAPS16])
    + _per_plan(R.L5[2:], ["x6_halo", "gemm", "x6_tile", "x6_tile", "x6_tile"])
    + _per_plan(R.P8[:1], ["x6_halo", "gemm", "x6_tile", "x6_tile", "x6_tile"])
    + [(R.P8[1], "fp32", {}, "x6_tr")])


@pytest.mark.parametrize("case,prec,opts,family", _FP32_ROWS, ids=_ids(_FP32_ROWS))
def test_conv_layout_fp32(gpu, face_ctx_factory, case, prec, opts, family):
    """P1 - P6 and P8 under the five fp32 plan names of conv_plan."""
    cprec, ctx = _ctx(face_ctx_factory, prec, opts)
    _check_conv(ctx, cprec, case, family)


@pytest.mark.parametrize("mode", ["silu", "fp32"])
def test_grouped_conv_equals_its_two_halves(gpu, face_ctx_factory, mode):
    """P2: the grouped 3x3 conv (one 64-wide N tile per group) is bit-identical to the two
    64 -> 64 convs run separately on the same buffer (the claim at the plate net's Detect head),
    on the sparse integer inputs and on random f32 operands."""
    _, ctx = _ctx(face_ctx_factory, "fp32")
    case = R.P2
    pr = R.conv_problem(case, mode)
    whole = _run_conv(ctx, case, pr, 3, 0.0)
    assert whole["family"] == "x6_halo"
    y = pr["y0"]
    for g, half in enumerate(R.P2_HALVES):
        kw = R.conv_kwargs(half, dict(pr, w=pr["w"][64 * g:64 * g + 64], scale=pr["scale"][64 * g:64 * g + 64],
                                      shift=pr["shift"][64 * g:64 * g + 64]), 3, 0.0)
        r = ctx.run_op("conv", pr["x"], y, **kw)
        assert r["family"] == "x6_halo"
        y = r["y"]
    assert np.array_equal(whole["y"], y), _diff(whole["y"], y)
    assert np.array_equal(whole["yslots"], np.abs(y[..., 8:136]).reshape(2, -1).max(1))


def test_tr_and_untransposed_tiles_bit_identical(gpu, face_ctx_factory):
    """P3: option x6_gemm1x1 1 (TR tile, register epilogue) and 0 (LDS epilogue) give the same bits
    on random f32 operands, FPN add and slices included."""
    got = {}
    for tr, fam in ((1, "x6_tr"), (0, "x6_tile")):
        _, ctx = _ctx(face_ctx_factory, "fp32", dict(x6_gemm1x1=tr))
        r = _run_conv(ctx, R.P3[0], R.conv_problem(R.P3[0], "fp32"), 2, R.FSLOPE)
        assert r["family"] == fam
        got[tr] = r
    assert np.array_equal(got[1]["y"], got[0]["y"]), _diff(got[1]["y"], got[0]["y"])
    assert np.array_equal(got[1]["yslots"], got[0]["yslots"])


# ------------------------------------------------------------------ pool / upsample / depthwise
_POOL_ROWS = [(c, p) for p in HALF for c in R.L8 + [R.L9]] + [(c, p) for p in ("fp32", "fp32-exact") for c in R.P7_POOL]


@pytest.mark.parametrize("case,prec", _POOL_ROWS, ids=[f"{c.name}-{p}" for c, p in _POOL_ROWS])
def test_pool_upsample_layout(gpu, face_ctx_factory, case, prec):
    """L8 / L9 / P7: bit-exact on random values of the type (frame 0 of a max-pool all negative: a
    zero-padded border would show), the rest of the y buffer untouched, and in the pair plan the
    output's slot = max(prior slot, x slot) for the frames run (in place: unchanged)."""
    cprec, ctx = _ctx(face_ctx_factory, prec)
    pr = R.pool_problem(case, cprec)
    exp = R.pool_reference(case, pr).astype(F32)
    prior = np.array([0.25, 100.0][:case.n], F32)
    for f0, n in ((0, case.n), (case.n - 1, 1)):
        r = ctx.run_op("maxpool" if case.k else "upsample", pr["x"], None if case.y_is_x else pr["y0"],
                       y_is_x=case.y_is_x, xcoff=case.xcoff, ycoff=case.ycoff, ch=case.ch, k=case.k, s=case.s, p=case.p,
                       f0=f0, n=n, yslots=prior)
        e = exp.copy()
        e[:f0] = (pr["x"] if case.y_is_x else pr["y0"])[:f0]
        assert np.array_equal(r["y"], e), f"{case.name} {cprec} frames [{f0}, {f0 + n}): " + _diff(r["y"], e)
        assert r["family"] == ""
        if r["xslots"] is not None:
            xmax = np.abs(pr["x"]).reshape(case.n, -1).max(1).astype(F32)
            assert np.array_equal(r["xslots"], xmax)
            es = xmax if case.y_is_x else np.array([max(prior[f], xmax[f]) if f >= f0 else prior[f]
                                                    for f in range(case.n)], F32)
            assert np.array_equal(r["yslots"], es), f"{case.name}: slots {r['yslots']} != {es}"
        else:
            assert cprec != "fp32" or prec == "fp32-exact"


_DW_ROWS = [(c, p) for p in HALF for c in R.L10] + [(c, p) for p in ("fp32", "fp32-exact") for c in R.P7_DW]


@pytest.mark.parametrize("case,prec", _DW_ROWS, ids=[f"{c.name}-{p}" for c, p in _DW_ROWS])
def test_dwconv_layout(gpu, face_ctx_factory, case, prec):
    """L10 / P7: depthwise 3x3 + BN + leaky, integer operands bit-equal (16-bit: rounded once), the
    channels past c untouched, the pair plan's slot = max |y|; then the random-float leg."""
    cprec, ctx = _ctx(face_ctx_factory, prec)
    c = case.c
    for mode, slope in (("int", R.SLOPE), (cprec, R.FSLOPE)):
        pr = R.dw_problem(case, mode)
        ref, _ = R.dw_reference(case, pr, slope)
        r = ctx.run_op("dwconv", pr["x"], pr["y0"], w=pr["w"], scale=pr["scale"], shift=pr["shift"], stride=case.stride,
                       act=2, slope=slope)
        got = r["y"]
        assert np.array_equal(got[..., c:], pr["y0"][..., c:]), f"{case.name} {cprec} {mode} (b): " + _diff(
            got[..., c:], pr["y0"][..., c:])
        if mode == "int":
            exp = _rne16(ref, cprec)
            assert np.array_equal(got[..., :c], exp[..., :c]), f"{case.name} {cprec} (a): " + _diff(got[..., :c], exp[..., :c])
        else:
            tol = CONV_TOL[cprec] + (U16[cprec] if cprec != "fp32" else 0.0)
            err = np.abs(got[..., :c] - ref[..., :c]).max() / np.abs(ref[..., :c]).max()
            print(f"{case.name} {cprec}: float leg rel err {err:.3e} (tol {tol:.3e})")
            assert err < tol
        if r["yslots"] is not None:
            assert np.array_equal(r["yslots"], np.abs(got[..., :c]).reshape(case.n, -1).max(1))
