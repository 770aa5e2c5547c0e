"""CPU checks of tests/layout_ref.py: the numpy references equal torch's own ops bit for bit, and
every case of tests/test_gpu_layouts.py meets the input conditions its exactness argument needs
(on the reference alone; no GPU)."""
import numpy as np
import pytest
import torch

import layout_ref as R

F = torch.nn.functional


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _dyadic(rng, shape):
    """float64 multiples of 1/8 in [-4, 4]: sums of a few thousand products are exact in any order,
    so "equal to the bit" does not depend on either side's summation order."""
    return rng.integers(-32, 33, shape).astype(np.float64) / 8


@pytest.mark.parametrize("stride,pad,k", [(1, 1, 3), (2, 1, 3), (1, 0, 1), (2, 3, 7)])
def test_conv64_equals_torch(stride, pad, k):
    rng = np.random.default_rng(k * 10 + stride)
    x, w = _dyadic(rng, (2, 9, 11, 6)), _dyadic(rng, (5, 6, k, k))
    ref = _nhwc(F.conv2d(_nchw(x), torch.from_numpy(w), stride=stride, padding=pad))
    assert np.array_equal(R.conv64(x, w, stride, pad), ref)


def test_grouped_conv_op_equals_torch_groups():
    """conv_op with grp_co / grp_ci = the group widths, on a slice of wider buffers, against
    torch conv2d(groups=2) on the slice."""
    rng = np.random.default_rng(2)
    xbuf, ybuf = _dyadic(rng, (2, 6, 10, 20)), _dyadic(rng, (2, 6, 10, 16))
    w = _dyadic(rng, (8, 6, 3, 3))
    scale, shift = np.ones(8), np.zeros(8)
    out, v = R.conv_op(xbuf, ybuf, w=w, scale=scale, shift=shift, xcoff=4, ycoff=8, pad=1, grp_co=4, grp_ci=6)
    ref = _nhwc(F.conv2d(_nchw(xbuf[..., 4:16]), torch.from_numpy(w), padding=1, groups=2))
    assert np.array_equal(v, ref) and np.array_equal(out[..., 8:], ref)
    assert np.array_equal(out[..., :8], ybuf[..., :8])
    # overlapping / strided groups are the general form: group 1 two channels on
    o2, _ = R.conv_op(xbuf, ybuf, w=w, scale=scale, shift=shift, xcoff=4, ycoff=8, pad=1, grp_co=4, grp_ci=2)
    assert np.array_equal(o2[..., 12:], _nhwc(F.conv2d(_nchw(xbuf[..., 6:12]), torch.from_numpy(w[4:]), padding=1)))


def test_conv_op_residual_second_conv_and_frames():
    """BN, the residual before / after the activation from a slice, res_up as res[b, oy >> 1, ox >> 1]
    (F.interpolate nearest), the second conv summed before the activation, and the frame window."""
    rng = np.random.default_rng(3)
    xbuf, ybuf = _dyadic(rng, (4, 5, 7, 12)), _dyadic(rng, (4, 5, 7, 10))
    res, x2 = _dyadic(rng, (4, 3, 4, 9)), _dyadic(rng, (4, 9, 13, 6))
    w, w2 = _dyadic(rng, (4, 8, 1, 1)), _dyadic(rng, (4, 5, 1, 1))
    sc, sh, sc2, sh2 = (rng.choice([0.5, 1.0, 2.0], 4), _dyadic(rng, 4), rng.choice([0.5, 1.0, 2.0], 4), _dyadic(rng, 4))
    up = _nhwc(F.interpolate(_nchw(res[..., 3:7]), size=(5, 7), mode="nearest"))
    base = _nhwc(F.conv2d(_nchw(xbuf[..., 2:10]), torch.from_numpy(w))) * sc + sh
    base2 = base + _nhwc(F.conv2d(_nchw(x2[..., :5]), torch.from_numpy(w2), stride=2)) * sc2 + sh2
    for rm in (1, 2):
        out, v = R.conv_op(xbuf, ybuf, w=w, scale=sc, shift=sh, xcoff=2, ycoff=6, act=2, slope=0.5, res=res, res_coff=3,
                           res_mode=rm, res_up=True, f0=1, n=2)
        pre = base + up if rm == 1 else base
        exp = np.where(pre > 0, pre, 0.5 * pre) + (up if rm == 2 else 0)
        assert np.array_equal(v, pre[1:3]) and np.array_equal(out[1:3, ..., 6:], exp[1:3])
        assert np.array_equal(out[[0, 3]], ybuf[[0, 3]]) and np.array_equal(out[..., :6], ybuf[..., :6])
    out, v = R.conv_op(xbuf, ybuf, w=w, scale=sc, shift=sh, xcoff=2, ycoff=6, act=1, x2=x2, w2=w2, scale2=sc2,
                       shift2=sh2, stride2=2)
    assert np.array_equal(v, base2) and np.array_equal(out[..., 6:], np.maximum(base2, 0))


@pytest.mark.parametrize("k,s,p", [(5, 1, 2), (3, 2, 1), (2, 2, 0)])
def test_maxpool_op_equals_torch(k, s, p):
    rng = np.random.default_rng(k)
    xbuf = -np.abs(rng.standard_normal((2, 7, 9, 10))) - 0.5          # all negative: padded taps must be ignored
    oh, ow = (7 + 2 * p - k) // s + 1, (9 + 2 * p - k) // s + 1
    ybuf = rng.standard_normal((2, oh, ow, 12))
    out = R.maxpool_op(xbuf, ybuf, ch=6, k=k, s=s, p=p, xcoff=2, ycoff=4)
    assert np.array_equal(out[..., 4:10], _nhwc(F.max_pool2d(_nchw(xbuf[..., 2:8]), k, s, p)))
    assert np.array_equal(out[..., :4], ybuf[..., :4]) and np.array_equal(out[..., 10:], ybuf[..., 10:])


def test_upsample_op_equals_torch():
    rng = np.random.default_rng(5)
    xbuf, ybuf = rng.standard_normal((2, 5, 7, 9)), rng.standard_normal((2, 10, 14, 8))
    out = R.upsample_op(xbuf, ybuf, ch=4, xcoff=3, ycoff=2)
    assert np.array_equal(out[..., 2:6], _nhwc(F.interpolate(_nchw(xbuf[..., 3:7]), scale_factor=2, mode="nearest")))
    assert np.array_equal(out[..., :2], ybuf[..., :2]) and np.array_equal(out[..., 6:], ybuf[..., 6:])


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_op_equals_torch(stride):
    rng = np.random.default_rng(stride)
    xbuf, w = _dyadic(rng, (2, 10, 13, 8)), _dyadic(rng, (6, 3, 3))
    oh, ow = (10 - 1) // stride + 1, (13 - 1) // stride + 1
    ybuf = _dyadic(rng, (2, oh, ow, 8))
    out, v = R.dwconv_op(xbuf, ybuf, w=w, scale=np.ones(6), shift=np.zeros(6), stride=stride)
    ref = _nhwc(F.conv2d(_nchw(xbuf[..., :6]), torch.from_numpy(w[:, None]), stride=stride, padding=1, groups=6))
    assert np.array_equal(v, ref) and np.array_equal(out[..., :6], ref) and np.array_equal(out[..., 6:], ybuf[..., 6:])


def _exact16(a):
    return np.array_equal(R.round16(a, "bf16"), a) and np.array_equal(R.round16(a, "fp16"), a)


def test_case_names_are_unique():
    names = [c.name for c in R.CONV_CASES + R.POOL_CASES + R.DW_CASES]
    assert len(names) == len(set(names))


def test_l1_shapes_are_the_big_cases():
    from test_gpu_kernels import BIG_CASES
    assert R.BIG_CASES == BIG_CASES and [c.shape for c in R.L1] == BIG_CASES


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_conv_case_input_conditions(case):
    """Conditions on the inputs, not tolerances: every pre-activation value is a multiple of 1/4
    below 2^22 (so every partial sum is exact in f32 in any order, and the leaky slope 1/2 keeps it
    exact), every stored value is below the fp16 maximum, every buffer value is exact in bf16 and
    fp16, and the SiLU legs keep |v| <= 16 with a non-negative residual."""
    d = case.dims
    act = d["act"]
    for mode in ("int", "silu") if act == 3 else ("int",):
        pr = R.conv_problem(case, mode)
        for name, a in pr.items():
            if name not in ("scale", "shift", "scale2", "shift2"):
                assert _exact16(a), name
        out, v = R.conv_reference(case, mode, 1 if (act == 3 and mode == "int") else act, R.SLOPE)
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() < 2 ** 22
        assert np.abs(out).max() < 65504 and np.abs(v).max() > 0
        assert np.array_equal(out.astype(np.float32), out) or act == 3 and mode == "silu"
        if mode == "silu":
            assert np.abs(v).max() <= 16
            if d["rm"]:
                res = pr["y0"] if case.r_is_y else pr["res"]
                assert res[..., case.res_coff:case.res_coff + d["cout"]].min() >= 0
        # the x buffer's channels outside the slice are nonzero; the y guard is within +-64
        outside = np.ones(d["ldx"], bool)
        outside[case.xcoff:case.xcoff + d["span"]] = False
        assert np.all(pr["x"][..., outside] != 0)
        if not case.y_is_x:
            assert np.abs(pr["y0"]).max() <= 64
        # the slices lie inside their buffers
        assert case.xcoff + d["span"] <= d["ldx"] and case.ycoff + d["cout"] <= d["ldy"]
        assert not d["rm"] or case.res_coff + d["cout"] <= (d["ldy"] if case.r_is_y else d["res_ld"])


@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: c.name)
def test_dw_case_input_conditions(case):
    pr = R.dw_problem(case, "int")
    out, v = R.dw_reference(case, pr, R.SLOPE)
    assert _exact16(pr["x"]) and _exact16(pr["y0"]) and _exact16(pr["w"])
    assert np.array_equal(v * 4, np.round(v * 4)) and 0 < np.abs(v).max() < 2 ** 22
    assert np.array_equal(out.astype(np.float32), out) and np.abs(out).max() < 65504


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: c.name)
def test_pool_case_input_conditions(case):
    for prec in ("bf16", "fp16", "fp32"):
        pr = R.pool_problem(case, prec)
        assert np.array_equal(R.round16(pr["x"], prec), pr["x"])
        assert not case.k or pr["x"][0].max() < 0
        out = R.pool_reference(case, pr)
        assert np.array_equal(out.astype(np.float32), out)
        assert case.xcoff + case.ch <= case.ldx and case.ycoff + case.ch <= case.ldy
