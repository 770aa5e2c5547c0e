"""layer1.0 (cin 64 + downsample) on the pipelined fp32 bottleneck kernel (block32.hip,
option block32_pipe_ds): against a float64 bottleneck, against the one-group kernel it
replaces (bit for bit), and through the whole face net."""
import numpy as np
import pytest
import torch

from conftest import face_weights

pytestmark = pytest.mark.gpu
F32 = np.float32

CASES = [
    # (n, h, w), cin 64 + downsample
    (1, 8, 5),         # narrower than one tile
    (2, 13, 18),       # ragged tiles
    (1, 21, 37),       # ragged on both axes
    (1, 40, 40),       # interior tile seams
    (3, 24, 48),       # frames scaled by 1, 2^10, 2^-10: a tile that took another frame's x scale would show
    (8, 96, 160),      # 960 tiles, several per persistent workgroup: the t1 / t2 / xs buffers and max-slot rings cycle
]

_DATA = {}


def _bn(rng, c):
    return np.concatenate([rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.1]).astype(F32)


def _case(case):
    """Inputs and the float64 reference of a case, made once and shared (read-only)."""
    if case not in _DATA:
        n, h, w = case
        rng = np.random.default_rng(h * 1000 + w * 10 + n)
        he = lambda co, ci, k: (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(F32)
        x = np.maximum(rng.standard_normal((n, h, w, 64)), 0).astype(F32)      # a ReLU output, as in the net
        if case == (3, 24, 48):
            x[1] *= F32(2.0 ** 10)
            x[2] *= F32(2.0 ** -10)
        args = (x, he(64, 64, 1), _bn(rng, 64), he(64, 64, 3), _bn(rng, 64), he(256, 64, 1), _bn(rng, 256),
                he(256, 64, 1), _bn(rng, 256))
        x, w1, b1, w2, b2, w3, b3, wd, bd = args
        T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        conv = lambda v, wt, p: torch.nn.functional.conv2d(v, T(wt), padding=p)
        aff = lambda v, b, c: v * T(b[:c]).view(1, c, 1, 1) + T(b[c:]).view(1, c, 1, 1)
        xt = T(x).permute(0, 3, 1, 2)
        t1 = torch.relu(aff(conv(xt, w1, 0), b1, 64))
        t2 = torch.relu(aff(conv(t1, w2, 1), b2, 64))
        ref = torch.relu(aff(conv(t2, w3, 0), b3, 256) + aff(conv(xt, wd, 0), bd, 256)).permute(0, 2, 3, 1).numpy()
        for a in args:
            a.setflags(write=False)
        ref.setflags(write=False)
        _DATA[case] = (args, ref, {})
    return _DATA[case]


def _run(face_ctx_factory, case, pipe_ds, fused=True):
    """The block's output for a case, computed once per (kernel, path)."""
    args, _, outs = _case(case)
    key = (pipe_ds, fused)
    if key not in outs:
        ctx = face_ctx_factory("fp32", 8, options=(("block32_pipe_ds", pipe_ds),))
        outs[key] = ctx.bottleneck(*args, fused=fused)
    return outs[key]


def _frame_err(got, ref):
    """Per frame: max |got - ref| over that frame's own output range."""
    n = ref.shape[0]
    return np.array([np.abs(got[b] - ref[b]).max() / np.abs(ref[b]).max() for b in range(n)])


@pytest.mark.parametrize("case", CASES)
def test_block32_ds_pipe_matches_float64(gpu, face_ctx_factory, case):
    """The pipelined downsample block against a float64 torch bottleneck on the same f32
    inputs: per frame, against that frame's own output range, below 2e-6 (f32 rounding of
    K = 576 sums), and the worst frame within 2x the conv-by-conv chain's worst + 1e-7."""
    _, ref, _ = _case(case)
    got = _run(face_ctx_factory, case, 1)
    chain = _run(face_ctx_factory, case, 1, fused=False)
    assert got.shape == ref.shape
    e_fused, e_chain = _frame_err(got, ref), _frame_err(chain, ref)
    print(f"block32 ds pipe {case}: fused {e_fused.max():.2e}, chain {e_chain.max():.2e}")
    assert (e_fused < 2e-6).all(), e_fused
    assert e_fused.max() <= 2 * e_chain.max() + 1e-7, (e_fused, e_chain)


@pytest.mark.parametrize("case", CASES)
def test_block32_ds_pipe_equals_one_group(gpu, face_ctx_factory, case):
    """block32_pipe_ds 1 against 0: the same products, K order, operand scales and the
    one-group kernel's two-K-half summation in stage 2 -- every output bit equal."""
    got = _run(face_ctx_factory, case, 1)
    one = _run(face_ctx_factory, case, 0)
    np.testing.assert_array_equal(got, one)


def test_heads_fp32_block32_pipe_ds_bit_identical(gpu):
    """Two 1080p frames through the face net with layer1.0 on the pipelined kernel against
    the one-group kernel: heads bit-identical (so the per-frame max |y| that layer1.1
    scales by is too), identical keep lists and int boxes."""
    import vdmi
    from vdmi import synth
    fr = synth.frames(2, 1080, 1920, seed=43)
    heads, boxes = {}, {}
    for v in (1, 0):
        ctx = vdmi.Context(precision="fp32", max_batch=2, options={"block32_pipe_ds": v})
        try:
            ctx.load_weights(0, face_weights("default"))
            heads[v] = ctx.forward_heads(fr)
            r = ctx.detect(fr)
            boxes[v] = [(r.frame(b)[3].copy(), r.frame(b)[0].copy()) for b in range(2)]
        finally:
            ctx.close()
    for a, b in zip(heads[1], heads[0]):
        np.testing.assert_array_equal(a, b)
    assert sum(len(x[0]) for x in boxes[0]) > 0
    for (ka, xa), (kb, xb) in zip(boxes[1], boxes[0]):
        np.testing.assert_array_equal(ka, kb)
        np.testing.assert_array_equal(xa, xb)
