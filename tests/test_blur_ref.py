"""CPU checks of the Gaussian-blur mode: the library's host weight routine against the
numpy formula, the integer definition against the real-valued Gaussian (the bound
include/vdmi.h states), the sequential-overlap rule of the reference the GPU tests compare
with, and the argument validation that needs no device."""
import ctypes

import numpy as np
import pytest

import gaussian_ref as gr

PAIRS = [(3, 0.0), (5, 0.0), (9, 2.0), (31, 0.0), (63, 0.0), (99, 30.0), (127, 0.0), (127, 40.0), (127, 0.5)]
SHAPES = [(1, 1), (1, 7), (2, 5), (5, 3), (17, 40), (64, 64), (100, 37)]     # (bh, bw)


@pytest.mark.parametrize("k,sigma", [(3, 0.0), (5, 0.0), (9, 2.0), (31, 0.0), (99, 30.0), (127, 0.0), (127, 0.5)])
def test_library_weights_match_the_formula(k, sigma):
    from vdmi import _lib
    q = _lib.blur_weights(k, sigma)
    assert q.dtype == np.uint32 and q.shape == (k,)
    np.testing.assert_array_equal(q, gr.weights_q20(k, sigma))
    assert int(q.astype(np.int64).sum()) == 1 << 20
    np.testing.assert_array_equal(q, q[::-1])
    assert (q.astype(np.int64) >= 0).all() and int(q.max()) <= 1 << 20      # no wrapped centre tap
    assert int(q[k // 2]) == int(q.max())


@pytest.mark.parametrize("k,sigma", [(4, 0.0), (30, 1.0), (1, 0.0), (2, 0.0), (-3, 0.0), (129, 0.0), (255, 0.0),
                                     (31, float("nan")), (31, float("inf")), (31, float("-inf"))])
def test_library_weights_refusals(k, sigma):
    from vdmi import _lib
    lib = _lib.load()
    q = np.zeros(256, np.uint32)
    assert lib.vdt_blur_weights(k, ctypes.c_float(sigma), _lib.ptr(q)) == _lib.VD_ERR_ARG
    assert not q.any()
    with pytest.raises(_lib.VdError):
        _lib.blur_weights(k, sigma)


def test_library_weights_null_pointer():
    from vdmi import _lib
    assert _lib.load().vdt_blur_weights(5, ctypes.c_float(0.0), None) == _lib.VD_ERR_ARG


def _inputs(bh, bw, rng):
    yy, xx = np.mgrid[0:bh, 0:bw]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    return {"random": rng.integers(0, 256, (bh, bw, 3), dtype=np.uint8),
            "const255": np.full((bh, bw, 3), 255, np.uint8),
            "checker": np.repeat(checker[:, :, None], 3, 2)}


@pytest.mark.parametrize("k,sigma", PAIRS)
def test_integer_definition_within_bound_of_float64(k, sigma):
    """|fixed - exact| <= 0.5925 (weight quantisation 0.031 per pass + Q8.4 rounding 0.031
    before the final rounding's 0.5), constants and 1x1 boxes unchanged, every sum in uint32."""
    rng = np.random.default_rng(1000 * k + int(sigma * 10))
    q = gr.weights_q20(k, sigma)
    worst, stats = 0.0, {}
    for bh, bw in SHAPES:
        for name, reg in _inputs(bh, bw, rng).items():
            got = gr.blur_region_int(reg, q, stats)
            exact = gr.blur_region_f64(reg, k, sigma)
            worst = max(worst, float(np.abs(got.astype(np.float64) - exact).max()))
            if name == "const255" or (bh, bw) == (1, 1):
                np.testing.assert_array_equal(got, reg)
    print(f"k={k} sigma={sigma}: worst |fixed - float64| = {worst:.4f}, max t = {stats['t']}, max s = {stats['s']}")
    assert worst <= 0.5925
    assert stats["t"] < 1 << 28 and stats["s"] < 1 << 32 and stats["out"] <= 255


def test_sequential_rule_order_matters():
    """Three chained overlapping boxes: the reversed list gives a different image, so a GPU
    test against blur_frame sees a path that applies overlapping boxes in the wrong order."""
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    keep = img.copy()
    boxes = [(4, 4, 30, 28), (20, 12, 46, 36), (36, 20, 60, 44)]
    a = gr.blur_frame(img, boxes, 9, 0.0)
    b = gr.blur_frame(img, boxes[::-1], 9, 0.0)
    assert not np.array_equal(a, b)
    # outside the union nothing changes; a box applied alone differs from its chained result
    mask = np.zeros(img.shape[:2], bool)
    for x1, y1, x2, y2 in boxes:
        mask[y1:y2, x1:x2] = True
    np.testing.assert_array_equal(a[~mask], img[~mask])
    alone = gr.blur_frame(img, boxes[1:2], 9, 0.0)
    x1, y1, x2, y2 = boxes[1]
    assert not np.array_equal(alone[y1:y2, x1:x2], a[y1:y2, x1:x2])
    np.testing.assert_array_equal(img, keep)             # the input is untouched


def test_reflection_narrower_than_radius():
    """Boxes narrower than r reflect more than once (borderInterpolate's loop)."""
    assert [gr.refl(p, 3) for p in range(-6, 9)] == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert [gr.refl(p, 1) for p in (-5, 0, 9)] == [0, 0, 0]
    assert [gr.refl(p, 2) for p in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]


def test_context_argument_validation_needs_no_device():
    import vdmi
    from vdmi import _lib
    with pytest.raises(ValueError, match="blur"):
        vdmi.Context(blur="median")
    for bad in (4, 1, 129, -5):
        with pytest.raises(_lib.VdError) as e:
            vdmi.Context(blur="gaussian", blur_ksize=bad)
        assert e.value.code == _lib.VD_ERR_ARG and "blur_ksize" in str(e.value)
    with pytest.raises(_lib.VdError) as e:
        vdmi.Context(blur="gaussian", blur_sigma=float("nan"))
    assert e.value.code == _lib.VD_ERR_ARG
    cfg = _lib.default_cfg()
    assert (cfg.blur_mode, cfg.blur_ksize, cfg.blur_sigma) == (_lib.VD_BLUR_PIXELATE, 0, 0.0)
    assert (cfg.microbatch, cfg.microbatch_stage) == (0, 0)
    cfg.blur_mode = 2
    h = ctypes.c_void_p()
    assert _lib.load().vd_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.VD_ERR_ARG
    assert "blur_mode" in _lib.last_error()


def test_cfg_keeps_the_microbatch_slots_in_place():
    """The named fields are the former reserved[8]: same struct size, micro-batch slots first."""
    from vdmi import _lib
    c = _lib.vd_cfg
    assert c.microbatch.offset == c.plate_max_det.offset + 4
    assert c.microbatch_stage.offset == c.microbatch.offset + 4
    assert c.reserved.offset + c.reserved.size == c.microbatch.offset + 8 * 4
    assert ctypes.sizeof(c) == 104                       # 100 bytes of fields, aligned for the doubles
