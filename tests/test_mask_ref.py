"""Mask shaping on the CPU: hand-computed cases and properties of the numpy definition
(mask_ref.py), the coverage guarantee include/vdmi.h states, the two new C entry points and
the argument checks of the Python layers (no GPU)."""
import ctypes

import numpy as np
import pytest

import gaussian_ref as gr
import mask_ref as mr
from oracle import mosaic as omosaic


def _mosaic(img, boxes):
    return omosaic.mosaic_frame(img, boxes, 8)


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_small_squares_by_hand():
    """Sides 1..3 are wholly inside (3x3 corner: 4 + 4 <= 9); 4x4 and 5x5 lose exactly their
    corners (4x4: 9 + 9 > 16 but 9 + 1 <= 16; 5x5: 16 + 16 > 25 but 16 + 4 <= 25)."""
    for s in (1, 2, 3):
        assert mr.ellipse_mask(8, 8, (2, 2, 2 + s, 2 + s))[2:2 + s, 2:2 + s].all()
    for s in (4, 5):
        exp = np.ones((s, s), bool)
        exp[0, 0] = exp[0, -1] = exp[-1, 0] = exp[-1, -1] = False
        m = mr.ellipse_mask(9, 9, (2, 3, 2 + s, 3 + s))
        np.testing.assert_array_equal(m[3:3 + s, 2:2 + s], exp)
        assert m.sum() == s * s - 4                    # nothing outside the box


def test_40x30_box_loses_260_pixels():
    m = mr.ellipse_mask(48, 64, (10, 8, 50, 38))
    assert 40 * 30 - int(m.sum()) == 260
    assert m[23, 30] and not m[8, 10] and not m[37, 49]
    assert not m[:8].any() and not m[38:].any() and not m[:, :10].any() and not m[:, 50:].any()


def test_grow_by_hand():
    assert mr.grow((10, 20, 17, 30), 30) == (8, 18, 19, 32)        # W = 7: 2.05 -> gx = 2 (ceil of 1.05); H = 10: 1.5 -> 2
    assert mr.grow((0, 0, 8, 20), 30) == (-2, -3, 10, 23)          # W = 8: 1.2 -> 2; H = 20: exactly 3
    assert mr.grow((5, 5, 6, 6), 200) == (4, 4, 7, 7)              # 1 px at the largest margin: 3 px
    assert mr.grow((5, 5, 6, 6), 1) == (4, 4, 7, 7)                # any margin > 0 grows by a whole pixel
    assert mr.grow((-7, 3, 4, 9), 0) == (-7, 3, 4, 9)
    for b in [(60, 30, 60, 50), (70, 50, 65, 58), (3, 9, 8, 9), (4, 4, 2, 1)]:
        assert mr.grow(b, 200) == b                                # an empty box stays empty
    big = 1 << 30
    assert mr.grow((big - 10, 0, big - 2, 10), 200) == (big - 18, -10, big, 20)      # clamped
    assert mr.grow((-2**31, -2**31, 2**31 - 1, 2**31 - 1), 200) == (-big, -big, big, big)


def test_default_setting_is_the_identity():
    img = _img(40, 56, 0)
    boxes = [(5, 4, 30, 20), (20, 10, 55, 39), (-3, 25, 12, 60), (9, 9, 9, 12)]
    np.testing.assert_array_equal(mr.shaped_frame(img, boxes, "rect", 0, _mosaic), _mosaic(img, boxes))
    assert mr.grow_list(boxes, 0) == boxes


@pytest.mark.parametrize("box", [(3, 2, 24, 13), (-6, 5, 17, 40), (10, -9, 30, 8), (1, 1, 5, 5), (0, 0, 33, 21)])
def test_ellipse_mask_is_symmetric_under_both_flips(box):
    h, w = 24, 36
    x1, y1, x2, y2 = box
    m = mr.ellipse_mask(h, w, box)
    np.testing.assert_array_equal(m[:, ::-1], mr.ellipse_mask(h, w, (w - x2, y1, w - x1, y2)))
    np.testing.assert_array_equal(m[::-1], mr.ellipse_mask(h, w, (x1, h - y2, x2, h - y1)))


def test_grow_42_covers_every_pixel_of_a_clipped_box():
    """What vdmi.h and the README state: with g >= 42 the grown box's ellipse holds every pixel
    of the box as stored, wherever the frame clips it (the centre of the ellipse may lie off
    the frame). At g = 41 a large box's corner pixel is outside."""
    h, w = mr.EDGE_HW
    rng = np.random.default_rng(42)
    boxes = list(mr.EDGE_BOXES)
    for _ in range(120):
        bw, bh = int(rng.integers(1, 150)), int(rng.integers(1, 120))
        # starts at a negative coordinate, or runs past the far edge
        x1 = int(rng.integers(-bw, 0)) if rng.random() < 0.5 else int(rng.integers(w - bw + 1, w + 1))
        y1 = int(rng.integers(-bh, 0)) if rng.random() < 0.5 else int(rng.integers(h - bh + 1, h + 1))
        if rng.random() < 0.3:
            x1 = int(rng.integers(-bw, w))             # clipped by a horizontal edge alone
        boxes.append((x1, y1, x1 + bw, y1 + bh))
    checked = 0
    for b in boxes:
        c = mr.clip(b, h, w)
        if c is None:
            continue
        m = mr.ellipse_mask(h, w, mr.grow(b, 42))
        assert m[c[1]:c[3], c[0]:c[2]].all(), b
        checked += 1
    assert checked >= 100
    assert not mr.inside(mr.grow((0, 0, 400, 400), 41), 0, 0)
    assert mr.inside(mr.grow((0, 0, 400, 400), 42), 0, 0)


def test_a_corner_inside_another_ellipse_stays_hidden():
    """(2, 2) is a corner pixel of the large box (outside its ellipse) and inside the small
    box's ellipse: it keeps R. (3, 37) is in no ellipse: the input shows."""
    img = _img(40, 48, 1)
    large, small = (2, 2, 42, 38), (1, 1, 4, 4)
    assert not mr.inside(large, 2, 2) and mr.inside(small, 2, 2)
    for boxes in ([large, small], [small, large]):
        R = _mosaic(img, boxes)
        out = mr.shaped_frame(img, boxes, "ellipse", 0, _mosaic)
        np.testing.assert_array_equal(out[2, 2], R[2, 2])
        np.testing.assert_array_equal(out[37, 3], img[37, 3])
        np.testing.assert_array_equal(out[20, 22], R[20, 22])
        np.testing.assert_array_equal(out[0], img[0])


def test_a_side_over_32768_hides_its_whole_clipped_rectangle():
    box = (-20000, 5, 20000, 40)
    m = mr.ellipse_mask(48, 64, box)
    assert m[5:40].all() and m.sum() == 35 * 64
    assert not mr.ellipse_mask(48, 70, (-32700, 5, 68, 40))[5, 66]         # W = 32768: still an ellipse
    assert mr.ellipse_mask(48, 70, (-32701, 5, 68, 40))[5, 66]             # W = 32769
    img = _img(48, 64, 2)
    q = gr.weights_q20(9, 0.0)
    blur = lambda im, bl: gr.blur_frame(im, bl, 9, 0.0, q=q)
    np.testing.assert_array_equal(mr.shaped_frame(img, [box], "ellipse", 0, blur), blur(img, [box]))


def test_symbols_are_exported_and_bound():
    from vdmi import _lib
    lib = _lib.load()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    P, I = ctypes.c_void_p, ctypes.c_int
    assert sig["vd_mask"] == (I, [P, I, I])
    assert sig["vd_mask_boxes"] == (I, [P, ctypes.POINTER(_lib.vd_boxes), I, ctypes.POINTER(_lib.vd_boxes)])
    assert lib.vd_mask.argtypes == [P, I, I] and lib.vd_mask.restype is I
    assert (_lib.VD_MASK_RECT, _lib.VD_MASK_ELLIPSE, _lib.VD_MASK_GROW_MAX) == (0, 1, 200)
    assert lib.vd_abi_version() == 2
    assert lib.vd_mask(None, _lib.VD_MASK_ELLIPSE, 30) == _lib.VD_ERR_ARG          # null context
    hb = _lib.HostBoxes(1, 1)
    s = hb.struct()
    assert lib.vd_mask_boxes(None, ctypes.byref(s), 1, ctypes.byref(s)) == _lib.VD_ERR_ARG


def test_header_declares_the_contract():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    for needle in ("#define VD_MASK_RECT 0", "#define VD_MASK_ELLIPSE 1", "#define VD_MASK_GROW_MAX 200",
                   "int vd_mask(vd_ctx* ctx, int shape, int grow_pct);",
                   "int vd_mask_boxes(vd_ctx* ctx, const vd_boxes* in, int n, vd_boxes* out);",
                   "#define VDMI_ABI_VERSION 2"):
        assert needle in text, needle


@pytest.mark.parametrize("kw", [dict(mask="oval"), dict(mask_grow=201), dict(mask="ellipse", mask_grow=-1)])
def test_bad_mask_settings_raise_before_the_library_is_touched(kw, tmp_path):
    import vdmi
    from vdmi import _lib
    from vdmi.pipeline import batch_process_images
    with pytest.raises(ValueError, match="mask"):
        _lib.check_mask(kw.get("mask", "rect"), kw.get("mask_grow", 0))
    with pytest.raises(ValueError, match="mask"):
        vdmi.Context(**kw)
    with pytest.raises(ValueError, match="mask"):
        vdmi.Retinaface(weights="random", **kw)
    (tmp_path / "in").mkdir()
    with pytest.raises(ValueError, match="mask"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), **kw)


def test_check_mask_accepts_the_range():
    from vdmi import _lib
    assert _lib.check_mask("rect", 0) == ("rect", 0)
    assert _lib.check_mask("ellipse", 200) == ("ellipse", 200)
    assert _lib.check_mask("ellipse", np.int64(42)) == ("ellipse", 42)
