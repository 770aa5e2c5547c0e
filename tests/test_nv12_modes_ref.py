"""The NV12 smooth blur and the NV12 ellipse on the CPU: properties of the numpy definitions
(nv12_modes_ref.py) and the new C entry point (no GPU)."""
import ctypes
import itertools

import numpy as np
import pytest

import cells_ref as cr
import mask_ref as mr
import nv12_modes_ref as nm
import nv12_ref as nr

H, W = 10, 12                       # the frame of the enumerations
CORNERS = range(-2, 13)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)


def _boxes():
    """Every non-empty box with corners in [-2, 12] (an empty box touches nothing by definition)."""
    spans = [(a, b) for a in CORNERS for b in CORNERS if b > a]
    return [(x1, y1, x2, y2) for (x1, x2), (y1, y2) in itertools.product(spans, spans)]


# ---- the smooth blur --------------------------------------------------------------------------------

@pytest.mark.parametrize("f", [1, 2, 3, 7, 8, 16, 50])
def test_generic_smooth_equals_cells_ref_on_rgb(f):
    img = np.random.default_rng(f).integers(0, 256, (23, 31, 3), dtype=np.uint8)
    np.testing.assert_array_equal(nm.cell_means(img, f), cr.cell_means(img, f))
    np.testing.assert_array_equal(nm.smooth_region(img, f), cr.smooth_region(img, f))
    # a one-channel plane is the RGB result of a grey image, a two-channel plane two of its channels
    grey = np.repeat(img[:, :, :1], 3, axis=2)
    np.testing.assert_array_equal(nm.smooth_region(img[:, :, 0], f), cr.smooth_region(grey, f)[:, :, 0])
    np.testing.assert_array_equal(nm.smooth_region(img[:, :, :2], f), cr.smooth_region(img, f)[:, :, :2])


def test_constant_planes_stay_constant():
    f = np.empty((48 * 3 // 2, 64), np.uint8)
    f[:48] = 201
    f[48:, 0::2] = 17
    f[48:, 1::2] = 255
    boxes = [(3, 5, 41, 37), (-4, 20, 33, 60), (0, 0, 64, 48), (7, 9, 8, 10)]
    for level, cells in [(1, 2), (8, 4), (3, 64)]:
        np.testing.assert_array_equal(nm.smooth(f, boxes, level, cells), f)


def test_level_1_is_the_identity_in_both_planes():
    f = _noise(48, 64, 1)
    boxes = [(2, 3, 30, 20), (0, 0, 64, 48), (11, 7, 12, 40)]          # at most 64 px a side: L = 1, fc = 1
    assert all(cr.box_level(b, 1, 64) == 1 for b in boxes)
    np.testing.assert_array_equal(nm.smooth(f, boxes, 1, 64), f)


def test_smooth_touches_only_the_boxes_rectangles_and_reads_the_input():
    f = _noise(48, 64, 2)
    boxes = [(5, 3, 30, 21), (21, 10, 55, 39), (-3, 25, 12, 60)]
    out = nm.smooth(f, boxes, 2, 4)
    hit = [np.zeros((48, 64), bool), np.zeros((24, 32), bool)]
    for b in boxes:
        c, cc = nm.rects(b, 48, 64)
        hit[0][c[1]:c[3], c[0]:c[2]] = True
        hit[1][cc[1]:cc[3], cc[0]:cc[2]] = True
    (Yi, UVi), (Yo, UVo) = nr.planes(f), nr.planes(out)
    np.testing.assert_array_equal(Yo[~hit[0]], Yi[~hit[0]])
    np.testing.assert_array_equal(UVo[~hit[1]], UVi[~hit[1]])
    assert (Yo[hit[0]] != Yi[hit[0]]).any() and (UVo[hit[1]] != UVi[hit[1]]).any()
    # strongest wins whatever the order; the owner is chosen by the luma level in both planes:
    # L = 7 and L = 8 share fc = 4, and the L = 8 box owns the chroma overlap from either position
    p, q = (4, 4, 32, 30), (18, 10, 50, 42)
    assert (cr.box_level(p, 1, 4), cr.box_level(q, 1, 4)) == (7, 8)
    np.testing.assert_array_equal(nm.smooth(f, [p, q], 1, 4), nm.smooth(f, [q, p], 1, 4))
    only_q = nm.smooth(f, [q], 1, 4)
    np.testing.assert_array_equal(nr.planes(nm.smooth(f, [p, q], 1, 4))[1][5:15, 9:16], nr.planes(only_q)[1][5:15, 9:16])


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("level", [1, 2])
def test_chroma_grid_never_exceeds_cells_plus_one_and_reaches_it(N, level):
    """cw <= bw / 2 + 1 <= N * L / 2 + 1 <= N * fc + 1: at most N + 1 chroma cells a side, N luma."""
    top = 0
    for b in _boxes():
        g = nm.chroma_grid(b, H, W, level, N)
        if g is None:
            continue
        (lw, lh), (cw, ch) = g
        assert 1 <= lw <= N and 1 <= lh <= N, (b, g)
        assert 1 <= cw <= N + 1 and 1 <= ch <= N + 1, (b, g)
        top = max(top, cw, ch)
    assert top == N + 1
    if (N, level) == (2, 1):
        assert nm.chroma_grid((1, 0, 5, 4), H, W, 1, 2) == ((2, 2), (3, 2))


# ---- the ellipse ------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [0, 42])
def test_span_form_of_the_chroma_hidden_set_equals_the_four_pixel_form(g):
    boxes = _boxes()
    for b in boxes:
        gb = mr.grow(b, g)
        hl = nm.ellipse_mask(H, W, gb)
        c = mr.clip(gb, H, W)
        if c is not None:                              # the spans are the predicate's rows
            for y in range(H):
                s = nm.row_span(gb, c, y)
                want = np.flatnonzero(hl[y])
                if s is None or s[0] == s[1]:
                    assert want.size == 0, (gb, y)
                else:
                    assert (want == np.arange(s[0], s[1])).all(), (gb, y, s)
        hc = nm.hidden_chroma(hl) if hl.any() else np.zeros((H // 2, W // 2), bool)
        assert np.array_equal(nm.hidden_chroma_spans(H, W, [gb]), hc), gb
        if g == 42:                                    # coverage: the stored box and its chroma samples are hidden
            sc = mr.clip(b, H, W)
            if sc is not None:
                assert hl[sc[1]:sc[3], sc[0]:sc[2]].all(), b
                cc = nr.chroma_box(sc)
                assert hc[cc[1]:cc[3], cc[0]:cc[2]].all(), b
    # several boxes at once: the union of the spans is the four-pixel rule on the union
    some = [mr.grow(b, g) for b in boxes[::997]]
    assert np.array_equal(nm.hidden_chroma_spans(H, W, some), nm.hidden_chroma(nm.hidden_luma(H, W, some)))


def test_vectorised_ellipse_mask_equals_mask_ref():
    for b in _boxes()[::53] + [(-40000, 2, 40000, 9), (3, -70000, 9, 70000)]:
        for g in (0, 42):
            gb = mr.grow(b, g)
            assert np.array_equal(nm.ellipse_mask(H, W, gb), mr.ellipse_mask(H, W, gb)), gb


@pytest.mark.parametrize("g", [0, 42])
@pytest.mark.parametrize("mode", ["mosaic", "smooth"])
def test_pixels_that_are_not_hidden_keep_their_colour(mode, g):
    h, w = 48, 64
    f = _noise(h, w, 5 + g)
    boxes = [(5, 3, 30, 21), (21, 10, 55, 39), (-3, 25, 12, 60), (40, 30, 44, 34), (50, 2, 53, 5)]
    fn = (lambda fr, bl: nr.mosaic(fr, bl, 4, 4)) if mode == "mosaic" else (lambda fr, bl: nm.smooth(fr, bl, 4, 4))
    out = nm.shaped(f, boxes, "ellipse", g, fn)
    grown = mr.grow_list(boxes, g)
    hl = nm.hidden_luma(h, w, grown)
    hc_px = nm.hidden_chroma(hl).repeat(2, 0).repeat(2, 1)           # per pixel: its chroma sample is hidden
    free = ~hl & ~hc_px
    assert free.any() and hl.any() and (hc_px & ~hl).any()
    np.testing.assert_array_equal(nr.to_rgb(out)[0][free], nr.to_rgb(f)[0][free])
    # a hidden luma pixel has both its Y and its UV from R
    R = fn(f, grown)
    (Yo, UVo), (Yr, UVr) = nr.planes(out), nr.planes(R)
    np.testing.assert_array_equal(Yo[hl], Yr[hl])
    np.testing.assert_array_equal(UVo[nm.hidden_chroma(hl)], UVr[nm.hidden_chroma(hl)])
    assert not np.array_equal(out, f)
    np.testing.assert_array_equal(nm.shaped(f, boxes, "rect", g, fn), R)


# ---- the C entry point ------------------------------------------------------------------------------

def test_vd_smooth_nv12_is_exported_and_bound():
    from vdmi import _lib
    lib = _lib.load()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.vd_nv12)
    assert sig["vd_smooth_nv12"] == (I, [P, D, D, I, I, I, I, ctypes.POINTER(_lib.vd_boxes), I, I])
    hb = _lib.HostBoxes(1, 1)
    s = hb.struct()
    buf = np.zeros((12, 8), np.uint8)
    d = _lib.vd_nv12(buf.ctypes.data, 8, 64, 96, 1, 0)
    assert lib.vd_smooth_nv12(None, ctypes.byref(d), ctypes.byref(d), 1, 8, 8, 0, ctypes.byref(s), 8, 16) == _lib.VD_ERR_ARG
    assert "null context" in _lib.last_error()


def test_header_declares_the_nv12_modes():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    for needle in ("int vd_smooth_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, int where,",
                   "at most N + 1", "(2cy + {0,1}, 2cx + {0,1})", "set cells"):
        assert needle in text, needle
