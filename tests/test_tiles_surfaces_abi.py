"""Tiled detection on 4:2:0 surfaces through the layers, without a GPU: include/vdmi.h declares
vd_tiles_surfaces and the surface tile hooks, libvdmi.so exports them, vdmi._lib binds them, Context
carries the argument and the methods; and the definition the kernel has to meet, in numpy: cropping the
converted frame equals converting the rectangle through the rectangle form with the origin's parities
(tests/tiles_yuv_ref.py), for the shapes tests/test_gpu_tiles_yuv420.py runs on the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import nv12_ref as nr
import tiles_ref as tr
import tiles_yuv_ref as tyr
import yuv420_16_ref as y16
import yuv420_ref as yr
from conftest import ROOT

HOOKS = {"vdt_letterbox_tiles_nv12": "vd_nv12", "vdt_letterbox_tiles_yuv420": "vd_yuv420",
         "vdt_letterbox_tiles_yuv420_16": "vd_yuv420_16"}
# (h, w, tiles, overlap) of the device tests: every parity of a tile origin occurs
SHAPES = [(174, 212, (2, 2), 20), (174, 212, (1, 3), 0), (174, 212, (3, 1), 50), (38, 54, (4, 4), 50)]


def test_header_declares_the_switch_and_the_hooks():
    text = " ".join(open(os.path.join(ROOT, "include", "vdmi.h")).read().split()).replace(" * ", " ")   # comments as prose
    for needle in ("int vd_tiles_surfaces(vd_ctx* ctx, int on);",
                   "int vdt_letterbox_tiles_nv12(vd_ctx* ctx, const vd_nv12* frames, int n, int h, int w, int where, "
                   "float* out_nhwc, int cpad);",
                   "int vdt_letterbox_tiles_yuv420(vd_ctx* ctx, const vd_yuv420* frames, int n, int h, int w, int where, "
                   "float* out_nhwc, int cpad);",
                   "int vdt_letterbox_tiles_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* frames, int n, int h, int w, int where, "
                   "float* out_nhwc, int cpad);",
                   "int vdt_plate_raw_tiles_yuv420(vd_ctx* ctx, const vd_yuv420* frames, int n, int h, int w, int where, "
                   "float* out, int* anchors);",
                   "(y0 & 1, x0 & 1)"):
        assert needle in text, needle
    assert "an NV12 call that would run a tiled net is VD_ERR_STATE" not in text
    # what is still not offered stays named
    for still in ("Rescue with tiling", "the fixed 31-tap Gaussian on surfaces", "4:2:2 / 4:4:4", "depth conversion"):
        assert still in text, still


def test_library_exports_the_switch():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    assert lib.vd_tiles_surfaces(None, 1) == _lib.VD_ERR_ARG and "null context" in _lib.last_error()
    sig = {s[0]: s for s in _lib.SIGNATURES}["vd_tiles_surfaces"]
    assert sig[1] is ctypes.c_int and sig[2] == [ctypes.c_void_p, ctypes.c_int]


@pytest.mark.parametrize("name", sorted(HOOKS))
def test_library_exports_the_face_hooks(name):
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    assert getattr(lib, name)(None, None, 1, 2, 2, 0, None, 4) == _lib.VD_ERR_ARG and "null context" in _lib.last_error()
    sig = {s[0]: s for s in _lib.SIGNATURES}[name]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 8 and sig[2][1] == ctypes.POINTER(getattr(_lib, HOOKS[name]))


def test_library_exports_the_plate_hook():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    a = ctypes.c_int(-1)
    assert lib.vdt_plate_raw_tiles_yuv420(None, None, 1, 2, 2, 0, None, ctypes.byref(a)) == _lib.VD_ERR_ARG
    assert "null context" in _lib.last_error() and a.value == -1
    sig = {s[0]: s for s in _lib.SIGNATURES}["vdt_plate_raw_tiles_yuv420"]
    assert len(sig[2]) == 8 and sig[2][1] == ctypes.POINTER(_lib.vd_yuv420) and sig[2][7] == ctypes.POINTER(ctypes.c_int)


def test_context_has_the_argument_and_the_methods():
    import vdmi
    from vdmi import _lib
    p = inspect.signature(vdmi.Context.__init__).parameters
    assert p["tile_surfaces"].default is False
    assert list(inspect.signature(vdmi.Context.set_tile_surfaces).parameters) == ["self", "on"]
    assert list(inspect.signature(vdmi.Context.letterbox_tiles_nv12).parameters) == \
        ["self", "frames", "cpad", "matrix", "range", "height"]
    assert list(inspect.signature(vdmi.Context.letterbox_tiles_yuv420).parameters) == \
        ["self", "frames", "cpad", "layout", "matrix", "range", "height"]
    assert list(inspect.signature(vdmi.Context.letterbox_tiles_yuv420_16).parameters) == \
        ["self", "frames", "cpad", "layout", "depth", "shift", "matrix", "range", "height"]
    assert list(inspect.signature(vdmi.Context.plate_raw_tiles_yuv420).parameters) == \
        ["self", "frames", "layout", "matrix", "range", "height"]
    # the argument is checked before the library is touched: no device is needed to be told
    assert _lib.check_tile_surfaces(True) is True and _lib.check_tile_surfaces(0) is False
    for bad in (2, -1, "on", None, 1.0):
        with pytest.raises(ValueError, match="tile_surfaces"):
            _lib.check_tile_surfaces(bad)
        with pytest.raises(ValueError, match="tile_surfaces"):
            vdmi.Context(precision="fp32", max_batch=1, tile_surfaces=bad)


def _rects(h, w, tiles, ov):
    from vdmi import _lib
    rects = tr.tile_rects(h, w, tiles[0], tiles[1], ov)
    assert np.array_equal(rects, _lib.tile_rects(h, w, tiles, ov))   # the library's host routine agrees
    return rects.tolist()


def test_the_shapes_cover_every_parity():
    seen = set()
    for h, w, tiles, ov in SHAPES:
        for x0, y0, tw, th in _rects(h, w, tiles, ov)[1:]:
            seen.add((y0 & 1, x0 & 1, tw & 1, th & 1))
    assert {(s[0], s[1]) for s in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {s[2] for s in seen} == {0, 1} and {s[3] for s in seen} == {0, 1}     # odd and even extents
    assert _rects(174, 212, (2, 2), 20)[4] == [84, 69, 128, 105]
    assert [r[0] for r in _rects(174, 212, (1, 3), 0)[1:]] == [0, 70, 141] and _rects(174, 212, (1, 3), 0)[1][2] == 71
    assert [r[1] for r in _rects(174, 212, (3, 1), 50)[1:]] == [0, 43, 87] and _rects(174, 212, (3, 1), 50)[1][3] == 87
    r44 = _rects(38, 54, (4, 4), 50)
    assert sorted({r[0] for r in r44[1:]}) == [0, 11, 22, 33] and sorted({r[1] for r in r44[1:]}) == [0, 7, 15, 23]
    assert r44[1][2:] == [21, 15]


@pytest.mark.parametrize("h,w,tiles,ov", SHAPES)
@pytest.mark.parametrize("matrix,rng", [("bt709", "limited"), ("bt601", "full")])
def test_cropping_the_converted_frame_is_converting_the_rectangle(h, w, tiles, ov, matrix, rng):
    """The definition, without the library's kernel: crop(to_rgb(frame)) == rect_to_rgb(frame, rectangle),
    against the numpy conversion and against the library's host conversions of two layouts and of 10-bit
    words with random unused bits."""
    import vdmi
    nv = np.random.default_rng(h * w + ov).integers(0, 256, (1, h * 3 // 2, w), dtype=np.uint8)
    Y, U, V = (p[0] for p in yr.planes_of(nv, "nv12"))
    rgb = nr.to_rgb(nv, matrix, rng)[0]
    assert np.array_equal(rgb, vdmi.nv12_to_rgb(nv, matrix, rng)[0])
    assert np.array_equal(rgb, vdmi.yuv420_to_rgb(yr.from_nv12(nv, "yv12"), "yv12", matrix, rng)[0])
    wide = y16.widen(yr.from_nv12(nv, "i420"), 10, 0, seed=h)
    assert np.array_equal(rgb, vdmi.yuv420_16_to_rgb(wide, "i420", 10, 0, matrix, rng)[0])
    for x0, y0, tw, th in _rects(h, w, tiles, ov):
        got = tyr.rect_to_rgb(Y, U, V, x0, y0, tw, th, matrix, rng)
        assert np.array_equal(got, rgb[y0:y0 + th, x0:x0 + tw]), (x0, y0, tw, th)
    # the parity matters: the same rectangle read as a frame of its own differs where an origin is odd
    x0, y0, tw, th = next(r for r in _rects(h, w, tiles, ov)[1:] if (r[0] | r[1]) & 1)
    Yr, Ur, Vr, _, _ = tyr.rect_source(Y, U, V, x0, y0)
    yy, xx = np.arange(th)[:, None], np.arange(tw)[None, :]
    naive = nr.convert(Yr[yy, xx], Ur[yy >> 1, xx >> 1], Vr[yy >> 1, xx >> 1], matrix, rng)
    assert not np.array_equal(naive, rgb[y0:y0 + th, x0:x0 + tw])
