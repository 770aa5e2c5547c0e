"""CPU checks of the 8-bit 4:2:0 layouts (include/vdmi.h at vd_yuv420): the ctypes mirror of the
descriptor against the header, the exported entries, the host conversion vd_yuv420_to_rgb in every
layout against tests/nv12_ref.py on the re-laid-out frames (tests/yuv420_ref.py), and the
descriptor's VD_ERR_ARG rules. No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import nv12_ref as nr
import yuv420_ref as yr
from conftest import ROOT

TABLES = sorted(nr.COEF)
MATRIX = {"bt601": 0, "bt709": 1}
RANGE = {"limited": 0, "full": 1}


def test_yuv420_struct_layout_matches_header(tmp_path):
    """The ctypes mirror of vd_yuv420 has the C compiler's size and field offsets."""
    import shutil
    import subprocess
    from vdmi import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fl = [f[0] for f in _lib.vd_yuv420._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdmi.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(vd_yuv420));']
    lines += [f'printf("{f} %zu\\n", offsetof(vd_yuv420, {f}));' for f in fl]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.vd_yuv420)
    for f in fl:
        assert int(out[f]) == getattr(_lib.vd_yuv420, f).offset, f


def test_entries_are_exported():
    import vdmi
    lib = vdmi.load()
    for name in ("vd_process_yuv420", "vd_mosaic_yuv420", "vd_smooth_yuv420", "vd_yuv420_to_rgb", "vdt_letterbox_yuv420"):
        assert hasattr(lib, name), name
    for name in ("process_yuv420", "mosaic_yuv420", "smooth_yuv420", "letterbox_yuv420"):
        assert callable(getattr(vdmi.Context, name)), name
    assert callable(vdmi.yuv420_to_rgb) and vdmi.Yuv420 is not None


def test_relayout_helper_round_trips():
    rng = np.random.default_rng(0)
    nv = rng.integers(0, 256, (2, 9, 10), dtype=np.uint8)
    for lay in yr.LAYOUTS:
        s = yr.from_nv12(nv, lay)
        assert np.array_equal(yr.to_nv12(s, lay), nv), lay
        assert np.array_equal(s[:, :6], nv[:, :6])
    assert np.array_equal(yr.from_nv12(nv, "nv12"), nv)
    i420 = yr.from_nv12(nv, "i420")
    assert np.array_equal(i420[:, 6:].reshape(2, -1)[:, :15].reshape(2, 3, 5), nv[:, 6:].reshape(2, 3, 5, 2)[..., 0])
    assert np.array_equal(yr.from_nv12(nv, "nv21")[:, 6:, 0::2], nv[:, 6:, 1::2])


@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (48, 64)])
@pytest.mark.parametrize("layout", yr.LAYOUTS)
def test_host_conversion_equals_the_definition(layout, hw):
    import vdmi
    h, w = hw
    rng = np.random.default_rng(h * 131 + w)
    nv = rng.integers(0, 256, (2, h * 3 // 2, w), dtype=np.uint8)
    s = yr.from_nv12(nv, layout)
    for matrix, r in TABLES:
        got = vdmi.yuv420_to_rgb(s, layout=layout, matrix=matrix, range=r)
        assert np.array_equal(got, nr.to_rgb(nv, matrix, r)), (matrix, r)


def _padded_cases(h, w):
    """(layout, pitch, cpitch, hpad, v_first, extra): odd chroma pitches, swapped planes, padded strides."""
    return [("i420", w + 6, w // 2 + 3, h + 2, True, 37), ("yv12", w, w // 2 + 1, h, False, 0),
            ("nv12", w + 2, w + 5, h + 4, True, 11), ("nv21", w + 16, w + 16, h, False, 16)]


@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (48, 64)])
def test_padded_layouts_read_the_described_bytes(hw):
    """Odd chroma pitch, U and V in swapped order, padded height and stride: the pad bytes (0xA5, then
    0x00) never matter, through the C entry and through vdmi.Yuv420."""
    import vdmi
    from vdmi import _lib
    h, w = hw
    n = 2
    rng = np.random.default_rng(7)
    nv = rng.integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    for matrix, r in TABLES:
        want = nr.to_rgb(nv, matrix, r)
        for lay, pitch, cpitch, hpad, v_first, extra in _padded_cases(h, w):
            for fill in (0xA5, 0x00):
                buf, fd = yr.padded(yr.from_nv12(nv, lay), lay, pitch, cpitch, hpad, v_first, extra, fill)
                d = _lib.vd_yuv420(buf.ctypes.data, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                                   fd["frame_stride"], fd["chroma_step"], MATRIX[matrix], RANGE[r])
                got = np.zeros((n, h, w, 3), np.uint8)
                assert _lib.load().vd_yuv420_to_rgb(ctypes.byref(d), n, h, w, got.ctypes.data, w * 3) == _lib.VD_OK, lay
                assert np.array_equal(got, want), (lay, matrix, r, fill)
            y = vdmi.Yuv420(buf, h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"], fd["chroma_step"],
                            fd["frame_stride"])
            assert y.n == n
            assert np.array_equal(vdmi.yuv420_to_rgb(y, matrix=matrix, range=r), want), lay


def test_python_padded_height():
    import vdmi
    rng = np.random.default_rng(9)
    n, h, w, H = 2, 6, 10, 8
    nv = rng.integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    Y, U, V = yr.planes_of(nv, "nv12")
    tall = np.full((n, H * 3 // 2, w), 0xA5, np.uint8)
    tall[:, :h] = Y
    c = tall[:, H:].reshape(n, 2, H // 2, w // 2)
    c[:, 0, :h // 2], c[:, 1, :h // 2] = U, V
    assert np.array_equal(vdmi.yuv420_to_rgb(tall, layout="i420", height=h), nr.to_rgb(nv))
    c[:, 0, :h // 2], c[:, 1, :h // 2] = V, U
    assert np.array_equal(vdmi.yuv420_to_rgb(tall, layout="yv12", height=h), nr.to_rgb(nv))


def test_host_err_arg_cases():
    """Every descriptor rule of the header, each with a message naming the field; nothing is written."""
    import vdmi
    from vdmi import _lib
    lib = _lib.load()
    h, w, n = 4, 6, 2
    buf = np.zeros(4096, np.uint8)
    rgb = np.zeros((n, h, w, 3), np.uint8)

    def desc(pitch=8, u=32, v=40, cp=4, st=48, step=1, matrix=1, rng=0, base=buf.ctypes.data):
        return _lib.vd_yuv420(base, pitch, u, v, cp, st, step, matrix, rng)

    def call(d, n=n, h=h, w=w, out=rgb, rgb_pitch=w * 3):
        return lib.vd_yuv420_to_rgb(ctypes.byref(d) if d is not None else None, n, h, w,
                                    out.ctypes.data if out is not None else None, rgb_pitch)

    assert call(desc()) == _lib.VD_OK                                         # I420: planes of 2 rows x 4 bytes
    assert call(desc(u=40, v=32)) == _lib.VD_OK                               # YV12
    assert call(desc(u=32, v=33, cp=8, step=2)) == _lib.VD_OK                 # NV12
    assert call(desc(u=33, v=32, cp=8, step=2)) == _lib.VD_OK                 # NV21
    assert call(desc(u=30, v=37, cp=4, st=44)) == _lib.VD_OK                  # tight: luma ends at 3 * 8 + 6 = 30
    assert call(desc(st=46), n=1) == _lib.VD_OK                               # one frame: frame_stride is not read
    bad = [
        (dict(h=3), desc(), "h"), (dict(w=5), desc(), "w"), (dict(h=0), desc(), "h"), (dict(w=-2), desc(), "w"),
        (dict(n=0), desc(), "n"),
        ({}, desc(pitch=5), "pitch"),
        ({}, desc(cp=2), "chroma_pitch"), ({}, desc(u=32, v=33, cp=5, step=2), "chroma_pitch"),
        ({}, desc(step=0), "chroma_step"), ({}, desc(step=3), "chroma_step"),
        ({}, desc(u=32, v=34, cp=8, step=2), "u_offset - v_offset"), ({}, desc(u=32, v=32, cp=8, step=2), "u_offset - v_offset"),
        ({}, desc(u=29, v=40), "u_offset"),                                   # U starts inside the luma plane
        ({}, desc(u=40, v=29, st=60), "v_offset"),                            # V inside the luma plane
        ({}, desc(u=32, v=38), "v_offset"),                                   # U [32, 40) and V [38, 46) overlap
        ({}, desc(u=32, v=32), "v_offset"),
        ({}, desc(u=29, v=30, cp=8, step=2), "u_offset"),                     # the pair plane inside the luma plane
        ({}, desc(st=46), "frame_stride"),                                    # V ends at 47
        ({}, desc(u=32, v=33, cp=8, step=2, st=45), "frame_stride"),          # the pairs end at 46
        ({}, desc(matrix=2), "matrix"), ({}, desc(rng=-1), "range"),
    ]
    for kw, d, field in bad:
        rgb[:] = 7
        assert call(d, **kw) == _lib.VD_ERR_ARG, (kw, field)
        msg = lib.vd_last_error().decode()
        assert field in msg.split(" (n=")[0] and "vd_yuv420_to_rgb" in msg, (field, msg)
        assert (rgb == 7).all(), field
    assert call(None) == _lib.VD_ERR_ARG and "null" in lib.vd_last_error().decode()
    assert call(desc(base=None)) == _lib.VD_ERR_ARG and "base" in lib.vd_last_error().decode()
    assert call(desc(), rgb_pitch=w * 3 - 1) == _lib.VD_ERR_ARG
    assert call(desc(), out=None) == _lib.VD_ERR_ARG
    # the Python forms refuse what they cannot describe
    with pytest.raises(ValueError):
        vdmi.yuv420_to_rgb(np.zeros((1, 6, 4), np.uint8), layout="p010")
    with pytest.raises(ValueError):
        vdmi.Yuv420(np.zeros(40, np.uint8), 4, 6, 8, 32, 40, 4, 1, 48)       # the buffer ends before V does
