"""CPU checks of 10- and 12-bit 4:2:0 frames (include/vdmi.h at vd_yuv420_16): the ctypes mirror of the
descriptor against the header, the exported and bound entries, the host conversion vd_yuv420_16_to_rgb
against vd_yuv420_to_rgb on D(S), the descriptor's VD_ERR_ARG rules, and the self-checks of the numpy
reference (tests/yuv420_16_ref.py). No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import nv12_modes_ref as nm
import nv12_ref as nr
import yuv420_16_ref as y16
import yuv420_ref as yr
from conftest import ROOT

FORMATS = [(10, 0), (10, 6), (12, 0), (12, 4), (10, 3)]        # low-, high-aligned, and one in between


def test_struct_layout_matches_header(tmp_path):
    """The ctypes mirror of vd_yuv420_16 has the C compiler's size and field offsets, and starts with
    the fields of vd_yuv420."""
    import shutil
    import subprocess
    from vdmi import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fl = [f[0] for f in _lib.vd_yuv420_16._fields_]
    assert fl == [f[0] for f in _lib.vd_yuv420._fields_] + ["depth", "shift"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdmi.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(vd_yuv420_16));']
    lines += [f'printf("{f} %zu\\n", offsetof(vd_yuv420_16, {f}));' for f in fl]
    lines += [f'printf("8:{f[0]} %zu\\n", offsetof(vd_yuv420, {f[0]}));' for f in _lib.vd_yuv420._fields_]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.vd_yuv420_16)
    for f in fl:
        assert int(out[f]) == getattr(_lib.vd_yuv420_16, f).offset, f
    for f in _lib.vd_yuv420._fields_:
        assert out["8:" + f[0]] == out[f[0]], f[0]


def test_entries_are_exported_and_bound():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in ("vd_process_yuv420_16", "vd_mosaic_yuv420_16", "vd_smooth_yuv420_16", "vd_yuv420_16_to_rgb",
                 "vdt_letterbox_yuv420_16"):
        assert hasattr(lib, name), name
        assert name in bound, name
    for name in ("process_yuv420_16", "mosaic_yuv420_16", "smooth_yuv420_16", "letterbox_yuv420_16"):
        assert callable(getattr(vdmi.Context, name)), name
    assert callable(vdmi.yuv420_16_to_rgb) and vdmi.Yuv420_16 is not None
    assert lib.vd_abi_version() == 2


def test_header_names_what_is_not_offered():
    text = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    block = text[text.index("10- and 12-bit 4:2:0 frames"):text.index("typedef struct vd_yuv420_16")]
    for word in ("look-ahead", "tiling", "fixed Gaussian", "depth or shift conversion", "16-bit-deep", "4:2:2", "4:4:4"):
        assert word in block, word


def test_reference_layout_helpers_round_trip():
    s = y16.noise(2, 6, 10, 10, 0, 0)
    for lay in y16.LAYOUTS:
        t = y16.relayout(s, "nv12", lay)
        assert np.array_equal(y16.relayout(t, lay, "nv12"), s), lay
        # the 8-bit helper on the byte planes moves the same samples
        assert np.array_equal(y16.lo(t), yr.from_nv12(y16.lo(s), lay)) and np.array_equal(y16.hi(t), yr.from_nv12(y16.hi(s), lay))
        buf, fd = y16.padded(t, lay, 13, 7 * (2 if lay in y16.INTERLEAVED else 1), 8, lay in ("yv12", "nv21"), 5, base_pad_w=3)
        assert np.array_equal(y16.unpadded(buf, fd, 2, 6, 10, lay), t), lay
        m = y16.picture_mask(fd, 2, 6, 10, buf.size)
        assert int(m.sum()) == 2 * 6 * 10 * 3 // 2 and (buf[~m] == 0xA5A5).all()
    assert np.array_equal(y16.join(y16.lo(s), y16.hi(s)), s)
    assert np.array_equal(y16.D(y16.widen(y16.D(s, 10, 0), 12, 4, 1), 12, 4), y16.D(s, 10, 0))


# ---- the host conversion ---------------------------------------------------------------------------

@pytest.mark.parametrize("depth,shift", FORMATS)
@pytest.mark.parametrize("layout", y16.LAYOUTS)
def test_host_conversion_equals_the_8_bit_conversion_on_D(layout, depth, shift):
    """vd_yuv420_16_to_rgb = vd_yuv420_to_rgb on D(S), with random bits in the unused positions (a
    missing mask or shift would show), packed and padded."""
    import vdmi
    for (h, w), (m, r) in zip(((2, 2), (6, 10), (48, 64)), (("bt709", "limited"), ("bt601", "full"), ("bt601", "limited"))):
        s = y16.noise(2, h, w, depth, shift, 100 * depth + shift + h)
        want = vdmi.yuv420_to_rgb(y16.D(s, depth, shift), layout, matrix=m, range=r)
        assert np.array_equal(want, nr.to_rgb(yr.to_nv12(y16.D(s, depth, shift), layout), m, r))
        got = vdmi.yuv420_16_to_rgb(s, layout, depth=depth, shift=shift, matrix=m, range=r)
        np.testing.assert_array_equal(got, want, err_msg=f"{h}x{w}")
        step = 2 if layout in y16.INTERLEAVED else 1
        buf, fd = y16.padded(s, layout, w + 5, (w // 2 + 3) * step, h + 2, layout in ("yv12", "nv21"), 9, base_pad_w=1)
        d = vdmi.Yuv420_16(buf[fd["base"] // 2:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                           fd["chroma_step"], fd["frame_stride"], depth=depth, shift=shift)
        assert d.n == 2
        np.testing.assert_array_equal(vdmi.yuv420_16_to_rgb(d, matrix=m, range=r), want, err_msg="padded")
        # the same bytes handed over as a uint8 buffer
        d8 = vdmi.Yuv420_16(buf[fd["base"] // 2:].view(np.uint8), h, w, fd["pitch"], fd["u_offset"], fd["v_offset"],
                            fd["chroma_pitch"], fd["chroma_step"], fd["frame_stride"], depth=depth, shift=shift)
        np.testing.assert_array_equal(vdmi.yuv420_16_to_rgb(d8, matrix=m, range=r), want, err_msg="uint8 buffer")


def test_default_shift_is_the_p010_convention():
    import vdmi
    s = y16.noise(1, 4, 6, 10, 6, 3)
    np.testing.assert_array_equal(vdmi.yuv420_16_to_rgb(s, "nv12"), vdmi.yuv420_to_rgb(y16.D(s, 10, 6), "nv12"))
    np.testing.assert_array_equal(vdmi.yuv420_16_to_rgb(s, "i420"), vdmi.yuv420_to_rgb(y16.D(s, 10, 0), "i420"))
    np.testing.assert_array_equal(vdmi.yuv420_16_to_rgb(s, "nv21", depth=12), vdmi.yuv420_to_rgb(y16.D(s, 12, 4), "nv21"))


# ---- descriptor rules ------------------------------------------------------------------------------

def test_descriptor_rules_answer_err_arg_and_name_the_field():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    h, w, n = 8, 12, 2
    buf = np.zeros(8192, np.uint16)
    rgb = np.zeros((n, h, w, 3), np.uint8)
    yb, cb = 2 * w * h, w * (h // 2)                              # bytes of a packed luma / planar chroma plane
    planar = dict(pitch=2 * w, u=yb, v=yb + cb, cp=w, st=yb + 2 * cb, step=1, matrix=1, range=0, depth=10, shift=0)
    inter = dict(planar, v=yb + 2, cp=2 * w, step=2, depth=10, shift=6)

    def call(base=None, nn=n, hh=h, ww=w, **kw):
        d = _lib.vd_yuv420_16(buf.ctypes.data if base is None else base, kw["pitch"], kw["u"], kw["v"], kw["cp"], kw["st"],
                              kw["step"], kw["matrix"], kw["range"], kw["depth"], kw["shift"])
        rc = lib.vd_yuv420_16_to_rgb(ctypes.byref(d), nn, hh, ww, rgb.ctypes.data, 3 * w)
        return rc, lib.vd_last_error().decode()

    assert call(**planar)[0] == 0 and call(**inter)[0] == 0
    assert call(**dict(inter, u=yb + 2, v=yb))[0] == 0            # V first
    assert call(**dict(planar, depth=12, shift=4))[0] == 0
    bad = [
        (dict(planar, pitch=2 * w + 1), "pitch"), (dict(planar, pitch=2 * w - 2), "pitch"), (dict(planar, pitch=w), "pitch"),
        (dict(planar, cp=w + 1, st=4096), "chroma_pitch"), (dict(planar, cp=w - 2), "chroma_pitch"),
        (dict(inter, cp=2 * w - 2), "chroma_pitch"),
        (dict(planar, u=yb + 1, v=yb + 1 + cb, st=4096), "u_offset"), (dict(planar, v=yb + cb + 1, st=4096), "v_offset"),
        (dict(planar, st=yb + 2 * cb + 1), "frame_stride"), (dict(planar, st=yb + 2 * cb - 2), "frame_stride"),
        (dict(planar, depth=8), "depth"), (dict(planar, depth=16), "depth"), (dict(planar, depth=11), "depth"),
        (dict(planar, shift=7), "shift"), (dict(planar, shift=-1), "shift"), (dict(planar, depth=12, shift=5), "shift"),
        (dict(inter, v=yb + 1), "u_offset - v_offset"), (dict(inter, v=yb + 4), "u_offset - v_offset"),
        (dict(inter, u=yb + 2, v=yb + 2), "u_offset - v_offset"),
        (dict(planar, u=yb - 2), "u_offset"), (dict(planar, v=yb + cb - 2), "v_offset"), (dict(planar, v=yb - 2), "v_offset"),
        (dict(inter, u=yb - 4, v=yb - 2), "u_offset"), (dict(inter, u=yb - 2, v=yb - 4), "v_offset"),
        (dict(planar, step=3), "chroma_step"), (dict(planar, step=0), "chroma_step"),
        (dict(planar, matrix=2), "matrix"), (dict(planar, range=5), "range"),
    ]
    for kw, field in bad:
        rc, msg = call(**kw)
        assert rc == _lib.VD_ERR_ARG, (kw, rc)
        assert field in msg, (kw, msg)
    for kw, field in ((dict(hh=7), "h and w"), (dict(ww=11), "h and w"), (dict(nn=0), "n > 0"),
                      (dict(base=buf.ctypes.data + 1), "base"), (dict(base=0), "base")):
        rc, msg = call(**dict(planar, **kw))
        assert rc == _lib.VD_ERR_ARG and field in msg, (kw, msg)
    # one frame may reach past frame_stride; two may not
    assert call(nn=1, **dict(planar, st=2))[0] == 0


# ---- the reference checks itself ---------------------------------------------------------------------

BOXES = [(3, 5, 41, 37), (30, 20, 70, 60), (-9, -4, 13, 9), (50, 1, 64, 47), (7, 9, 8, 10), (20, 30, 22, 32), (10, 10, 60, 44)]


@pytest.mark.parametrize("level,cells", [(8, 8), (3, 2), (9, 5), (1, 3)])
def test_smooth_reference_at_depth_8_is_the_nv12_reference(level, cells):
    f = np.random.default_rng(level).integers(0, 256, (72, 64), dtype=np.uint8)
    want = nm.smooth(f, BOXES, level, cells)
    assert not np.array_equal(want, f)
    got = y16.smooth(f.astype(np.uint16), BOXES, level, cells, 8, 0)
    np.testing.assert_array_equal(got, want.astype(np.uint16))
    # ... and with the 8 bits sitting higher in the word, junk below and above them
    s = y16.widen(f, 8, 5, 2)
    got = y16.smooth(s, BOXES, level, cells, 8, 5)
    owned = got != s
    np.testing.assert_array_equal(np.where(owned, got >> 5, f), np.where(owned, want, f))
    assert ((got[owned] & ~np.uint16(0xFF << 5)) == 0).all()


def test_smooth_reference_extreme_stays_inside_32_bits():
    """A frame of all-4095 samples, the largest level: every output value is 4095 (the reference asserts
    T < 2^32 on the way, the bound of the header)."""
    f = np.full((6, 4), 4095 << 4, np.uint16)
    out = y16.smooth(f, [(0, 0, 4, 4)], 32768, 2, 12, 4)
    assert (out == 4095 << 4).all()


@pytest.mark.parametrize("level,cells", [(8, 0), (3, 0), (2, 4)])
def test_lo_hi_pixelation_is_a_gather_of_whole_words(level, cells):
    """The definition pixelates the low and the high bytes apart. Pixelation is a pure sample copy with a
    map that does not depend on the data, so the two halves of every output word come from one input
    word: the word at the position that the same pixelation of a position index names."""
    h, w = 48, 64
    s = y16.noise(1, h, w, 10, 6, 7)[0]
    got = y16.mosaic(s[None], [BOXES], level, cells)[0]
    assert not np.array_equal(got, s)
    idx = np.empty_like(s)
    Yi, UVi = nr.planes(idx)
    Yi[...] = np.arange(h * w, dtype=np.uint16).reshape(h, w)
    UVi[...] = np.arange(h * w // 4, dtype=np.uint16).reshape(h // 2, w // 2, 1)
    where = y16.mosaic(idx[None], [BOXES], level, cells)[0]
    Yw, UVw = nr.planes(where)
    Ys, UVs = nr.planes(s)
    Yg, UVg = nr.planes(got)
    np.testing.assert_array_equal(Yg, Ys.reshape(-1)[Yw])
    for ch in range(2):
        assert np.array_equal(UVw[..., 0], UVw[..., 1])
        np.testing.assert_array_equal(UVg[..., ch], UVs[..., ch].reshape(-1)[UVw[..., ch]])
