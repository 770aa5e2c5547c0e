"""CPU checks of the NV12 frame format: the library's host conversion (vd_nv12_to_rgb, the routine the
letterbox kernels' conversion is compiled from) against the numpy definition in tests/nv12_ref.py,
the coefficient table, the descriptor's layout and its VD_ERR_ARG rules, and the properties of the
plane-wise reference mosaic that the GPU tests compare against. No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import nv12_ref as nr
from conftest import ROOT

TABLES = sorted(nr.COEF)


def _all_triples():
    """One 4096 x 4096 NV12 frame in which every (Y, U, V) triple occurs: chroma pair (cy, cx) holds
    (U, V) = (cy * 2048 + cx) divmod 256 -- all 65536 pairs over the first 32 chroma rows, repeated
    below -- and the four luma samples of pair (cy, cx) hold 4 * (cy // 32) + (0..3), so the 64
    bands of 32 chroma rows carry all 256 luma values against every pair."""
    h = w = 4096
    f = np.empty((h * 3 // 2, w), np.uint8)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    pair = (cy % 32) * 2048 + cx
    uv = f[h:].reshape(h // 2, w // 2, 2)
    uv[..., 0] = pair >> 8
    uv[..., 1] = pair & 255
    yy, xx = np.mgrid[0:h, 0:w]
    f[:h] = 4 * ((yy >> 1) // 32) + 2 * (yy & 1) + (xx & 1)
    return f


@pytest.fixture(scope="module")
def triples():
    f = _all_triples()
    Y, UV = nr.planes(f)
    key = (Y.astype(np.int64) << 16) | (UV[..., 0].repeat(2, 0).repeat(2, 1).astype(np.int64) << 8) | \
        UV[..., 1].repeat(2, 0).repeat(2, 1)
    assert np.unique(key).size == 1 << 24
    return f


@pytest.mark.parametrize("matrix,rng", TABLES)
def test_host_conversion_equals_the_definition_on_every_triple(triples, matrix, rng):
    import vdmi
    got = vdmi.nv12_to_rgb(triples[None], matrix=matrix, range=rng)
    assert np.array_equal(got, nr.to_rgb(triples[None], matrix, rng))


@pytest.mark.parametrize("matrix,rng", TABLES)
def test_table_is_the_rounded_real_coefficients(matrix, rng):
    real = nr.real_coefficients(matrix, rng)
    assert nr.COEF[(matrix, rng)] == tuple(int(np.floor(v + 0.5)) for v in real)


def test_known_answers():
    c = lambda y, u, v, m, r: tuple(int(x) for x in nr.convert(y, u, v, m, r))
    for m in ("bt601", "bt709"):
        assert c(16, 128, 128, m, "limited") == (0, 0, 0)
        assert c(235, 128, 128, m, "limited") == (255, 255, 255)
        assert c(0, 128, 128, m, "full") == (0, 0, 0)
        assert c(255, 128, 128, m, "full") == (255, 255, 255)
    # t = 298 * 224 + 128 = 66880; R = (66880 + 459 * 112) >> 8 = 462 -> 255; G = (66880 - 55 * -128 - 136 * 112)
    # >> 8 = 229; B = (66880 + 541 * -128) >> 8 = -10 -> 0
    assert c(240, 0, 240, "bt709", "limited") == (255, 229, 0)
    import vdmi
    f = np.array([[240, 240], [240, 240], [0, 240]], np.uint8)
    assert vdmi.nv12_to_rgb(f).reshape(4, 3).tolist() == [[255, 229, 0]] * 4


def test_round_trip_through_the_test_inverse_is_close():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (1, 8, 8, 3)).repeat(2, axis=1).repeat(2, axis=2).astype(np.uint8)
    for m, r in TABLES:
        back = nr.to_rgb(nr.from_rgb(base, m, r), m, r)
        assert np.abs(back.astype(int) - base).max() <= 3, (m, r)   # 2 x 2 constant blocks: rounding only


def test_nv12_struct_layout_matches_header(tmp_path):
    """The ctypes mirror of vd_nv12 has the C compiler's size and field offsets."""
    import shutil
    import subprocess
    from vdmi import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fl = [f[0] for f in _lib.vd_nv12._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdmi.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(vd_nv12));']
    lines += [f'printf("{f} %zu\\n", offsetof(vd_nv12, {f}));' for f in fl]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.vd_nv12)
    for f in fl:
        assert int(out[f]) == getattr(_lib.vd_nv12, f).offset, f


def _desc(buf, pitch, uv_offset, frame_stride, matrix=1, rng=0):
    from vdmi import _lib
    return _lib.vd_nv12(buf.ctypes.data, pitch, uv_offset, frame_stride, matrix, rng)


def test_host_err_arg_cases():
    from vdmi import _lib
    lib = _lib.load()
    h, w, n = 4, 6, 2
    buf = np.zeros(4096, np.uint8)
    rgb = np.zeros((n, h, w, 3), np.uint8)

    def call(d, n=n, h=h, w=w, out=rgb, rgb_pitch=w * 3):
        return lib.vd_nv12_to_rgb(ctypes.byref(d) if d is not None else None, n, h, w,
                                  out.ctypes.data if out is not None else None, rgb_pitch)

    good = dict(pitch=8, uv_offset=4 * 8, frame_stride=4 * 8 + 2 * 8)
    assert call(_desc(buf, **good)) == _lib.VD_OK
    assert call(_desc(buf, 8, 5 * 8, 5 * 8 + 2 * 8 + 3)) == _lib.VD_OK          # padded height and stride
    bad = [
        (dict(h=3), good, "odd h"), (dict(w=5), good, "odd w"), (dict(h=0), good, "h = 0"), (dict(w=-2), good, "w < 0"),
        (dict(n=0), good, "n = 0"),
        ({}, dict(good, pitch=4), "pitch < w"),
        ({}, dict(good, uv_offset=4 * 8 - 1), "uv_offset < h * pitch"),
        ({}, dict(good, frame_stride=4 * 8 + 2 * 8 - 1), "frame_stride too small"),
        ({}, dict(good, matrix=2), "unknown matrix"), ({}, dict(good, rng=-1), "unknown range"),
        (dict(rgb_pitch=w * 3 - 1), good, "rgb_pitch < 3 w"), (dict(out=None), good, "null rgb"),
    ]
    for kw, d, what in bad:
        rgb[:] = 7
        assert call(_desc(buf, **d), **kw) == _lib.VD_ERR_ARG, what
        assert (rgb == 7).all(), what
    assert call(None) == _lib.VD_ERR_ARG
    null = _lib.vd_nv12(None, 8, 32, 48, 1, 0)
    assert call(null) == _lib.VD_ERR_ARG


def test_padded_layout_reads_the_described_bytes():
    """pitch > w, a padded luma height and a padded frame stride: the pad bytes never matter."""
    import vdmi
    from vdmi import _lib
    rng = np.random.default_rng(5)
    n, h, w, pitch, H = 2, 6, 10, 16, 8
    stride = (H + H // 2) * pitch + 32
    packed = rng.integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    want = nr.to_rgb(packed)
    for fill in (0, 255):
        buf = np.full(n * stride, fill, np.uint8)
        for f in range(n):
            fr = buf[f * stride:f * stride + (H + H // 2) * pitch].reshape(H + H // 2, pitch)
            fr[:h, :w] = packed[f, :h]
            fr[H:H + h // 2, :w] = packed[f, h:]
        got = np.zeros((n, h, w, 3), np.uint8)
        d = _lib.vd_nv12(buf.ctypes.data, pitch, H * pitch, stride, 1, 0)
        assert _lib.load().vd_nv12_to_rgb(ctypes.byref(d), n, h, w, got.ctypes.data, w * 3) == _lib.VD_OK
        assert np.array_equal(got, want)
    # the Python form of the same: height= with a taller rows
    tall = np.zeros((n, H * 3 // 2, w), np.uint8)
    tall[:, :h] = packed[:, :h]
    tall[:, H:H + h // 2] = packed[:, h:]
    assert np.array_equal(vdmi.nv12_to_rgb(tall, height=h), want)


def _random_boxes(rng, h, w, k):
    out = []
    for _ in range(k):
        x1, y1 = int(rng.integers(-10, w + 5)), int(rng.integers(-10, h + 5))
        out.append((x1, y1, x1 + int(rng.integers(-3, w // 2)), y1 + int(rng.integers(-3, h // 2))))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_mosaic_properties(seed):
    rng = np.random.default_rng(seed)
    h, w, H = 36, 52, 40
    level, cells = [(1, 0), (2, 0), (8, 0), (9, 0), (3, 4), (8, 8)][seed]
    boxes = _random_boxes(rng, h, w, 6)
    frame = rng.integers(0, 256, (H * 3 // 2, w), dtype=np.uint8)
    out = nr.mosaic(frame, boxes, level, cells, height=h)
    Y0, UV0 = nr.planes(frame, h)
    Y1, UV1 = nr.planes(out, h)
    in_l = np.zeros((h, w), bool)
    in_c = np.zeros((h // 2, w // 2), bool)
    for b in boxes:
        c = nr.clip(b, h, w)
        if c is None:
            continue
        cc = nr.chroma_box(c)
        in_l[c[1]:c[3], c[0]:c[2]] = True
        in_c[cc[1]:cc[3], cc[0]:cc[2]] = True
        # every luma pixel of the clipped box has its chroma sample inside cc, and cc stays in the plane
        ys, xs = np.mgrid[c[1]:c[3], c[0]:c[2]]
        assert ((xs >> 1 >= cc[0]) & (xs >> 1 < cc[2]) & (ys >> 1 >= cc[1]) & (ys >> 1 < cc[3])).all()
        assert 0 <= cc[0] < cc[2] <= w // 2 and 0 <= cc[1] < cc[3] <= h // 2
    # bytes outside every box are untouched in both planes, and so are the pad rows
    assert np.array_equal(Y1[~in_l], Y0[~in_l]) and np.array_equal(UV1[~in_c], UV0[~in_c])
    assert np.array_equal(out[h:H], frame[h:H]) and np.array_equal(out[H + h // 2:], frame[H + h // 2:])
    # the result does not depend on the pad bytes
    other = frame.copy()
    other[h:H] = 255 - other[h:H]
    other[H + h // 2:] = 255 - other[H + h // 2:]
    out2 = nr.mosaic(other, boxes, level, cells, height=h)
    assert np.array_equal(nr.planes(out2, h)[0], Y1) and np.array_equal(nr.planes(out2, h)[1], UV1)
    # a pixelated sample is a source sample of its own plane (a pure gather)
    assert np.isin(Y1, Y0).all()


def test_chroma_cell_never_spans_fewer_luma_pixels_than_a_luma_cell():
    for L in range(1, 70):
        assert 2 * ((L + 1) >> 1) >= L
