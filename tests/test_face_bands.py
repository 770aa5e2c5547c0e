"""Letterbox bands, host side (no GPU): the library's row rule (face_bands.h through
vdt_face_band_rows) against a brute-force propagation of "depends on band rows only" through the
stem's and layer1's conv and pool steps, and against the closed-form rule of face_bands_ref.py."""
import numpy as np
import pytest

import face_bands_ref as ref

# (canvas rows, top, nh, left): 1920x1080 in 640x640; 256x64 in 256x256; 256x128; an odd top;
# a portrait frame (bands are columns); a square frame (no bands)
CASES = [(640, 140, 360, 0), (256, 96, 64, 0), (256, 64, 128, 0), (640, 107, 426, 0), (640, 0, 640, 140),
         (640, 0, 640, 0), (256, 0, 256, 0)]


def _lib_rows(canvas_h, top, nh, left):
    from vdmi import _lib
    out = np.zeros((4, 5), np.int32)
    _lib.check(_lib.load().vdt_face_band_rows(canvas_h, top, nh, left, _lib.ptr(out)))
    return out


@pytest.mark.parametrize("case", CASES)
def test_rows_match_brute_force(case):
    canvas_h = case[0]
    got = _lib_rows(*case)
    dep = ref.brute(*case)
    for k in range(4):
        te, bb, tr, lo, hi = (int(v) for v in got[k])
        h = len(dep[k])
        assert h == (canvas_h // 4)
        y = np.arange(h)
        assert np.array_equal(dep[k], (y < te) | (y >= bb)), (k, te, bb)
        # a band tile holds band rows only; the first and last tiles kept hold an image row
        th = ref.TILE_H[k]
        assert tr == -(-h // th)
        for t in range(tr):
            rows = dep[k][t * th:(t + 1) * th]
            assert (t < lo or t >= hi) <= bool(rows.all()), (k, t)
        if (lo, hi) != (0, tr):
            assert not dep[k][lo * th:(lo + 1) * th].all() and not dep[k][(hi - 1) * th:hi * th].all()


@pytest.mark.parametrize("case", CASES)
def test_rows_match_closed_form(case):
    got = _lib_rows(*case)
    assert [tuple(int(v) for v in r) for r in got] == ref.rule(*case)


def test_values_at_1080p_and_without_bands():
    got = _lib_rows(640, 140, 360, 0)
    # pool map rows 0..33 / 127.., layer1 blocks 0..32 / 128.., 0..31 / 129.., 0..30 / 130..
    assert [(int(r[0]), int(r[1])) for r in got] == [(34, 127), (33, 128), (32, 129), (31, 130)]
    # 5 + 5 of the stem's 27 tile rows of 6; 8, 7 and 6 of the blocks' 20 tile rows of 8
    assert [(int(r[2]), int(r[3]), int(r[4])) for r in got] == [(27, 5, 22), (20, 4, 16), (20, 4, 17), (20, 3, 17)]
    for case in [(640, 0, 640, 140), (640, 0, 640, 0)]:   # column bands, no bands: nothing qualifies
        for r in _lib_rows(*case):
            assert (int(r[0]), int(r[1]), int(r[3]), int(r[4])) == (0, 160, 0, int(r[2]))
