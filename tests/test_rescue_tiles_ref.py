"""Rescue on tiled nets, CPU side (include/vdmi.h at vd_rescue_tiles): the prefix property the split inside
the tile merge rests on, pinned on the references alone (tests/rescue_tiles_ref.py composes tiles_ref /
plate_tiles_ref with rescue_ref); the history across call cuts; and the switch through the layers -- header,
library export, binding, Context, the drop-in detectors and batch_process_images."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import rescue_tiles_ref as rtr
import tiles_ref as tr
from conftest import ROOT

H, W = 360, 640
A = 16800            # the face net's anchor count at 640 x 640: label = t * A + anchor
IOU = {False: 0.4, True: 0.7}


def _rects(T):
    r = tr.tile_rects(H, W, 2, 2, 20) if T == 5 else tr.tile_rects(H, W, 4, 4, 20)
    assert len(r) == T
    return r


def _same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                                     y.view(np.uint32) if y.dtype == np.float32 else y)
    assert list(a[4]) == list(b[4])


@pytest.mark.parametrize("plates", [False, True], ids=["faces", "plates"])
@pytest.mark.parametrize("T", [5, 17])
def test_the_merge_at_low_cut_is_the_merge_of_the_strong_prefixes(T, plates):
    """The merged list at low, cut where the score stops passing the net's threshold, equals the merged list
    of the per-input strong prefixes field by field (and box by box: the same (t, pos) sources). The
    generated lists must show, on the reference alone, everything the argument is about."""
    rects = _rects(T)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    thr = rtr.PLATE_THR if plates else rtr.FACE_THR
    lists = rtr.random_lists(100 + T + plates, 2, rects, 64, plates=plates)
    strong = weak = by_other = weak_from_tile = at_thr = 0
    for f in range(2):
        li = lists.frame_lists(f, T)
        D, Wk, merged = rtr.split_frame(li, origins, A, IOU[plates], thr, plates)
        ref = rtr.merge_low(rtr.strong_prefixes(li, thr, plates), origins, A, IOU[plates], plates)
        _same(D, ref)
        strong += len(D[2])
        weak += len(Wk[2])
        by_other += rtr.suppressed_by_strong_of_another_input(li, origins, merged, len(D[2]), IOU[plates], plates)
        weak_from_tile += sum(1 for t, _ in Wk[4] if t > 0)
        # a face at exactly the threshold is strong, a plate at exactly the threshold is weak
        at_thr += int((np.asarray((Wk if plates else D)[2]) == np.float32(thr)).sum())
        assert not (np.asarray((D if plates else Wk)[2]) == np.float32(thr)).any()
        # scores repeat across inputs: the tie rule (lower t, then lower position) is exercised
        sc = np.asarray(merged[2])
        ties = [(merged[4][i], merged[4][i + 1]) for i in range(len(sc) - 1) if sc[i] == sc[i + 1]]
        assert any(a[0] != b[0] for a, b in ties) and all(a < b for a, b in ties)
    assert strong > 0 and weak > 0 and by_other > 0 and weak_from_tile > 0 and at_thr > 0


def _stream(frames, T, plates, seed):
    """Per frame D_t and W_t (int boxes) of one net: an object list that persists over the frames, each input
    scoring each object anew per frame (so a track is strong in one frame and weak in the next)."""
    rects = _rects(T)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    thr = rtr.PLATE_THR if plates else rtr.FACE_THR
    D, Wk = [], []
    for f in range(frames):
        # the same seed: the same objects and labels in every frame; other scores through another score order
        sc = rtr.SCORES[f % 3:] + rtr.SCORES[:f % 3]
        li = rtr.random_lists(seed, 1, rects, 24, plates=plates, scores=sc[:4] if f % 2 else sc[2:]).frame_lists(0, T)
        d, w, _ = rtr.split_frame(li, origins, A, IOU[plates], thr, plates)
        D.append(d[0])
        Wk.append(w[0])
    return D, Wk


@pytest.mark.parametrize("hold", [1, 2])
def test_history_across_call_cuts(hold):
    """Six frames run as 2 + 2 + 2 and one at a time give the E and since of one call: faces merged from five
    inputs beside plates merged per class."""
    fd, fw = _stream(6, 5, False, 7)
    pd, pw = _stream(6, 5, True, 8)
    strong = [np.concatenate([a, b]) for a, b in zip(fd, pd)]
    weak = [np.concatenate([a, b]) for a, b in zip(fw, pw)]
    Wn, S, P = max(1, hold), 3, 30
    E, SI, R, _, _ = rtr.rescue_stream(strong, weak, H, W, Wn, S, P)
    assert sum(len(r) for r in R) > 0 and sum(len(w) - len(r) for w, r in zip(weak, R)) > 0
    for step in (2, 1):
        hist, e2, s2 = None, [], []
        for s0 in range(0, 6, step):
            e, s, _, _, hist = rtr.rescue_stream(strong[s0:s0 + step], weak[s0:s0 + step], H, W, Wn, S, P, hist)
            e2 += e
            s2 += s
        assert e2 == E and s2 == SI, step


# ---- the switch through the layers ----
def test_header_declares_the_switch():
    text = " ".join(open(os.path.join(ROOT, "include", "vdmi.h")).read().split()).replace(" * ", " ")
    assert "int vd_rescue_tiles(vd_ctx* ctx, int on);" in text
    assert "int vdt_tiles_merge_low(vd_ctx* ctx, const vd_boxes* lists, int n, int h, int w, int plates, float thr, " \
           "vd_boxes* out_strong, vd_boxes* out_all);" in text
    assert "Rescue with tiling is refused unless vd_rescue_tiles" in text


def test_library_exports_the_switch():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    assert lib.vd_rescue_tiles(None, 1) == _lib.VD_ERR_ARG and "null context" in _lib.last_error()
    sig = {s[0]: s for s in _lib.SIGNATURES}["vd_rescue_tiles"]
    assert sig[1] is ctypes.c_int and sig[2] == [ctypes.c_void_p, ctypes.c_int]
    assert lib.vdt_tiles_merge_low(None, None, 1, 2, 2, 0, 0.5, None, None) == _lib.VD_ERR_ARG
    assert "null context" in _lib.last_error()
    sig = {s[0]: s for s in _lib.SIGNATURES}["vdt_tiles_merge_low"]
    assert len(sig[2]) == 9 and sig[2][6] is ctypes.c_float and sig[2][8] == ctypes.POINTER(_lib.vd_boxes)


def test_python_carries_the_keyword():
    import vdmi
    from vdmi import _lib, pipeline
    from vdmi.face import Retinaface
    from vdmi.plate import YOLO
    assert inspect.signature(vdmi.Context.__init__).parameters["rescue_tiles"].default is False
    assert list(inspect.signature(vdmi.Context.set_rescue_tiles).parameters) == ["self", "on"]
    assert Retinaface.get_defaults("rescue_tiles") is False
    assert inspect.signature(YOLO.__init__).parameters["rescue_tiles"].default is False
    assert inspect.signature(pipeline.batch_process_images).parameters["rescue_tiles"].default is False
    # checked before the library is touched: no device is needed to be told
    assert _lib.check_rescue_tiles(True) is True and _lib.check_rescue_tiles(0) is False
    for bad in (2, -1, "on", None, 1.0):
        with pytest.raises(ValueError, match="rescue_tiles"):
            _lib.check_rescue_tiles(bad)
        with pytest.raises(ValueError, match="rescue_tiles"):
            vdmi.Context(precision="fp32", max_batch=1, rescue_tiles=bad)
        with pytest.raises(ValueError, match="rescue_tiles"):
            Retinaface(weights="random", rescue_tiles=bad)
        with pytest.raises(ValueError, match="rescue_tiles"):
            YOLO(weights="random", rescue_tiles=bad)


def test_batch_process_images_checks_the_agreement(tmp_path):
    """The keyword must be what the detectors were built with; the check comes before a file is read."""
    from vdmi import pipeline

    class Ctx:
        rescue_tiles = False

    class Det:
        ctx = Ctx()

    with pytest.raises(ValueError, match="rescue_tiles"):
        pipeline.batch_process_images(str(tmp_path), str(tmp_path / "out"), Det(), Det(), rescue_tiles=True)
    with pytest.raises(ValueError, match="rescue_tiles"):
        pipeline.batch_process_images(str(tmp_path), str(tmp_path / "out"), Det(), Det(), rescue_tiles="yes")
