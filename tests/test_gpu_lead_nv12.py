"""Look-ahead hold on NV12 surfaces on the GPU (vd_process_lead_nv12; csrc/nv12.hip's ring push,
csrc/track.cpp's NV12 branch of the lead step). Nothing new is defined, so everything is checked
against existing definitions: the lists against vd_process_lead on the converted RGB stream in a
twin context and against tests/lead_ref.py, the pixels against the plane-wise references
(tests/nv12_ref.py, tests/nv12_modes_ref.py) over B_t."""
import ctypes

import numpy as np
import pytest

import lead_ref as lr
import nv12_modes_ref as nm
import nv12_ref as nr
from test_gpu_hold import _frame, _lists, _rows

pytestmark = pytest.mark.gpu

H, W, J, P = 360, 640, 2, 30
BOX = (10, 10, 30, 30)

_NETS = {}


@pytest.fixture(scope="module")
def nets(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by keyword arguments (max_batch 4 unless
    given; `tag` tells twins with equal settings apart)."""
    import vdmi
    from vdmi import weights

    def make(tag="", **kw):
        key = (tag,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in _NETS:
            args = dict(precision="fp32", max_batch=4)
            args.update(kw)
            c = vdmi.Context(**args)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[key] = c
        c = _NETS[key]
        c.hold_reset()
        c.set_cells(kw.get("cells", 0))
        return c

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


@pytest.fixture(scope="module")
def clip():
    """tests/test_gpu_lead.py's [A, A, B, B, C, A] clip as packed NV12 [6, 540, 640]."""
    a, b, c = nr.from_rgb(np.stack([_frame(0), _frame(1), _frame(2)]))
    return np.stack([a, a, b, b, c, a])


def _flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _run(ctx, frames, calls, device=False, rgb=False):
    """frames through process_lead_nv12 (rgb: process_lead) in `calls` then a flush: the emitted
    frames in order, D of every pushed frame, read_lead's (B_t, labels) of every emitted frame, every
    call's m, and whether some call emitted both from the ring and from its own frames."""
    outs, D, B, ms, lo, both = [], [], [], [], 0, False
    for n in list(calls) + [0]:
        pend = ctx.lead_pending()
        if n:
            batch = frames[lo:lo + n]
            push = ctx.process_lead if rgb else ctx.process_lead_nv12
            out, faces, plates = push(_dev(batch) if device else batch, flags=_flags())
            D += [_lists(faces, b) + _lists(plates, b) for b in range(n)]
        else:
            out = ctx.lead_flush()
        m = len(out)
        ms.append(m)
        both = both or 0 < pend < m
        if m:
            rows = ctx.read_lead(m, "all")
            B += [_rows(rows, i) for i in range(m)]
        outs += list(_np(out))
        lo += n
    assert ctx.lead_pending() == 0
    return outs, D, B, ms, both


# ---- 1: the lists are the RGB twin's ----------------------------------------------------------------

@pytest.mark.parametrize("calls", [(4, 2), (3, 3)])
@pytest.mark.parametrize("K", [0, 2])
def test_lists_equal_the_rgb_twin(nets, clip, K, calls):
    import vdmi
    _, D, B, ms, both = _run(nets(lead=J, hold=K), clip, calls)
    _, D2, B2, ms2, _ = _run(nets("twin", lead=J, hold=K), vdmi.nv12_to_rgb(clip), calls, rgb=True)
    assert D == D2 and B == B2 and ms == ms2
    assert ms == ([2, 2, 2] if calls == (4, 2) else [1, 3, 2])
    wantB, wantL = lr.blur_lists(D, H, W, J, P, K=K)
    assert [b for b, _ in B] == wantB and [l for _, l in B] == wantL
    assert any(v < 0 for l in wantL for v in l)                   # some A_t is non-empty
    assert both == (calls == (3, 3))                              # (3, 3): 2 from the ring and 1 from `in`


# ---- 2: the pixels are the plane-wise references over B_t --------------------------------------------

MODES = {
    "pixelate": (dict(), 0, lambda fr, b: nr.mosaic(fr, b, 8, 0)),
    "smooth_ellipse": (dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42, hold=2), 2,
                       lambda fr, b: nm.shaped(fr, b, "ellipse", 42, lambda f, bb: nm.smooth(f, bb, 8, 8))),
    "cells": (dict(cells=4), 0, lambda fr, b: nr.mosaic(fr, b, 8, 4)),
}
_WANT = {}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_pixels(nets, clip, mode, device):
    kw, K, render = MODES[mode]
    outs, D, B, ms, _ = _run(nets(lead=J, **kw), clip, (4, 2), device)
    assert ms == [2, 2, 2] and len(outs) == 6
    wantB, wantL = lr.blur_lists(D, H, W, J, P, K=K)
    assert [b for b, _ in B] == wantB and any(v < 0 for l in wantL for v in l)
    key = (mode, repr(wantB))
    if key not in _WANT:                                          # host and device share the reference
        _WANT[key] = [render(clip[t], wantB[t]) for t in range(6)]
    for t in range(6):
        np.testing.assert_array_equal(outs[t], _WANT[key][t], err_msg=f"frame {t}")
    off, outs0, lo = nets(**kw), [], 0
    for n in (4, 2):
        o, f, p = off.process_nv12(clip[lo:lo + n], flags=_flags())
        assert [_lists(f, b) + _lists(p, b) for b in range(n)] == D[lo:lo + n]
        outs0 += list(o)
        lo += n
    assert any(not np.array_equal(x, y) for x, y in zip(outs, outs0))


# ---- 3: the cut into calls does not matter ------------------------------------------------------------

@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_cut_invariance(nets, clip, motion):
    ctx = nets(lead=J, lead_motion=motion, max_batch=6)
    cuts = [(1,) * 6, (6,)] if motion else [(1,) * 6, (3, 2, 1), (6,), (2, 4)]
    delay = J + (1 if motion else 0)
    want = None
    for c in cuts:
        outs, D, B, ms, _ = _run(ctx, clip, c, device=c == (6,))
        pend, exp = 0, []
        for n in c:
            exp.append(max(0, pend + n - delay))
            pend += n - exp[-1]
        assert ms == exp + [pend], c
        if want is None:
            want = (outs, D, B)
            assert any(v < 0 for _, l in B for v in l)
            continue
        assert D == want[1] and B == want[2], c
        for t in range(6):
            np.testing.assert_array_equal(outs[t], want[0][t], err_msg=f"{c} frame {t}")


# ---- 4: the ring push at awkward layouts --------------------------------------------------------------

def _surfaces(frames, h, Hp, pitch, slack, offset, fill, room=None):
    """Packed frames [k, 3h/2, w] laid out in a device buffer filled with `fill`: rows at `pitch`, the
    luma plane padded to Hp rows, frames `slack` bytes further apart than their rows, the first byte
    `offset` bytes in; the buffer holds `room` >= k surfaces. -> (vd_nv12, the device buffer, its host image)."""
    from vdmi import _lib
    k, _, w = frames.shape
    fstride = Hp * 3 // 2 * pitch + slack
    host = np.full(offset + max(room or k, k) * fstride + 16, fill, np.uint8)
    for i in range(k):
        b = offset + i * fstride
        host[b:b + h * pitch].reshape(h, pitch)[:, :w] = frames[i, :h]
        c = b + Hp * pitch
        host[c:c + h // 2 * pitch].reshape(h // 2, pitch)[:, :w] = frames[i, h:]
    buf = _dev(host)
    return _lib.vd_nv12(buf.data_ptr() + offset, pitch, Hp * pitch, fstride, 1, 0), buf, host


def _raw(ctx, ind, outd, n, h, w, where, cap, flush, flags=None):
    from vdmi import _lib
    m = ctypes.c_int(-7)
    hb = _lib.HostBoxes(max(n, 1), 64)
    s = hb.struct()
    rc = ctx._lib.vd_process_lead_nv12(ctx._h, ctypes.byref(ind) if ind is not None else None,
                                       ctypes.byref(outd) if outd is not None else None, n, h, w, where,
                                       _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC if flags is None else flags,
                                       ctypes.byref(s), None, cap, 1 if flush else 0, ctypes.byref(m))
    return rc, m.value


LAYOUTS = [(134, 104, 7, 1), (144, 104, 7, 16), (134, 104, 7, 16), (144, 104, 7, 1), (131, 98, 0, 3)]


@pytest.mark.parametrize("h,w,cuts,aligned", [(98, 130, (1, 1, 1, 1, 1), False), (98, 130, (3, 2), False),
                                              (96, 128, (1, 1, 1, 1, 1), True)])
def test_ring_push_layouts(nets, h, w, cuts, aligned):
    """Noise surfaces in changing device layouts, one frame per call so every frame passes through
    the ring ((3, 2): two surfaces in one launch): each emitted surface is the reference over its
    B_t -- the input itself where B_t is empty -- and the pad bytes of `out` keep their pattern."""
    from vdmi import _lib
    ctx = nets(lead=J)
    f = np.random.default_rng(h + len(cuts)).integers(0, 256, (5, h * 3 // 2, w), dtype=np.uint8)
    got, lo = 0, 0
    for i, n in enumerate(list(cuts) + [0]):
        pitch, Hp, slack, offset = (w, h, 0, 0) if aligned else LAYOUTS[i % len(LAYOUTS)]
        opitch, oHp, oslack, ooffset = (w, h, 0, 0) if aligned else LAYOUTS[(i + 2) % len(LAYOUTS)]
        room = ctx.lead_pending() + n
        ind = None
        if n:
            ind, ibuf, _ = _surfaces(f[lo:lo + n], h, Hp, pitch, slack, offset, 0xA5)
        outd, obuf, _ = _surfaces(np.zeros((room, h * 3 // 2, w), np.uint8), h, oHp, opitch, oslack, ooffset, 0x5A)
        obuf[:] = 0x5A
        rc, m = _raw(ctx, ind, outd, n, h, w, _lib.VD_DEVICE, room, n == 0)
        assert rc == _lib.VD_OK, _lib.last_error()
        assert m == (room if n == 0 else max(0, room - J))
        if m:
            rows = ctx.read_lead(m, "all")
            want = np.stack([nr.mosaic(f[got + t], _rows(rows, t)[0], 8, 0) for t in range(m)])
            for t in range(m):
                if not _rows(rows, t)[0]:
                    np.testing.assert_array_equal(want[t], f[got + t])
            _, _, exp = _surfaces(want, h, oHp, opitch, oslack, ooffset, 0x5A, room)
            np.testing.assert_array_equal(obuf.cpu().numpy(), exp, err_msg=f"call {i}")
        else:
            assert (obuf.cpu().numpy() == 0x5A).all()
        got += m
        lo += n
    assert got == 5 and ctx.lead_pending() == 0


# ---- 5: refusals ----------------------------------------------------------------------------------------

def _code(fn, *a, match=None, **k):
    from vdmi import _lib
    with pytest.raises(_lib.VdError, match=match) as e:
        fn(*a, **k)
    return e.value.code


def test_refusals(nets, clip):
    import vdmi
    from vdmi import _lib
    S, AR, CAP = _lib.VD_ERR_STATE, _lib.VD_ERR_ARG, _lib.VD_ERR_CAPACITY
    HOST, DEV = _lib.VD_HOST, _lib.VD_DEVICE
    ctx = nets(lead=J, blur="gaussian", cells=8)
    want, _, wantB, _, _ = _run(ctx, clip, (4, 2))
    rgb = vdmi.nv12_to_rgb(clip)
    want_rgb, _, _, _, _ = _run(ctx, rgb[:3], (1, 2), rgb=True)

    def desc(a, n, h, w, pitch=None):
        pitch = pitch or w
        return _lib.vd_nv12(a.ctypes.data, pitch, h * pitch, h * pitch * 3 // 2, 1, 0)

    ibuf, obuf = np.ascontiguousarray(clip[:4]), np.zeros_like(clip[:4])
    ok_in, ok_out = desc(ibuf, 4, H, W), desc(obuf, 4, H, W)

    def refused(pend):
        """Every refusal that does not need a state of its own, with `pend` frames pending."""
        assert _raw(ctx, desc(ibuf, 4, H, W, pitch=W - 2), ok_out, 1, H, W, HOST, 4, 0) == (AR, -7)      # pitch < w
        assert _raw(ctx, ok_in, ok_out, 1, H - 1, W, HOST, 4, 0) == (AR, -7)                            # odd h
        assert _raw(ctx, ok_in, ok_out, 1, H, W - 1, HOST, 4, 0) == (AR, -7)                            # odd w
        assert _raw(ctx, None, ok_out, 1, H, W, HOST, 4, 0) == (AR, -7)                                 # no descriptor
        assert _raw(ctx, ok_in, ok_out, 1, H, W, 7, 4, 0) == (AR, -7)                                   # bad where
        assert _raw(ctx, ok_in, ok_out, 1, H, W, HOST, 4, 0, flags=_lib.VD_PROC_FACES) == (AR, -7)      # no MOSAIC
        assert _raw(ctx, ok_in, ok_out, 1, H, W, HOST, 4, 0,
                    flags=_lib.VD_PROC_MOSAIC | _lib.VD_PROC_PLATES) == (AR, -7)                        # nothing to blur
        assert _raw(ctx, None, None, 0, H, W, HOST, 0, 0) == (AR, -7)                                   # n == 0 without flush
        assert _raw(ctx, ok_in, ok_out, 4, H, W, HOST, pend + 1, 0) == (CAP, -7)                        # m = pend + 2
        assert _raw(ctx, ok_in, None, 4, H, W, HOST, 4, 0) == (AR, -7)                                  # m > 0, out NULL
        assert _raw(ctx, ok_in, desc(obuf, 4, H, W, pitch=W - 2), 4, H, W, HOST, 4, 0) == (AR, -7)      # bad out
        d = _dev(np.concatenate([clip[:4], clip[:4]]))
        di = _lib.vd_nv12(d.data_ptr(), W, H * W, H * W * 3 // 2, 1, 0)
        do = _lib.vd_nv12(d.data_ptr() + 3 * (H * W * 3 // 2), W, H * W, H * W * 3 // 2, 1, 0)
        assert _raw(ctx, di, do, 4, H, W, DEV, 4, 0) == (AR, -7)                                        # out overlaps in
        ctx.set_cells(0)                                                                                 # the fixed Gaussian
        assert _code(ctx.process_lead_nv12, clip[:1], match="cells") == S
        ctx.set_cells(8)
        assert ctx.lead_pending() == pend

    # nothing pending: the refusals, tiling (a change of tiling is itself refused while frames are pending)
    refused(0)
    ctx.set_tiles((2, 2), 20)
    try:
        assert _code(ctx.process_lead_nv12, clip[:1], match="tile") == S
    finally:
        ctx.set_tiles((1, 1), 20)
    assert ctx.lead_pending() == 0
    assert _raw(ctx, None, None, 0, H, W, HOST, 0, 1) == (_lib.VD_OK, 0)                                # an empty stream ends
    # NV12 frames pending: the same refusals, another geometry, the other entry points
    outs = list(ctx.process_lead_nv12(clip[:4], flags=_flags())[0])
    assert len(outs) == 2 and ctx.lead_pending() == 2
    refused(2)
    assert _code(ctx.process_lead_nv12, clip[:1, :H * 3 // 2 - 12], match="pending") == S               # 352 x 640
    assert _code(ctx.process_lead_nv12, clip[:1, :, :W - 8], match="pending") == S                      # 360 x 632
    assert _code(ctx.process_lead, rgb[:1], match="vd_process_lead_nv12") == S
    assert _code(ctx.lead_lists, [[BOX]], H, W, match="vd_process_lead_nv12") == S
    assert _code(ctx.process_nv12, clip[:1], flags=_lib.VD_PROC_FACES) == S
    assert _code(ctx.process, rgb[:1], flags=_lib.VD_PROC_FACES) == S
    assert _code(ctx.set_lead, 3, False) == S
    assert ctx.lead_pending() == 2
    outs += list(ctx.process_lead_nv12(clip[4:], flags=_flags())[0])
    assert [_rows(ctx.read_lead(2, "all"), i) for i in range(2)] == wantB[2:4]
    outs += list(ctx.lead_flush())
    assert len(outs) == 6 and ctx.lead_pending() == 0
    for t in range(6):
        np.testing.assert_array_equal(outs[t], want[t], err_msg=f"frame {t}")
    # RGB frames pending, then lists pending: the NV12 call is refused and their streams go on
    outs = list(ctx.process_lead(rgb[:1], flags=_flags())[0])
    assert ctx.lead_pending() == 1
    assert _code(ctx.process_lead_nv12, clip[:1], match="vd_process_lead \\(flush first\\)") == S
    assert _raw(ctx, None, ok_out, 0, H, W, HOST, 4, 1) == (S, -7)                                      # nor may it flush them
    assert ctx.lead_pending() == 1
    outs += list(ctx.process_lead(rgb[1:3], flags=_flags())[0]) + list(ctx.lead_flush())
    assert len(outs) == 3
    for t in range(3):
        np.testing.assert_array_equal(outs[t], want_rgb[t], err_msg=f"rgb frame {t}")
    ctx.lead_lists([[BOX]], H, W)
    assert _code(ctx.process_lead_nv12, clip[:1], match="vd_lead_lists") == S and ctx.lead_pending() == 1
    out = ctx.lead_lists(None, H, W, flush=True)
    assert out.n == 1 and _rows(out, 0) == ([BOX], [0])
    # hold_reset abandons pending NV12 frames; the next stream starts clean
    ctx.process_lead_nv12(clip[:2], flags=_flags())
    assert ctx.lead_pending() == 2
    ctx.hold_reset()
    assert ctx.lead_pending() == 0 and len(ctx.lead_flush()) == 0
    outs, _, _, _, _ = _run(ctx, clip, (4, 2))
    for t in range(6):
        np.testing.assert_array_equal(outs[t], want[t], err_msg=f"after reset, frame {t}")
    # J == 0, and motion on frames past 32768
    off = nets()
    assert _code(off.process_lead_nv12, clip[:1], match="vd_lead") == S
    mo = nets(lead=J, lead_motion=True, max_batch=6)
    wide = np.zeros((3, 32770), np.uint8)
    assert _raw(mo, desc(wide, 1, 2, 32770), desc(wide, 1, 2, 32770), 1, 2, 32770, HOST, 1, 0) == (AR, -7)
    assert mo.lead_pending() == 0


# ---- 6: lead off ------------------------------------------------------------------------------------------

def test_lead_off_is_untouched(gpu, nets, clip):
    """process_nv12 in a lead=0 context: the same bytes and per-family launch counts before and after
    another context ran process_lead_nv12, and no ring traffic (family 4) at all."""
    import vdmi
    from vdmi import weights
    ctx = vdmi.Context(precision="fp32", max_batch=4, hold=2)
    try:
        ctx.load_weights(0, weights.retinaface_state_dict(0))
        ctx.timing(True)
        res = []
        for again in (False, True):
            if again:
                other = nets(lead=J)
                assert len(other.process_lead_nv12(clip[:3])[0]) == 1 and other.lead_pending() == 2
                other.hold_reset()
            ctx.hold_reset()
            ctx.timing_reset()
            out, faces, _ = ctx.process_nv12(clip[:4])
            ctx.sync()
            res.append((out.copy(), [_lists(faces, b) for b in range(4)], [ctx.timing_read(f)[1] for f in range(7)]))
            assert ctx.lead_pending() == 0 and ctx.lead == 0
    finally:
        ctx.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    assert res[0][1:] == res[1][1:]
    assert res[0][2][4] == 0 and res[0][2][1] > 0
