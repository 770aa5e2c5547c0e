"""Look-ahead hold on 10- and 12-bit 4:2:0 surfaces on the GPU (vd_process_lead_yuv420_16: the ring of
16-bit words, its pending mode, depth and shift as pending geometry). Lists are checked against the 8-bit
entry on D(frames), pixels against tests/yuv420_16_ref.py over B_t: pixelation by the lo / hi definition,
the smooth blur and the ellipse restore on values, and every word no box owns bit for bit."""
import numpy as np
import pytest

import lead_ref as lr
import yuv420_16_ref as y16
import yuv420_ref as yr
from test_gpu_hold import _lists, _rows
from test_gpu_lead_nv12 import H, J, P, W, _code, _flags, clip, nets   # noqa: F401 (fixtures)
from test_gpu_lead_yuv420 import PACK_STEP, RING_CASES, cut_invariance, forms, refusals, ring_push
from test_gpu_lead_yuv420 import run as run8

pytestmark = pytest.mark.gpu

# depth, shift, layout in, layout out (None: the input's)
CASES = {"p010": (10, 6, "nv12", None), "yuv420p10le": (10, 0, "i420", None), "p012_vu": (12, 4, "nv21", None),
         "p010_to_planar": (10, 6, "nv12", "i420")}


def _dev16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def _np16(x):
    return x.cpu().numpy().view(np.uint16) if hasattr(x, "cpu") else np.asarray(x).view(np.uint16)


def quiet(n):
    """n flat NV12 frames of H x W: no face fires on them (the seeded plate net does), so under the
    face flags the first has an empty blur list."""
    return np.full((n, H * 3 // 2, W), 128, np.uint8)


def face_flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC


def run16(ctx, words_nv12, calls, pushes, device=False, flags=None):
    """test_gpu_lead_yuv420.run for NV12-layout uint16 frames through process_lead_yuv420_16: pushes[i] =
    (layout, keyword arguments). Every emitted surface comes back in NV12 layout."""
    outs, D, B, ms, lo, olay = [], [], [], [], 0, None
    flags = _flags() if flags is None else flags
    for i, n in enumerate(list(calls) + [0]):
        if n:
            lay, kw = pushes[min(i, len(pushes) - 1)]
            batch = y16.relayout(words_nv12[lo:lo + n], "nv12", lay)
            olay = kw.get("out_layout") or lay
            out, faces, plates = ctx.process_lead_yuv420_16(_dev16(batch) if device else batch, flags=flags, layout=lay, **kw)
            D += [_lists(faces, b) + (_lists(plates, b) if plates is not None else []) for b in range(n)]
        else:
            out = ctx.lead_flush()
        m = len(out)
        ms.append(m)
        if m:
            rows = ctx.read_lead(m, "all")
            B += [_rows(rows, t) for t in range(m)]
            outs += list(y16.relayout(_np16(out), olay, "nv12"))
        lo += n
    assert ctx.lead_pending() == 0
    return outs, D, B, ms


# ---- 3: lists are the 8-bit entry's on D, pixels the references over B_t -------------------------------------

RENDER = {
    "pixelate": (dict(), 0, lambda fr, b, d, s: y16.mosaic([fr], [b], 8, 0)[0]),
    "cells": (dict(cells=4), 0, lambda fr, b, d, s: y16.mosaic([fr], [b], 8, 4)[0]),
    "smooth_ellipse": (dict(blur="gaussian", cells=8, mask="ellipse", mask_grow=42, hold=2), 2,
                       lambda fr, b, d, s: y16.shaped(fr, b, "ellipse", 42, lambda f, bb: y16.smooth(f, bb, 8, 8, d, s))),
}
_EIGHT = {}
CALLS = (3, 4, 2)


# every mode in every format; the change of layout between in and out once
PIXEL_CASES = [(c, m) for c in sorted(CASES) for m in sorted(RENDER) if CASES[c][3] is None or m == "pixelate"]


@pytest.mark.parametrize("case,mode", PIXEL_CASES)
def test_lists_and_pixels(nets, clip, case, mode):
    depth, shift, lay, olay = CASES[case]
    kw, K, render = RENDER[mode]
    frames8 = np.concatenate([quiet(3), clip])
    words = y16.widen(frames8, depth, shift, seed=depth + shift)                   # noise in the low and the unused bits
    np.testing.assert_array_equal(y16.D(words, depth, shift), frames8)
    device = case in ("p010", "p010_to_planar")
    outs, D, B, ms = run16(nets(lead=J, **kw), words, CALLS, [(lay, dict(shift=shift, depth=depth, out_layout=olay))], device,
                              face_flags())
    assert ms == [1, 4, 2, 2] and len(outs) == 9
    key = (mode, lay)
    if key not in _EIGHT:                                         # the 8-bit entry on D(frames), in the same layout
        _EIGHT[key] = run8(nets("eight", lead=J, **kw), frames8, CALLS, [("process_lead_yuv420", lay, {})], flags=face_flags())
    assert D == _EIGHT[key][1] and B == _EIGHT[key][2] and ms == _EIGHT[key][3]
    wantB, wantL = lr.blur_lists(D, H, W, J, P, K=K)
    assert [b for b, _ in B] == wantB and any(v < 0 for l in wantL for v in l)
    empty = [t for t in range(9) if not wantB[t]]
    assert empty and len(empty) < 9                               # some surface is untouched, some are blurred
    for t in range(9):
        want = words[t] if t in empty else render(words[t], wantB[t], depth, shift)
        np.testing.assert_array_equal(outs[t], want, err_msg=f"frame {t}")         # empty B_t: word for word, unused bits included
    assert any(not np.array_equal(outs[t], words[t]) for t in range(9))


# ---- 4: the cut into calls does not matter ------------------------------------------------------------------

@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_cut_invariance(nets, clip, motion):
    words = y16.widen(clip, 10, 6, seed=4)
    run_fn = lambda ctx, fr, c, pushes, device: run16(ctx, words, c, pushes, device)
    cut_invariance(nets(lead=J, lead_motion=motion, max_batch=6), clip, motion, ("nv12", dict(depth=10, shift=6)), run_fn)


# ---- 5: the ring push at awkward layouts ----------------------------------------------------------------------

def laid_out16(depth, shift):
    def laid(frames_nv12, form, fill, room=None):
        """test_gpu_lead_yuv420.laid_out for words: the form's sizes count words."""
        import vdmi
        lay, vf, pitch, cp, hpad, extra, base = form
        k, rows, w = frames_nv12.shape
        h = rows // 3 * 2
        room = max(room or k, k)
        full = np.concatenate([frames_nv12, np.zeros((room - k, rows, w), np.uint16)]) if room > k else frames_nv12
        host, fd = y16.padded(y16.relayout(full, "nv12", lay), lay, pitch, cp, hpad, vf, extra, fill=fill * 0x101,
                              base_pad_w=base)
        if room > k:
            host[base + k * (fd["frame_stride"] // 2):] = fill * 0x101
        buf = _dev16(host)
        y = vdmi.Yuv420_16(buf[base:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"],
                           fd["chroma_step"], fd["frame_stride"], depth=depth, shift=shift, n=room)
        return y, buf, host
    return laid


# w in words: a chroma ring row of 2 * w bytes spans the same grid-x steps as the 8-bit cases'
RING_CASES_16 = [(h, w if kind != "wide" else PACK_STEP + 18, cuts, kind) for h, w, cuts, kind in RING_CASES]


@pytest.mark.parametrize("h,w,cuts,kind", RING_CASES_16)
def test_ring_push_layouts(nets, h, w, cuts, kind):
    depth, shift = (12, 4) if kind == "aligned" else (10, 6 if len(cuts) > 2 else 0)
    ctx = nets(lead=J)
    f = y16.noise(sum(cuts), h, w, depth, shift, seed=h + len(cuts))
    ring_push(ctx, ctx.process_lead_yuv420_16, ctx.lead_flush, f, cuts, kind, laid_out16(depth, shift),
              lambda fr, b: y16.mosaic([fr], [b], 8, 0)[0], _np16)


# ---- 6: refusals ------------------------------------------------------------------------------------------------

def desc16(ptr, h, w, depth=10, shift=0, **changes):
    from vdmi import _lib
    f = dict(pitch=2 * w, u_offset=2 * h * w, v_offset=2 * h * w + h * w // 2, chroma_pitch=w, frame_stride=3 * h * w,
             chroma_step=1)
    f.update(changes)
    return _lib.vd_yuv420_16(ptr, f["pitch"], f["u_offset"], f["v_offset"], f["chroma_pitch"], f["frame_stride"],
                             f["chroma_step"], 1, 0, depth, shift)


def test_refusals(nets, clip):
    from vdmi import _lib
    S, AR, HOST = _lib.VD_ERR_STATE, _lib.VD_ERR_ARG, _lib.VD_HOST
    i420 = yr.from_nv12(clip, "i420")

    def extra(ctx, refuse, pend, ok_in, ok_out, ibuf, obuf):
        """depth and shift: bad values, out differing from in, and (pending) a push or a flush in another format."""
        ip, op = ibuf.ctypes.data, obuf.ctypes.data
        refuse(AR, "depth outside", desc16(ip, H, W, depth=11), ok_out, 1, H, W, HOST, 4, 0)
        refuse(AR, "shift outside", desc16(ip, H, W, shift=7), ok_out, 1, H, W, HOST, 4, 0)
        refuse(AR, "no depth conversion", ok_in, desc16(op, H, W, depth=12), 4, H, W, HOST, 4, 0)
        refuse(AR, "no depth conversion", ok_in, desc16(op, H, W, shift=2), 4, H, W, HOST, 4, 0)
        if pend:
            refuse(S, "flush first", desc16(ip, H, W, depth=12), desc16(op, H, W, depth=12), 1, H, W, HOST, 4, 0)
            refuse(S, "flush first", desc16(ip, H, W, shift=3), desc16(op, H, W, shift=3), 1, H, W, HOST, 4, 0)
            refuse(S, "flush first", None, desc16(op, H, W, shift=3), 0, H, W, HOST, 4, 1)     # a flush takes them from out

    refusals(nets, "vd_process_lead_yuv420_16", "process_lead_yuv420_16", desc16, y16.widen(i420, 10, 0, 1),
             "process_lead_yuv420", i420, extra)
