"""Look-ahead hold on 8-bit 4:2:0 surfaces in any layout on the GPU (vd_process_lead_yuv420; csrc/nv12.hip's
generalised ring push, csrc/track.cpp's surface branch of the lead step). Nothing new is defined, so
everything is checked against existing definitions: lists and pixels against vd_process_lead_nv12 on the
NV12 frames with the same samples in a twin context, the lists also against tests/lead_ref.py, the pixels
against the plane-wise references (tests/nv12_ref.py, tests/nv12_modes_ref.py) over B_t."""
import ctypes

import numpy as np
import pytest

import lead_ref as lr
import nv12_ref as nr
import yuv420_ref as yr
from test_gpu_hold import _lists, _rows
from test_gpu_lead_nv12 import BOX, H, J, MODES, P, W, _code, _dev, _flags, _np, clip, nets   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# the ring push kernel's bytes of a target row per grid-x step (csrc/nv12.hip: PACK_STEP = 64 lanes x 16 B)
PACK_STEP = 1024


def run(ctx, frames_nv12, calls, pushes, device=False, flags=None):
    """NV12 frames through a stream of look-ahead calls, then lead_flush(). pushes[i] = (method name,
    layout or None for the NV12 entry, extra keyword arguments) of call i, the last one repeated. Every
    emitted surface comes back as NV12 samples. -> (outs, D, B, ms)."""
    outs, D, B, ms, lo, olay = [], [], [], [], 0, None
    flags = _flags() if flags is None else flags
    for i, n in enumerate(list(calls) + [0]):
        if n:
            name, lay, kw = pushes[min(i, len(pushes) - 1)]
            batch = frames_nv12[lo:lo + n] if lay is None else yr.from_nv12(frames_nv12[lo:lo + n], lay)
            if lay is not None:
                kw = dict(kw, layout=lay)
            olay = None if lay is None else kw.get("out_layout") or lay
            out, faces, plates = getattr(ctx, name)(_dev(batch) if device else batch, flags=flags, **kw)
            D += [_lists(faces, b) + (_lists(plates, b) if plates is not None else []) for b in range(n)]
        else:
            out = ctx.lead_flush()
        m = len(out)
        ms.append(m)
        if m:
            rows = ctx.read_lead(m, "all")
            B += [_rows(rows, t) for t in range(m)]
            o = _np(out)
            outs += list(o if olay is None else yr.to_nv12(o, olay))
        lo += n
    assert ctx.lead_pending() == 0
    return outs, D, B, ms


_TWIN = {}


def twin(nets, clip, K, calls, **kw):
    """process_lead_nv12's stream on the NV12 clip in a twin context, once per setting."""
    key = (K, calls, repr(sorted(kw.items())))
    if key not in _TWIN:
        _TWIN[key] = run(nets("twin", lead=J, hold=K, **kw), clip, calls, [("process_lead_nv12", None, {})])
    return _TWIN[key]


def same(got, want):
    outs, D, B, ms = got
    assert D == want[1] and B == want[2] and ms == want[3]
    assert len(outs) == len(want[0])
    for t, (a, b) in enumerate(zip(outs, want[0])):
        np.testing.assert_array_equal(a, b, err_msg=f"frame {t}")


# ---- 1: lists and pixels are the NV12 stream's ---------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("calls", [(4, 2), (3, 3)])
@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("layout", yr.LAYOUTS)
def test_equals_the_nv12_stream(nets, clip, layout, K, calls, device):
    want = twin(nets, clip, K, calls)
    got = run(nets(lead=J, hold=K), clip, calls, [("process_lead_yuv420", layout, {})], device)
    same(got, want)
    assert got[3] == ([2, 2, 2] if calls == (4, 2) else [1, 3, 2])
    wantB, wantL = lr.blur_lists(got[1], H, W, J, P, K=K)
    assert [b for b, _ in got[2]] == wantB and [l for _, l in got[2]] == wantL
    assert any(v < 0 for l in wantL for v in l)                   # some A_t is non-empty


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_i420_in_nv12_out(nets, clip, device):
    want = twin(nets, clip, 0, (3, 3))
    same(run(nets(lead=J, hold=0), clip, (3, 3), [("process_lead_yuv420", "i420", dict(out_layout="nv12"))], device), want)


def test_entries_alternate_within_a_stream(nets, clip):
    """One stream pushed by the NV12 entry and the yuv420 entry in turn: the ring and the pending mode are shared."""
    want = twin(nets, clip, 2, (2, 1, 2, 1))
    pushes = [("process_lead_nv12", None, {}), ("process_lead_yuv420", "yv12", {}),
              ("process_lead_yuv420", "nv21", dict(out_layout="i420")), ("process_lead_nv12", None, {})]
    same(run(nets(lead=J, hold=2), clip, (2, 1, 2, 1), pushes), want)
    pushes = [pushes[1], pushes[0], pushes[3], pushes[2]]         # ... and the flush leaves through the yuv420 entry
    same(run(nets(lead=J, hold=2), clip, (2, 1, 2, 1), pushes, device=True), want)


# ---- 2: the pixels are the plane-wise references over B_t ------------------------------------------------

_WANT = {}


@pytest.mark.parametrize("layout,device", [("i420", False), ("nv21", True)])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_modes(nets, clip, mode, layout, device):
    kw, K, render = MODES[mode]
    outs, D, B, ms = run(nets(lead=J, **kw), clip, (4, 2), [("process_lead_yuv420", layout, {})], device)
    assert ms == [2, 2, 2] and len(outs) == 6
    wantB, wantL = lr.blur_lists(D, H, W, J, P, K=K)
    assert [b for b, _ in B] == wantB and any(v < 0 for l in wantL for v in l)
    key = (mode, repr(wantB))
    if key not in _WANT:                                          # the cases of a mode share the reference
        _WANT[key] = [render(clip[t], wantB[t]) for t in range(6)]
    for t in range(6):
        np.testing.assert_array_equal(outs[t], _WANT[key][t], err_msg=f"frame {t}")
    off, outs0, lo = nets(**kw), [], 0                            # the lead changes some emitted frame
    for n in (4, 2):
        o, f, p = off.process_yuv420(yr.from_nv12(clip[lo:lo + n], layout), flags=_flags(), layout=layout)
        assert [_lists(f, b) + _lists(p, b) for b in range(n)] == D[lo:lo + n]
        outs0 += list(yr.to_nv12(o, layout))
        lo += n
    assert any(not np.array_equal(x, y) for x, y in zip(outs, outs0))


# ---- 4: the cut into calls does not matter ----------------------------------------------------------------

def cut_invariance(ctx, clip, motion, push, run_fn):
    cuts = [(1,) * 6, (6,)] if motion else [(1,) * 6, (3, 2, 1), (6,), (2, 4)]
    delay = J + (1 if motion else 0)
    want = None
    for c in cuts:
        outs, D, B, ms = run_fn(ctx, clip, c, [push], device=c == (6,))
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


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_cut_invariance(nets, clip, motion):
    cut_invariance(nets(lead=J, lead_motion=motion, max_batch=6), clip, motion, ("process_lead_yuv420", "yv12", {}), run)


# ---- 5: the ring push at awkward layouts --------------------------------------------------------------------
# A source form: (chroma step as a layout name, V first, luma pitch, chroma pitch, padded luma rows, bytes
# between surfaces, bytes before the first). Pitches, offsets and strides count samples here (8-bit: bytes).

def forms(h, w, kind):
    c = w // 2
    if kind == "aligned":                                         # packed, everything 16-B aligned
        return [("i420", False, w, c, h, 0, 0), ("nv12", True, w, w, h, 0, 0), ("i420", True, w, c, h, 0, 0),
                ("nv12", False, w, w, h, 0, 0)]
    if kind == "wide":                                            # some rows vectorise after a sample-wise head, some do not
        return [("i420", False, w + 6, c + 7, h, 0, 4), ("nv12", True, w + 14, w + 14, h + 2, 16, 0),
                ("i420", True, w + 1, c + 3, h, 9, 3), ("nv12", False, w + 6, w + 22, h, 4, 1)]
    return [("i420", False, w + 1, c + 2, h, 5, 1),               # odd pitches, base offsets 1 and 3
            ("nv12", True, w + 3, w + 5, h + 2, 7, 3),            # NV21
            ("i420", True, w + 14, c + 15, h + 6, 0, 16),         # YV12
            ("nv12", False, w + 4, w + 4, h + 6, 7, 16),          # NV12 itself: the kernel NV12 callers run
            ("nv12", False, w + 4, w + 20, h, 3, 1),              # U-first pairs at a chroma pitch of their own
            ("i420", False, w + 14, c + 15, h, 16, 0)]


def laid_out(frames_nv12, form, fill, room=None):
    """NV12-sample frames laid out by `form` in a device buffer of `room` surfaces -> (vdmi.Yuv420, buffer, host image)."""
    import vdmi
    lay, vf, pitch, cp, hpad, extra, base = form
    k, rows, w = frames_nv12.shape
    h = rows // 3 * 2
    room = max(room or k, k)
    full = np.concatenate([frames_nv12, np.zeros((room - k, rows, w), np.uint8)]) if room > k else frames_nv12
    host, fd = yr.padded(yr.from_nv12(full, lay), lay, pitch, cp, hpad, vf, extra, fill=fill, base_pad=base)
    if room > k:                                                  # the surfaces past k hold the fill alone
        host[base + k * fd["frame_stride"]:] = fill
    buf = _dev(host)
    y = vdmi.Yuv420(buf[base:], h, w, fd["pitch"], fd["u_offset"], fd["v_offset"], fd["chroma_pitch"], fd["chroma_step"],
                    fd["frame_stride"], n=room)
    return y, buf, host


RING_CASES = [(98, 130, (1, 1, 1, 1, 1), "odd"), (98, 130, (3, 2), "odd"), (96, 128, (1, 1, 1, 1, 1), "aligned"),
              (32, 2 * PACK_STEP + 34, (1, 1, 1, 1), "wide"), (32, 2 * PACK_STEP + 34, (2, 2), "wide")]


def ring_push(ctx, push, flush, f, cuts, kind, laid, render, np_out):
    """Noise surfaces in device layouts that change every call, the output layout differing from the
    input's: each emitted surface is the reference over its B_t -- the input itself where B_t is empty --
    and every pad byte of `out` keeps its pattern."""
    from vdmi import _lib
    k, rows, w = f.shape
    h = rows // 3 * 2
    fs = forms(h, w, kind)
    got = lo = 0
    for i, n in enumerate(list(cuts) + [0]):
        pend = ctx.lead_pending()
        room = pend + n
        oy, obuf, _ = laid(np.zeros((0, rows, w), f.dtype), fs[(i + 2) % len(fs)], 0x5A, room)
        if n:
            iy, ibuf, ihost = laid(f[lo:lo + n], fs[i % len(fs)], 0xA5)
            push(iy, out=oy, flags=_lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC)
            np.testing.assert_array_equal(np_out(ibuf), ihost)
        else:
            flush(out=oy)
        m = room - ctx.lead_pending()
        assert m == (room if n == 0 else max(0, room - J))
        want = f[:0]
        if m:
            rows_ = ctx.read_lead(m, "all")
            want = np.stack([render(f[got + t], _rows(rows_, t)[0]) for t in range(m)])
            for t in range(m):
                if not _rows(rows_, t)[0]:
                    np.testing.assert_array_equal(want[t], f[got + t])
        _, _, exp = laid(want, fs[(i + 2) % len(fs)], 0x5A, room)
        np.testing.assert_array_equal(np_out(obuf), exp, err_msg=f"call {i}")
        got += m
        lo += n
    assert got == k and ctx.lead_pending() == 0


@pytest.mark.parametrize("h,w,cuts,kind", RING_CASES)
def test_ring_push_layouts(nets, h, w, cuts, kind):
    ctx = nets(lead=J)
    f = np.random.default_rng(h + len(cuts)).integers(0, 256, (sum(cuts), h * 3 // 2, w), dtype=np.uint8)
    ring_push(ctx, ctx.process_lead_yuv420, ctx.lead_flush, f, cuts, kind, laid_out, lambda fr, b: nr.mosaic(fr, b, 8, 0),
              lambda t: t.cpu().numpy())


# ---- 6: refusals ----------------------------------------------------------------------------------------------

def raw(ctx, name, ind, outd, n, h, w, where, cap, flush, flags=None):
    from vdmi import _lib
    m = ctypes.c_int(-7)
    hb = _lib.HostBoxes(max(n, 1), 64)
    s = hb.struct()
    rc = getattr(ctx._lib, name)(ctx._h, ctypes.byref(ind) if ind is not None else None,
                                 ctypes.byref(outd) if outd is not None else None, n, h, w, where,
                                 _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC if flags is None else flags,
                                 ctypes.byref(s), None, cap, 1 if flush else 0, ctypes.byref(m))
    return rc, m.value


def refusals(nets, name, push, desc, frames, other_push, other_frames, extra=None):
    """Every refusal of entry `name`, with 0 and with 2 surfaces pending. desc(ptr, h, w, **changes) -> its
    descriptor of packed I420 surfaces; frames: its packed I420 clip; other_push / other_frames: the other
    bit depth's method and clip. extra(refuse, pend): the family's own refusals."""
    import vdmi
    from vdmi import _lib
    S, AR, CAP = _lib.VD_ERR_STATE, _lib.VD_ERR_ARG, _lib.VD_ERR_CAPACITY
    HOST, DEV = _lib.VD_HOST, _lib.VD_DEVICE
    ctx = nets(lead=J, blur="gaussian", cells=8)
    method = getattr(ctx, push)
    ibuf, obuf = np.ascontiguousarray(frames[:4]), np.zeros_like(frames[:4])
    ok_in, ok_out = desc(ibuf.ctypes.data, H, W), desc(obuf.ctypes.data, H, W)
    es = ibuf.itemsize

    def refuse(code, field, *a, **k):
        assert raw(ctx, name, *a, **k) == (code, -7), _lib.last_error()
        assert field in _lib.last_error(), _lib.last_error()

    def refused(pend):
        refuse(AR, "pitch <", desc(ibuf.ctypes.data, H, W, pitch=(W - 2) * es), ok_out, 1, H, W, HOST, 4, 0)
        refuse(AR, "chroma_step outside", desc(ibuf.ctypes.data, H, W, chroma_step=3), ok_out, 1, H, W, HOST, 4, 0)
        refuse(AR, "v_offset:", desc(ibuf.ctypes.data, H, W, v_offset=H * W * es), ok_out, 1, H, W, HOST, 4, 0)
        refuse(AR, "positive h and w", ok_in, ok_out, 1, H - 1, W, HOST, 4, 0)                                  # odd h
        refuse(AR, "positive h and w", ok_in, ok_out, 1, H, W - 1, HOST, 4, 0)                                  # odd w
        refuse(AR, "null", None, ok_out, 1, H, W, HOST, 4, 0)                                          # no descriptor
        refuse(AR, "where", ok_in, ok_out, 1, H, W, 7, 4, 0)
        refuse(AR, "MOSAIC", ok_in, ok_out, 1, H, W, HOST, 4, 0, flags=_lib.VD_PROC_FACES)
        refuse(AR, "nothing to blur", ok_in, ok_out, 1, H, W, HOST, 4, 0, flags=_lib.VD_PROC_MOSAIC | _lib.VD_PROC_PLATES)
        refuse(AR, "flush", None, None, 0, H, W, HOST, 0, 0)                                           # n == 0 without flush
        refuse(CAP, "to emit", ok_in, ok_out, 4, H, W, HOST, pend + 1, 0)                              # m = pend + 2
        refuse(AR, "output descriptor", ok_in, None, 4, H, W, HOST, 4, 0)                              # m > 0, out NULL
        refuse(AR, "pitch <", ok_in, desc(obuf.ctypes.data, H, W, pitch=(W - 2) * es), 4, H, W, HOST, 4, 0)
        d = _dev(np.concatenate([frames[:4], frames[:4]]).view(np.uint8).reshape(8, -1))
        fb = H * W * 3 // 2 * es
        refuse(AR, "overlap", desc(d.data_ptr(), H, W), desc(d.data_ptr() + 3 * fb, H, W), 4, H, W, DEV, 4, 0)
        ctx.set_cells(0)                                                                               # the fixed Gaussian
        assert _code(method, frames[:1], match="cells") == S
        ctx.set_cells(8)
        if extra:
            extra(ctx, refuse, pend, ok_in, ok_out, ibuf, obuf)
        assert ctx.lead_pending() == pend

    refused(0)
    ctx.set_tiles((2, 2), 20)                                     # a change of tiling is itself refused while frames are pending
    try:
        assert _code(method, frames[:1], match="tile") == S
    finally:
        ctx.set_tiles((1, 1), 20)
    assert ctx.lead_pending() == 0
    assert raw(ctx, name, None, None, 0, H, W, HOST, 0, 1) == (_lib.VD_OK, 0)                          # an empty stream ends
    want = list(method(frames[:4], flags=_flags())[0])
    assert len(want) == 2 and ctx.lead_pending() == 2
    refused(2)
    assert _code(method, frames[:1, :H * 3 // 2 - 12], match="pending") == S                           # 352 x 640
    assert _code(method, frames[:1, :, :W - 8], match="pending") == S                                  # 360 x 632
    rgb = np.zeros((1, H, W, 3), np.uint8)
    assert _code(ctx.process_lead, rgb, match=name) == S                                               # names the pusher
    assert _code(ctx.lead_lists, [[BOX]], H, W, match=name) == S
    assert _code(getattr(ctx, other_push), other_frames[:1], match=name) == S                          # 8-bit against 16-bit
    assert _code(ctx.process, rgb, flags=_lib.VD_PROC_FACES) == S
    assert _code(ctx.set_lead, 3, False) == S
    assert ctx.lead_pending() == 2
    want += list(method(frames[4:], flags=_flags())[0]) + list(ctx.lead_flush())
    assert len(want) == 6 and ctx.lead_pending() == 0
    # RGB frames pending, then lists: this entry is refused, pushing or flushing
    ctx.process_lead(rgb, flags=_flags())
    assert _code(method, frames[:1], match="vd_process_lead \\(flush first\\)") == S
    assert raw(ctx, name, None, ok_out, 0, H, W, HOST, 4, 1) == (S, -7) and ctx.lead_pending() == 1
    assert len(ctx.lead_flush()) == 1
    ctx.lead_lists([[BOX]], H, W)
    assert _code(method, frames[:1], match="vd_lead_lists") == S and ctx.lead_pending() == 1
    ctx.lead_lists(None, H, W, flush=True)
    # hold_reset abandons pending surfaces; the next stream starts clean
    method(frames[:2], flags=_flags())
    assert ctx.lead_pending() == 2
    ctx.hold_reset()
    assert ctx.lead_pending() == 0 and len(ctx.lead_flush()) == 0
    outs = list(method(frames[:4], flags=_flags())[0]) + list(method(frames[4:], flags=_flags())[0]) + list(ctx.lead_flush())
    for t in range(6):
        np.testing.assert_array_equal(_np(outs[t]), _np(want[t]), err_msg=f"after reset, frame {t}")
    # J == 0, and motion on frames past 32768
    assert _code(getattr(nets(), push), frames[:1], match="vd_lead") == S
    mo = nets(lead=J, lead_motion=True, max_batch=6)
    wide = np.zeros((3, 32770), ibuf.dtype)
    refuse_mo = raw(mo, name, desc(wide.ctypes.data, 2, 32770), desc(wide.ctypes.data, 2, 32770), 1, 2, 32770, HOST, 1, 0)
    assert refuse_mo == (AR, -7) and "motion" in _lib.last_error() and mo.lead_pending() == 0


def desc8(ptr, h, w, **changes):
    from vdmi import _lib
    f = dict(pitch=w, u_offset=h * w, v_offset=h * w + h * w // 4, chroma_pitch=w // 2, frame_stride=h * w * 3 // 2,
             chroma_step=1)
    f.update(changes)
    return _lib.vd_yuv420(ptr, f["pitch"], f["u_offset"], f["v_offset"], f["chroma_pitch"], f["frame_stride"],
                          f["chroma_step"], 1, 0)


def test_refusals(nets, clip):
    import yuv420_16_ref as y16
    i420 = yr.from_nv12(clip, "i420")
    refusals(nets, "vd_process_lead_yuv420", "process_lead_yuv420", desc8, i420, "process_lead_yuv420_16",
             y16.widen(i420, 10, 0, 1))


def test_nv12_entry_refuses_pending_words(nets, clip):
    """Surfaces of 16-bit words pending: the NV12 entry is refused as the yuv420 entry is."""
    import yuv420_16_ref as y16
    from vdmi import _lib
    ctx = nets(lead=J)
    ctx.process_lead_yuv420_16(y16.widen(yr.from_nv12(clip[:2], "i420"), 10, 0, 1), flags=_flags())
    assert ctx.lead_pending() == 2
    assert _code(ctx.process_lead_nv12, clip[:1], match="vd_process_lead_yuv420_16") == _lib.VD_ERR_STATE
    assert ctx.lead_pending() == 2
    ctx.hold_reset()


# ---- 7: lead off ------------------------------------------------------------------------------------------------

def test_lead_off_is_untouched(gpu, nets, clip):
    """process_yuv420 / process_yuv420_16 in a lead=0 context: the same bytes and per-family launch counts
    before and after another context ran the new entries, and no ring traffic (family 4) at all."""
    import vdmi
    import yuv420_16_ref as y16
    from vdmi import weights
    i420 = yr.from_nv12(clip, "i420")
    p010 = y16.widen(clip, 10, 6, 3)
    ctx = vdmi.Context(precision="fp32", max_batch=4, hold=2)
    try:
        ctx.load_weights(0, weights.retinaface_state_dict(0))
        ctx.timing(True)
        res = []
        for again in (False, True):
            if again:
                other = nets(lead=J)
                assert len(other.process_lead_yuv420(i420[:3])[0]) == 1 and other.lead_pending() == 2
                other.hold_reset()
                assert len(other.process_lead_yuv420_16(p010[:3], layout="nv12")[0]) == 1 and other.lead_pending() == 2
                other.hold_reset()
            for call, frames, kw in ((ctx.process_yuv420, i420, {}), (ctx.process_yuv420_16, p010, dict(layout="nv12"))):
                ctx.hold_reset()
                ctx.timing_reset()
                out, faces, _ = call(frames[:4], **kw)
                ctx.sync()
                res.append((out.copy(), [_lists(faces, b) for b in range(4)], [ctx.timing_read(f)[1] for f in range(7)]))
                assert ctx.lead_pending() == 0 and ctx.lead == 0
    finally:
        ctx.close()
    for a, b in ((res[0], res[2]), (res[1], res[3])):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1:] == b[1:]
        assert a[2][4] == 0 and a[2][1] > 0
