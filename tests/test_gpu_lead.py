"""Look-ahead hold on the GPU (csrc/lead.hip through vd_lead_lists and vd_process_lead), exact
against the definition in tests/lead_ref.py: lists, labels, the emission arithmetic across
calls, and the pixels of the frames blurred with B_t = D_t ++ H_t ++ A_t."""
import ctypes

import numpy as np
import pytest

import cells_ref as cr
import gaussian_ref as gr
import hold_ref as hr
import lead_ref as lr
import mask_ref as mr
from oracle import mosaic as omosaic
from test_gpu_hold import _device_boxes, _frame, _host_boxes, _lists, _random_sequence, _rows

pytestmark = pytest.mark.gpu

LDS_BOXES = 2048       # csrc/lead.hip: clipped reference boxes (frames t .. t+J-1) the kernel keeps in LDS

_CTX = {}


@pytest.fixture(scope="module")
def lead_ctx(gpu):
    """Weight-less lead contexts by (J, P, motion, K): vd_lead_lists needs no network."""
    import vdmi

    def make(J, P=30, motion=False, K=0):
        key = (J, P, motion, K)
        if key not in _CTX:
            _CTX[key] = vdmi.Context(precision="fp32", max_batch=4, lead=J, lead_motion=motion, hold=K,
                                     hold_iou_pct=P)
        _CTX[key].hold_reset()
        return _CTX[key]

    yield make
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _stream(ctx, seq, h, w, cuts, device=False):
    """seq through ctx.lead_lists in calls ending at `cuts`, then a flush: per frame (B_t, labels)
    through `out`, (A_t, labels) and B_t again through read_lead, and every call's n_out."""
    from vdmi import _lib
    B, L, Al, AL, ms, lo = [], [], [], [], [], 0
    for hi in list(cuts) + [None]:
        part = seq[lo:hi] if hi is not None else []
        room = ctx.lead_pending() + len(part)
        out = _lib.HostBoxes(max(room, 1), 4096)
        boxes = (_device_boxes(part) if device else _host_boxes(part)) if part else None
        _, m = ctx.lead_lists(boxes, h, w, flush=hi is None, out=out)
        ms.append(m)
        if m:
            led, both = ctx.read_lead(m, "lead"), ctx.read_lead(m, "all")
        for i in range(m):
            b, l = _rows(out, i)
            B.append(b)
            L.append(l)
            assert _rows(both, i) == (b, l)
            a, al = _rows(led, i)
            Al.append(a)
            AL.append(al)
        lo = hi
    assert ctx.lead_pending() == 0
    return B, L, Al, AL, ms


A, FAR = (10, 10, 30, 30), (60, 60, 90, 95)
EMPTIES = [(200, 200, 240, 230), (60, 30, 60, 50), (-50, -50, -10, -10)]
CRAFTED = {   # name: (sequence, J, P, motion, expected A per frame) on a 100 x 100 frame (tests/test_lead_ref.py)
    "before_first_detection": ([[], [], [A], [A]], 2, 30, False, [[A], [A], [], []]),
    "age_then_list_order": ([[], [FAR], [A]], 2, 30, False, [[FAR, A], [A], []]),
    "motion": ([[], [], [(40, 40, 60, 60)], [(45, 40, 65, 60)]], 2, 30, True,
               [[(30, 40, 60, 60)], [(35, 40, 60, 60)], [], []]),
    "inclusive_match": ([[(0, 0, 10, 3)], [(0, 0, 10, 10)]], 1, 30, False, [[], []]),
    "just_below": ([[(0, 0, 9, 3)], [(0, 0, 10, 10)]], 1, 30, False, [[(0, 0, 10, 10)], []]),
    "empties_never_led": ([[], EMPTIES], 2, 30, False, [[], []]),
    "empties_never_match": ([EMPTIES, [(50, 20, 70, 60)]], 1, 30, False, [[(50, 20, 70, 60)], []]),
    "led_unclipped": ([[], [(-5, -5, 10, 10)]], 1, 30, False, [[(-5, -5, 10, 10)], []]),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_vd_lead_lists_known_answers(lead_ctx, name):
    seq, J, P, motion, want = CRAFTED[name]
    _, _, Al, AL, _ = _stream(lead_ctx(J, P, motion), seq, 100, 100, (len(seq),))
    assert Al == want
    assert (Al, [[-a for a in l] for l in AL]) == lr.lead_lists(seq, 100, 100, J, P, motion)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("P", [1, 30, 100])
@pytest.mark.parametrize("J", [1, 3, 8])
def test_random_sequences(lead_ctx, J, P, device):
    seq, h, w = _random_sequence(100 * J + P)
    moved = {}
    for motion in (False, True):
        B, L, Al, AL, _ = _stream(lead_ctx(J, P, motion), seq, h, w, (len(seq),), device=device)
        wantB, wantL = lr.blur_lists(seq, h, w, J, P, motion)
        assert B == wantB and L == wantL
        wantA, ages = lr.lead_lists(seq, h, w, J, P, motion)
        assert Al == wantA and AL == [[-a for a in l] for l in ages]
        moved[motion] = Al
    led1 = sum(a.count(1) for a in ages)
    cands1 = sum(1 for d in seq[1:] for b in d if hr.clip_box(b, h, w))
    assert led1 > 0 and cands1 - led1 > 0                    # both outcomes: led, and matched away
    n_moved = sum(1 for x, y in zip(moved[False], moved[True]) for b, c in zip(x, y) if b != c)
    if P == 100:
        assert n_moved == 0                                   # a predecessor equals the box: nothing moves
    else:
        assert n_moved > 0


def test_combined_with_hold(lead_ctx):
    """Hold K = 2 and lead J = 3 in one context: the order D, H, A and the label signs."""
    J, K, P = 3, 2, 30
    seq, h, w = _random_sequence(321)
    for motion in (False, True):
        ctx = lead_ctx(J, P, motion, K)
        if motion:
            ctx.set_hold_motion(True)
        B, L, _, _, _ = _stream(ctx, seq, h, w, (7, 12))
        wantB, wantL = lr.blur_lists(seq, h, w, J, P, motion, K=K, hold_motion=motion)
        assert B == wantB and L == wantL
        if motion:
            ctx.set_hold_motion(False)
    for l in L:
        kinds = [0 if v == 0 else (1 if v > 0 else 2) for v in l]
        assert kinds == sorted(kinds)                            # D, then H, then A
    assert any(v > 0 for l in L for v in l) and any(v < 0 for l in L for v in l)


def test_call_split_invariance(lead_ctx):
    """12 frames as one call + flush, as 5 + 7 and as twelve calls of one frame at J = 3 with
    motion (delay 4: calls smaller than the delay) give identical B_t; n_out follows
    max(0, pending + n - delay)."""
    J, P, delay = 3, 30, 4
    seq, h, w = _random_sequence(7)
    ctx = lead_ctx(J, P, True)
    want = lr.blur_lists(seq, h, w, J, P, True)
    assert any(v < 0 for l in want[1] for v in l)
    for cuts in ((12,), (5, 12), tuple(range(1, 13))):
        ctx.hold_reset()
        B, L, _, _, ms = _stream(ctx, seq, h, w, cuts)
        assert (B, L) == want, cuts
        pend, lo, exp = 0, 0, []
        for hi in cuts:
            exp.append(max(0, pend + (hi - lo) - delay))
            pend += (hi - lo) - exp[-1]
            lo = hi
        assert ms == exp + [pend], cuts


def test_global_memory_path(lead_ctx):
    """600 boxes per frame at J = 8 on 4 frames at 1080x1920: frame 0 compares its age-3
    candidates against 1800 and would stage 2400 clipped boxes, more than LDS_BOXES, so it reads
    them from global memory; frames 1..3 (1800 / 1200 / 600 staged) take the LDS path."""
    J, P = 8, 30
    rng = np.random.default_rng(3)
    seq = []
    for t in range(4):
        xy = rng.integers(0, 1800, (600, 2))
        wh = rng.integers(4, 40, (600, 2))
        seq.append([tuple(int(v) for v in (x, y, x + a, y + b)) for (x, y), (a, b) in zip(xy, wh)])
    assert 3 * 600 <= LDS_BOXES < 4 * 600
    B, L, Al, _, _ = _stream(lead_ctx(J, P), seq, 1080, 1920, (4,), device=True)
    assert (B, L) == lr.blur_lists(seq, 1080, 1920, J, P)
    assert len(Al[0]) > 0 and 3 * 600 - len(Al[0]) > 0


# ---- end to end through vd_process_lead --------------------------------------------------

_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by their keyword arguments."""
    import vdmi
    from vdmi import weights

    def make(**kw):
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        if key not in _NETS:
            c = vdmi.Context(precision="fp32", max_batch=4, **kw)
            c.load_weights(0, weights.retinaface_state_dict(0))
            c.load_weights(1, weights.yolov8n_state_dict(0))
            _NETS[key] = c
        _NETS[key].hold_reset()
        return _NETS[key]

    yield make
    for c in _NETS.values():
        c.close()
    _NETS.clear()


@pytest.fixture(scope="module")
def clip_frames():
    a, b, c = _frame(0), _frame(1), _frame(2)
    return [a, a, b, b, c, a]


def _flags():
    from vdmi import _lib
    return _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES


def _process_lead_sequence(ctx, frames, calls, device=False):
    """frames through ctx.process_lead in `calls` then a flush: the emitted frames in order, the
    D list of every pushed frame, read_lead's B_t of every emitted frame, and each call's m."""
    import torch
    outs, D, B, ms, lo = [], [], [], [], 0
    for n in list(calls) + [0]:
        if n:
            batch = np.stack(frames[lo:lo + n])
            out, faces, plates = ctx.process_lead(torch.from_numpy(batch).cuda() if device else batch, flags=_flags())
            D += [_lists(faces, b) + _lists(plates, b) for b in range(n)]
        else:
            out = ctx.lead_flush()
        m = len(out)
        ms.append(m)
        if m:
            rows = ctx.read_lead(m, "all")
            B += [_rows(rows, i) for i in range(m)]
        out = out.cpu().numpy() if device else out
        outs += [out[i] for i in range(m)]
        lo += n
    return outs, D, B, ms


def _check_pixels(ctx, frames, K, render, device=False):
    J, P = 2, 30
    outs, D, B, ms = _process_lead_sequence(ctx, frames, (4, 2), device)
    assert ms == [2, 2, 2] and len(outs) == len(frames)
    wantB, wantL = lr.blur_lists(D, 360, 640, J, P, K=K)
    assert [b for b, _ in B] == wantB and [l for _, l in B] == wantL
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], render(fr, wantB[t]), err_msg=f"frame {t}")
    assert any(v < 0 for l in wantL for v in l)                 # some A_t is non-empty
    return outs, D, wantB


@pytest.mark.parametrize("device", [False, True], ids=["host_frames", "device_frames"])
@pytest.mark.parametrize("K", [0, 2])
def test_process_lead_pixels(net_ctx, clip_frames, K, device):
    """[A, A, B, B, C, A] as calls of 4 + 2 + flush at J = 2: every emitted frame is the oracle
    mosaic of B_t built by the references over the returned detections, some box is led, and the
    output differs from the lead-off output."""
    outs, D, B = _check_pixels(net_ctx(lead=2, hold=K), clip_frames, K, lambda fr, b: omosaic.mosaic_frame(fr, b, 8),
                               device)
    off = net_ctx(hold=K)
    outs0 = []
    for lo, n in ((0, 4), (4, 2)):
        o, f, p = off.process(np.stack(clip_frames[lo:lo + n]), flags=_flags())
        assert [_lists(f, b) + _lists(p, b) for b in range(n)] == D[lo:lo + n]     # the same detections
        outs0 += list(o)
    assert any(not np.array_equal(x, y) for x, y in zip(outs, outs0))


def test_process_lead_gaussian(net_ctx, clip_frames):
    from vdmi import _lib
    q = _lib.blur_weights(9, 0.0)
    _check_pixels(net_ctx(lead=2, blur="gaussian", blur_ksize=9), clip_frames, 0,
                  lambda fr, b: gr.blur_frame(fr, b, 9, 0.0, q=q))


def test_process_lead_ellipse_mask(net_ctx, clip_frames):
    _check_pixels(net_ctx(lead=2, hold=2, mask="ellipse", mask_grow=42), clip_frames, 2,
                  lambda fr, b: mr.shaped_frame(fr, b, "ellipse", 42, lambda im, bb: omosaic.mosaic_frame(im, bb, 8)))


def test_process_lead_cells(net_ctx, clip_frames):
    _check_pixels(net_ctx(lead=2, cells=4), clip_frames, 0, lambda fr, b: cr.mosaic_frame_cells(fr, b, 8, 4))


def test_process_lead_splits_a_batch_under_tiling(net_ctx, clip_frames):
    """tiles=(1, 2) at max_batch=4 carries one frame per call: process_lead splits [A, B, C] into
    three calls and concatenates what they emit; with the flush every frame is the oracle mosaic
    of B_t over the returned (merged) detections."""
    ctx = net_ctx(lead=1, tiles=(1, 2))
    assert ctx.frames_per_call() == 1
    frames = [clip_frames[0], clip_frames[2], clip_frames[4]]
    out, faces, plates = ctx.process_lead(np.stack(frames), flags=_flags())
    assert len(out) == 2 and ctx.lead_pending() == 1
    outs = list(out) + list(ctx.lead_flush())
    D = [_lists(faces, b) + _lists(plates, b) for b in range(3)]
    B, L = lr.blur_lists(D, 360, 640, 1, 30)
    assert len(outs) == 3 and any(v < 0 for l in L for v in l)
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], omosaic.mosaic_frame(fr, B[t], 8), err_msg=f"frame {t}")


def test_lead_off_is_untouched(gpu, clip_frames):
    """A lead=0 context's process() output and launch counts equal those of a context that never
    heard of lead (Context(lead=0) never calls vd_lead; the second context sets lead 0 explicitly)."""
    import vdmi
    from vdmi import weights
    sd = weights.retinaface_state_dict(0)
    batch = np.stack(clip_frames[:4])
    res = []
    for touch in (False, True):
        ctx = vdmi.Context(precision="fp32", max_batch=4, hold=2)
        try:
            if touch:
                ctx.set_lead(0, False)
            ctx.load_weights(0, sd)
            ctx.timing(True)
            ctx.timing_reset()
            out, faces, _ = ctx.process(batch)
            ctx.sync()
            res.append((out.copy(), [_lists(faces, b) for b in range(4)], [ctx.timing_read(f)[1] for f in range(7)]))
            assert ctx.lead_pending() == 0
        finally:
            ctx.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    assert res[0][1:] == res[1][1:]


def _code(fn, *a, **k):
    from vdmi import _lib
    with pytest.raises(_lib.VdError) as e:
        fn(*a, **k)
    return e.value.code


def test_refusals(gpu, lead_ctx, net_ctx, clip_frames):
    import torch
    import vdmi
    from vdmi import _lib
    S, AR, CAP = _lib.VD_ERR_STATE, _lib.VD_ERR_ARG, _lib.VD_ERR_CAPACITY
    # J == 0 in either lead call, and in the reader
    off = vdmi.Context(precision="fp32", max_batch=2)
    try:
        assert _code(off.lead_lists, [[A]], 100, 100) == S
        assert _code(off.process_lead, np.zeros((1, 64, 64, 3), np.uint8)) == S
        assert _code(off.read_lead, 1) == S
        # bad J, bad motion, motion without J: the raw ABI (check_lead stops them in Python)
        for frames, motion in ((9, 0), (-1, 0), (2, 2), (2, -1), (0, 1)):
            assert off._lib.vd_lead(off._h, frames, motion) == AR
        assert off.lead == 0 and off.lead_pending() == 0
    finally:
        off.close()
    # lists: a host list past its cap, mixing, settings while pending, geometry, motion on huge frames
    ctx = lead_ctx(2, 30, False, 2)
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    assert _code(ctx.lead_lists, hb, 100, 100) == CAP
    assert ctx.lead_pending() == 0                               # a refused call has no effect
    ctx.lead_lists([[A]], 100, 100)
    assert ctx.lead_pending() == 1
    assert _code(ctx.lead_lists, [[A]], 100, 120) == S           # another geometry: flush first
    assert _code(ctx.set_lead, 3, False) == S
    assert _code(ctx.set_hold_motion, True) == S
    assert _code(ctx.set_tiles, (2, 2), 20) == S
    assert _code(ctx.hold, [[A]], 100, 100) == S
    assert _code(ctx.process_lead, np.zeros((1, 100, 100, 3), np.uint8)) == S      # pending from lead_lists
    ctx.set_lead(2, False)                                       # the setting it already has: nothing changes
    ctx.set_hold_motion(False)
    assert ctx.lead_pending() == 1
    out = ctx.lead_lists(None, 100, 100, flush=True)
    assert out.n == 1 and _rows(out, 0) == ([A], [0])
    ctx.lead_lists([[A]], 100, 100)
    ctx.hold_reset()                                             # the explicit abandon
    assert ctx.lead_pending() == 0
    assert ctx.lead_lists(None, 100, 100, flush=True).n == 0
    mo = lead_ctx(2, 30, True)
    assert _code(mo.lead_lists, [[A]], 100, 40000) == AR
    assert mo.lead_pending() == 0
    # pixels: the mosaic flag is required, process() with it is refused, capacity, mixing, geometry
    net = net_ctx(lead=2)
    batch = np.stack(clip_frames[:4])
    assert _code(net.process, batch) == S                        # would silently skip A_t
    assert _code(net.process_lead, batch, flags=_lib.VD_PROC_FACES) == AR
    net.process(batch[:2], flags=_lib.VD_PROC_FACES)             # without the flag: legal while nothing is pending
    out, _, _ = net.process_lead(batch)
    assert len(out) == 2 and net.lead_pending() == 2
    assert _code(net.process, batch[:2], flags=_lib.VD_PROC_FACES) == S            # ... and refused while pending
    assert _code(net.lead_lists, [[A]], 360, 640) == S           # pending from process_lead
    assert _code(net.process_lead, batch[:, :352]) == S          # another geometry
    small = np.empty((1, 360, 640, 3), np.uint8)
    assert _code(net.process_lead, batch[:2], out=small) == CAP  # m = 2 > out_cap = 1
    dev = torch.from_numpy(batch).cuda()
    m = ctypes.c_int(-1)
    rc = net._lib.vd_process_lead(net._h, dev.data_ptr(), 4, 360, 640, 640 * 3, _lib.VD_DEVICE,
                                  _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC, None, None, dev.data_ptr(), 4, 0,
                                  ctypes.byref(m))
    assert rc == AR and m.value == -1                            # out overlaps in
    assert net.lead_pending() == 2                               # every refusal left the state alone
    assert len(net.lead_flush()) == 2 and net.lead_pending() == 0


# ---- pipeline ---------------------------------------------------------------------------------

NP = 10


def _detectors(device_ids, lead, hold=0):
    import vdmi
    from vdmi import weights
    face = vdmi.Retinaface(input_shape=[640, 640, 3], nms_iou=0.4, max_batch=4, device_ids=device_ids,
                           weights=weights.retinaface_state_dict(0), lead=lead, hold=hold)
    plate = vdmi.YOLO(weights="random", max_batch=4, device_ids=device_ids)
    return face, plate


def _empty_inputs(d, names):
    d.mkdir(exist_ok=True)
    for n in names:
        (d / n).write_bytes(b"")


def test_batch_process_images_lead(gpu, tmp_path):
    """batch_process_images(lead=2, batch_size=4) over 10 frames (no JPEG involved: loader and
    saver are the test's): every input file gets exactly one output, equal to the frame the
    direct process_lead stream emits for it; two device shards write the same frames."""
    import os
    from vdmi import _lib
    from vdmi.pipeline import batch_process_images, fused_context
    J = 2
    frames = {f"f{i:03d}.jpg": _frame(i) for i in range(NP)}
    names = sorted(frames)
    _empty_inputs(tmp_path / "in", names)
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES
    direct_det = _detectors([0], J)
    ctx = fused_context(*direct_det, 4)
    ctx.hold_reset()
    direct, led = [], 0
    for lo in (0, 4, 8):
        out, _, _ = ctx.process_lead(np.stack([frames[n] for n in names[lo:lo + 4]]), flags=flags)
        direct += list(out)
        led += int(ctx.read_lead(len(out), "lead").count.sum()) if len(out) else 0
    out = ctx.lead_flush()
    direct += list(out)
    led += int(ctx.read_lead(len(out), "lead").count.sum())
    assert len(direct) == NP and led > 0
    for name, ids, shard in (("one", [0], None), ("two", [0, 0], "devices")):
        saved = {}
        tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / name), *_detectors(ids, J), batch_size=4,
                                   shard=shard, mosaic_plates=True, lead=J,
                                   loader=lambda p: frames[os.path.basename(p)],
                                   saver=lambda img, p, saved=saved: saved.__setitem__(os.path.basename(p), img.copy()))
        assert tot[0] == NP and sorted(saved) == [f"processed_{n}" for n in names], name
        for t, n in enumerate(names):
            np.testing.assert_array_equal(saved[f"processed_{n}"], direct[t], err_msg=f"{name} {n}")


def test_batch_process_images_lead_refusals(gpu, tmp_path):
    from vdmi.pipeline import batch_process_images
    (tmp_path / "in").mkdir()
    face, plate = _detectors([0], 0)
    with pytest.raises(ValueError, match="lead"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, lead=2)
    face, plate = _detectors([0], 2)
    with pytest.raises(ValueError, match="codec"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, lead=2, gpu_codec=True)
    with pytest.raises(ValueError, match="lead"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, lead=9)


def test_dropped_batch_flushes_the_pending_frames(gpu, tmp_path):
    """A batch whose inference fails is dropped; the two frames pending before it are flushed
    (the stream ends there), so every input frame but the dropped batch's is written once, and
    the batch after it starts a new stream."""
    import os
    from vdmi import _lib
    from vdmi.pipeline import batch_process_images, fused_context
    J = 2
    frames = {f"f{i:03d}.jpg": _frame(i) for i in range(NP)}
    names = sorted(frames)
    _empty_inputs(tmp_path / "in", names)
    face, plate = _detectors([0], J)
    ctx = fused_context(face, plate, 4)
    real, calls = ctx.process_lead, []

    def flaky(*a, **k):
        calls.append(1)
        if len(calls) == 2:                              # the second batch: frames 4..7
            raise RuntimeError("inference failure")
        return real(*a, **k)

    ctx.process_lead = flaky
    saved = {}
    try:
        tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, batch_size=4, shard=None,
                                   mosaic_plates=True, lead=J, loader=lambda p: frames[os.path.basename(p)],
                                   saver=lambda img, p: saved.__setitem__(os.path.basename(p), img.copy()))
    finally:
        del ctx.process_lead
    kept = [names[i] for i in (0, 1, 2, 3, 8, 9)]
    assert tot[0] == 6 and sorted(saved) == [f"processed_{n}" for n in kept] and len(calls) == 3
    # the same two streams through the context directly: frames 0..3 then a stream end, frames 8..9 then one
    flags = _lib.VD_PROC_FACES | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC | _lib.VD_PROC_MOSAIC_PLATES
    ctx.hold_reset()
    want = []
    for part in (names[:4], names[8:]):
        out, _, _ = ctx.process_lead(np.stack([frames[n] for n in part]), flags=flags, flush=True)
        want += list(out)
    for n, img in zip(kept, want):
        np.testing.assert_array_equal(saved[f"processed_{n}"], img, err_msg=n)
