"""Weak-detection rescue on the GPU (csrc/rescue.hip and the low threshold of csrc/post.hip, through
vd_rescue_lists, vdt_postprocess, vd_process, vd_process_lead and the pipeline), exact against the
definition in tests/rescue_ref.py: E_t, since, the history across calls, the strong / weak split of
the keep lists, and the pixels of the frames blurred with B_t = E_t ++ H_t ++ A_t."""
import os

import numpy as np
import pytest

import gaussian_ref as gr
import hold_ref as hr
import lead_ref as lr
import rescue_ref as rr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu

LDS_BOXES = 2048       # csrc/vd_common.h VD_RESCUE_LDS_BOXES: clipped reference boxes a workgroup keeps in LDS
RESCUE_STEPS = 1       # include/vdmi.h at vd_rescue: one more timed step of family 3 per call
SETTINGS = [(1, 1, 30), (3, 5, 30), (8, 4, 1), (1, 255, 100)]   # (W, S, P)

_CTX = {}


@pytest.fixture(scope="module")
def list_ctx(gpu):
    """Weight-less rescue contexts by (W, S, P): vd_rescue_lists needs no network."""
    import vdmi

    def make(W, S, P=30):
        if (W, S, P) not in _CTX:
            _CTX[(W, S, P)] = vdmi.Context(precision="fp32", max_batch=4, hold=W, hold_iou_pct=P, rescue=0.2,
                                           rescue_span=S)
        _CTX[(W, S, P)].hold_reset()
        return _CTX[(W, S, P)]

    yield make
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _host_boxes(seq, cap=None):
    from vdmi import _lib
    hb = _lib.HostBoxes(len(seq), cap or max(1, max(len(d) for d in seq)))
    for i, d in enumerate(seq):
        hb.count[i] = len(d)
        if len(d):
            hb.xyxy[i, :len(d)] = np.asarray(d, np.int32).reshape(-1, 4)
    return hb


def _device_boxes(seq):
    import torch
    from vdmi.context import DeviceBoxes
    hb = _host_boxes(seq)
    db = DeviceBoxes(hb.n, hb.cap, "cuda:0")
    db.count.copy_(torch.from_numpy(hb.count))
    db.xyxy.copy_(torch.from_numpy(hb.xyxy))
    torch.cuda.synchronize()
    return db


def _rows(boxes, i):
    k = int(boxes.count[i])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[i, :k]], [int(v) for v in boxes.label[i, :k]]


def _step(ctx, strong, weak, h, w, W, S, P, history, device=False):
    """One vd_rescue_lists call, checked against the reference continued from `history`: E_t with
    label = since. Returns the reference."""
    ref = rr.rescue_lists(strong, weak, h, w, W, S, P, history)
    mk = _device_boxes if device else _host_boxes
    out = ctx.rescue_lists(mk(strong), mk(weak), h, w)
    for i in range(len(strong)):
        got, lab = _rows(out, i)
        assert got == ref[0][i], (i, got, ref[0][i])
        assert lab == ref[1][i], (i, lab, ref[1][i])
    return ref


@pytest.mark.parametrize("name", sorted(rr.CRAFTED))
def test_rescue_lists_known_answers(list_ctx, name):
    strong, weak, W, S, P, want_r, want_s = rr.CRAFTED[name]
    _, since, R, _, _ = _step(list_ctx(W, S, P), strong, weak, 100, 100, W, S, P, None)
    assert R == want_r
    assert [s[len(d):] for s, d in zip(since, strong)] == want_s


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("W,S,P", SETTINGS)
def test_random_sequences(list_ctx, W, S, P, device):
    strong, weak, h, w = rr.random_sequence(10 * W + S)
    _, since, R, _, _ = _step(list_ctx(W, S, P), strong, weak, h, w, W, S, P, None, device=device)
    assert sum(len(r) for r in R) > 0                                        # both outcomes
    assert sum(len(k) for k in weak) - sum(len(r) for r in R) > 0
    assert S < 2 or any(s >= 2 for row in since for s in row)                 # chains (S = 1 allows none)
    assert any(hr.clip_box(b, h, w) is None for k in weak for b in k)


def test_frames_without_weak_or_without_strong_boxes(list_ctx):
    W, S, P = 3, 5, 30
    strong, weak, h, w = rr.random_sequence(4)
    weak[2], weak[7] = [], []
    strong[3], strong[4], strong[8] = [], [], []
    _, _, R, _, _ = _step(list_ctx(W, S, P), strong, weak, h, w, W, S, P, None)
    assert len(R[3]) > 0 and len(R[4]) > 0 and R[2] == []


def test_call_split_invariance_reset_and_size_change(list_ctx):
    """12 frames as one call, as 5 + 7 and as twelve calls of one frame (W = 3: the history shifts
    with n < W) give the same E_t and since; hold_reset and another frame size clear the history."""
    W, S, P = 3, 5, 30
    strong, weak, h, w = rr.random_sequence(7)
    ctx = list_ctx(W, S, P)
    one = _step(ctx, strong, weak, h, w, W, S, P, None)
    for cuts in ((5, 12), tuple(range(1, 13))):
        ctx.hold_reset()
        hist, E, lo = None, [], 0
        for hi in cuts:
            ref = _step(ctx, strong[lo:hi], weak[lo:hi], h, w, W, S, P, hist, device=hi % 2 == 0)
            E += list(zip(ref[0], ref[1]))
            hist = ref[4]
            lo = hi
        assert E == list(zip(one[0], one[1])), cuts
    # the history is still the sequence's tail: after a reset the same weak boxes find nothing
    assert len(rr.rescue_lists([[]], weak[5:6], h, w, W, S, P, one[4])[2][0]) > 0
    ctx.hold_reset()
    assert _step(ctx, [[]], weak[5:6], h, w, W, S, P, None)[2] == [[]]
    ref = _step(ctx, strong[:6], weak[:6], h, w, W, S, P, None)
    # another (h, w): the old history is gone, without a reset ... and back: cleared again
    assert _step(ctx, [[]], weak[5:6], h + 8, w, W, S, P, None)[2] == [[]]
    assert _step(ctx, [[]], weak[5:6], h, w, W, S, P, None)[2] == [[]]
    assert sum(len(r) for r in ref[2]) > 0


def test_global_memory_path_and_cap_overflow(list_ctx):
    """550 strong and 60 weak boxes per frame at W = 8. Call 1, 4 frames: frame 3 compares against
    3 x 550 strong boxes, staged in LDS. Call 2: its frame compares against the history's four E
    rows, more than LDS_BOXES boxes, read from global memory. Then a caller cap below |E_t|."""
    from vdmi import _lib
    W, S, P = 8, 4, 30
    rng = np.random.default_rng(3)
    strong, weak = [], []
    for t in range(5):
        xy = rng.integers(0, 1800, (550, 2))
        wh = rng.integers(4, 40, (550, 2))
        strong.append([tuple(int(v) for v in (x, y, x + a, y + b)) for (x, y), (a, b) in zip(xy, wh)])
        src = strong[t - 1] if t else strong[0]
        weak.append([tuple(int(v) for v in np.asarray(src[i]) + rng.integers(-2, 3, 4)) for i in range(0, 540, 9)])
    ctx = list_ctx(W, S, P)
    ref = _step(ctx, strong[:4], weak[:4], 1080, 1920, W, S, P, None, device=True)
    assert 3 * 550 <= LDS_BOXES < sum(len(e) for e in ref[0])
    assert all(len(r) > 0 for r in ref[2][1:])
    nxt = _step(ctx, strong[4:], weak[4:], 1080, 1920, W, S, P, ref[4], device=True)
    assert 0 < len(nxt[2][0]) < 60
    # a caller cap smaller than E_t: the count is complete, the arrays hold the first cap entries
    ctx.hold_reset()
    _step(ctx, strong[:1], weak[:1], 1080, 1920, W, S, P, None)
    E, since, _, _, _ = rr.rescue_lists(strong[1:2], weak[1:2], 1080, 1920, W, S, P, [(strong[0], [0] * 550)])
    cap = 555
    assert len(E[0]) > cap
    out = _lib.HostBoxes(1, cap)
    ctx.rescue_lists(_host_boxes(strong[1:2]), _host_boxes(weak[1:2]), 1080, 1920, out=out)
    assert int(out.count[0]) == len(E[0])
    assert [tuple(int(v) for v in r) for r in out.xyxy[0]] == E[0][:cap]
    assert [int(v) for v in out.label[0]] == since[0][:cap]


def test_phase2_global_memory_path(list_ctx):
    """Phase 2 (the walk against the rescued boxes) past LDS_BOXES: 1100 weak boxes per frame that all
    chain back to frame 0, so frame 3 sees 2 x 1100 > LDS_BOXES rescued boxes of frames 1 and 2."""
    W, S, P = 2, 200, 30
    rng = np.random.default_rng(5)
    xy = np.stack([rng.integers(0, 1800, 1100), rng.integers(0, 1000, 1100)], 1)
    base = [tuple(int(v) for v in (x, y, x + 20, y + 20)) for x, y in xy]
    strong = [base, [], [], []]
    weak = [[]] + [[(x1 + t, y1, x2 + t, y2) for x1, y1, x2, y2 in base] for t in (1, 2, 3)]
    ref = _step(list_ctx(W, S, P), strong, weak, 1080, 1920, W, S, P, None, device=True)
    assert len(ref[2][1]) + len(ref[2][2]) > LDS_BOXES and len(ref[2][3]) == 1100
    assert set(ref[1][3]) == {3}


def test_refusals(gpu, list_ctx):
    import vdmi
    from vdmi import _lib
    lib = _lib.load()
    off = vdmi.Context(precision="fp32", max_batch=2)
    try:
        with pytest.raises(_lib.VdError) as e:
            off.rescue_lists([[rr.A]], [[rr.A]], 100, 100)
        assert e.value.code == _lib.VD_ERR_STATE
        with pytest.raises(_lib.VdError) as e:
            off.read_rescue(0, 1)
        assert e.value.code == _lib.VD_ERR_STATE
        for lo, plo, span in ((float("nan"), 0.0, 60), (-0.1, 0.0, 60), (0.5, 0.0, 60), (0.7, 0.0, 60),
                              (0.0, float("nan"), 60), (0.0, -1.0, 60), (0.0, 0.5, 60), (0.2, 0.0, 0),
                              (0.2, 0.0, 256), (0.2, 0.0, -1)):
            assert lib.vd_rescue(off.handle, lo, plo, span) == _lib.VD_ERR_ARG, (lo, plo, span)
        assert off.rescue_low == 0.0
        off.set_tiles((2, 2))
        with pytest.raises(_lib.VdError) as e:
            off.rescue(0.2)
        assert e.value.code == _lib.VD_ERR_STATE
        off.set_tiles((1, 1))
        off.rescue(0.2, 0.25, 7)
        assert (off.rescue_low, off.plate_rescue_low, off.rescue_span) == (0.2, 0.25, 7)
        with pytest.raises(_lib.VdError) as e:
            off.set_tiles((2, 2))
        assert e.value.code == _lib.VD_ERR_STATE
        # a change while lead frames are pending
        off.set_lead(2)
        off.lead_lists([[rr.A]], 100, 100)
        assert off.lead_pending() == 1
        with pytest.raises(_lib.VdError) as e:
            off.rescue(0.3)
        assert e.value.code == _lib.VD_ERR_STATE
        off.rescue(0.2, 0.25, 7)                 # the value it has: nothing changes
        assert off.lead_pending() == 1
        off.hold_reset()
        off.rescue(0.0)
        with pytest.raises(_lib.VdError):
            off.rescue_lists([[rr.A]], [[rr.A]], 100, 100)
    finally:
        off.close()
    with pytest.raises(ValueError):
        vdmi.Context(precision="fp32", max_batch=2, rescue=0.2, rescue_span=0)
    with pytest.raises(ValueError):
        vdmi.Context(precision="fp32", max_batch=2, rescue=-0.5)
    ctx = list_ctx(2, 5)
    hb = _lib.HostBoxes(1, 2)
    hb.count[0] = 3
    for s, k in ((hb, _host_boxes([[rr.A]])), (_host_boxes([[rr.A]]), hb)):
        with pytest.raises(_lib.VdCapacityError) as e:
            ctx.rescue_lists(s, k, 100, 100)
        assert e.value.code == _lib.VD_ERR_CAPACITY
    # a change of setting forgets the history; the same setting keeps it
    _step(ctx, [[rr.A]], [[]], 100, 100, 2, 5, 30, None)
    ctx.rescue(0.2, 0.0, 5)
    assert _rows(ctx.rescue_lists([[]], [[rr.A2]], 100, 100), 0) == ([rr.A2], [1])
    ctx.rescue(0.2, 0.0, 6)
    assert _rows(ctx.rescue_lists([[]], [[rr.A2]], 100, 100), 0) == ([], [])
    ctx.rescue(0.2, 0.0, 5)


# ---- the strong / weak split of the keep list on crafted heads ---------------------------------

def test_split_exact_on_crafted_heads(gpu):
    """Logits (0, 0) give a score of exactly 0.5: strong at confidence=0.5 (inclusive), weak at
    confidence=0.6 with rescue=0.5 (inclusive at the low threshold too), nothing at rescue=0.55."""
    import vdmi
    from conftest import face_weights
    A = 16800
    loc = np.zeros((1, A, 4), np.float32)
    conf = np.zeros((1, A, 2), np.float32)
    conf[0, :, 0] = 4.0                          # background everywhere ...
    half = [100, 5000, 12000, 16000]
    conf[0, half] = 0.0                          # ... score exactly 0.5 here
    conf[0, 9000] = (0.0, 3.0)                   # ... and a clearly strong box here
    got = {}
    for name, kw in (("c50", dict(confidence=0.5)), ("c60_r50", dict(confidence=0.6, rescue=0.5)),
                     ("c60_r55", dict(confidence=0.6, rescue=0.55)), ("c60", dict(confidence=0.6))):
        ctx = vdmi.Context(precision="fp32", max_batch=1, **kw)
        try:
            ctx.load_weights(0, face_weights())
            d = ctx.postprocess(loc, conf, (640, 640), cap=64)
            rb = ctx.read_boxes(0, 1, cap=64)
            wk = ctx.read_rescue(0, 1, "weak", cap=64) if "rescue" in kw else None
            got[name] = (d, rb, wk)
        finally:
            ctx.close()
    lab = lambda b: sorted(int(v) for v in b.frame(0)[3])
    assert lab(got["c50"][0]) == sorted(half + [9000])
    assert [float(s) for s in got["c50"][0].frame(0)[2][1:]] == [0.5] * 4
    for name in ("c60_r50", "c60_r55", "c60"):
        for b in got[name][:2]:                  # the caller's list and vd_read_boxes: the strong box only
            assert lab(b) == [9000] and int(b.count[0]) == 1
        for a, b in zip(got[name][0].frame(0), got["c60"][0].frame(0)):
            np.testing.assert_array_equal(a, b)
    wk = got["c60_r50"][2]
    assert lab(wk) == sorted(half) and [float(s) for s in wk.frame(0)[2]] == [0.5] * 4
    assert int(got["c60_r55"][2].count[0]) == 0
    # D ++ W at (0.6, 0.5) is the keep list at 0.5 in every field
    for k in range(4):
        np.testing.assert_array_equal(np.concatenate([got["c60_r50"][0].frame(0)[k], wk.frame(0)[k]]),
                                      got["c50"][0].frame(0)[k])


# ---- through the networks ------------------------------------------------------------------------

H, W_ = 360, 640


def _frame(i):
    from vdmi import synth
    return np.repeat(np.repeat(synth.frame(180, 320, i, seed=5), 2, 0), 2, 1)     # 360x640, faces fire


_NETS = {}


@pytest.fixture(scope="module")
def net_ctx(gpu):
    """fp32 contexts with seeded RetinaFace + YOLO weights by their keyword arguments."""
    import vdmi
    from vdmi import weights

    def make(**kw):
        key = tuple(sorted(kw.items()))
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


def _lists(boxes, b):
    k = int(boxes.count[b])
    assert k <= boxes.cap
    return [tuple(int(v) for v in r) for r in boxes.xyxy[b, :k]]


def _fields(boxes, b):
    return [np.array(a) for a in boxes.frame(b)]


def test_prefix_property_through_the_networks(net_ctx, clip_frames):
    """The keep list at `low`, cut at the net's threshold, is the keep list at that threshold: a rescue
    context returns bit-identical faces, plates and vd_read_boxes, and its D ++ W is the keep list of a
    context whose thresholds are the low ones, in every field."""
    batch = np.stack([clip_frames[0], clip_frames[2], clip_frames[4], clip_frames[0]])
    off = net_ctx()
    on = net_ctx(rescue=0.2, plate_rescue=0.25)
    low = net_ctx(confidence=0.2, plate_conf=0.25)
    res = {}
    for name, ctx in (("off", off), ("on", on), ("low", low)):
        _, faces, plates = ctx.process(batch, flags=_flags())
        res[name] = (faces, plates, ctx.read_boxes(0, 4), ctx.read_boxes(1, 4))
    wk = [on.read_rescue(net, 4, "weak") for net in (0, 1)]
    for b in range(4):
        for k in range(4):                       # faces, plates, read_boxes of both nets
            for x, y in zip(_fields(res["off"][k], b), _fields(res["on"][k], b)):
                np.testing.assert_array_equal(x, y, err_msg=f"frame {b} list {k}")
            assert int(res["off"][k].count[b]) == int(res["on"][k].count[b])
        for net in (0, 1):
            d, w_, full = _fields(res["on"][2 + net], b), _fields(wk[net], b), _fields(res["low"][2 + net], b)
            for x, y, z in zip(d, w_, full):
                np.testing.assert_array_equal(np.concatenate([x, y]), z, err_msg=f"frame {b} net {net}")
        assert int(res["on"][2].count[b]) > 0 and int(wk[0].count[b]) > 0      # both parts are non-empty
        sc = wk[0].frame(b)[2]
        assert float(sc.max()) < 0.5 and float(sc.min()) >= 0.2
    assert sum(int(c) for c in wk[1].count) + sum(int(c) for c in res["on"][3].count) == \
        sum(int(c) for c in res["low"][3].count)


def _process_sequence(ctx, frames, calls, K, rescue=True):
    """frames through ctx.process in `calls`: per frame the output, D_t, W_t, and what read_rescue and
    read_held return (boxes, labels)."""
    outs, D, Wk, R, Hh = [], [], [], [], []
    lo = 0
    for n in calls:
        out, faces, plates = ctx.process(np.stack(frames[lo:lo + n]), flags=_flags())
        held = ctx.read_held(n) if K else None
        if rescue:
            weak = [ctx.read_rescue(net, n, "weak") for net in (0, 1)]
            resc = [ctx.read_rescue(net, n, "rescued") for net in (0, 1)]
        for b in range(n):
            outs.append(out[b])
            D.append(_lists(faces, b) + _lists(plates, b))
            if rescue:
                Wk.append(_lists(weak[0], b) + _lists(weak[1], b))
                r0, r1 = _rows(resc[0], b), _rows(resc[1], b)
                R.append((r0[0] + r1[0], r0[1] + r1[1]))
                sc = resc[0].frame(b)[2]
                assert len(sc) == 0 or (float(sc.max()) < 0.5 and float(sc.min()) >= 0.2)
            if K:
                Hh.append(_rows(held, b))
        lo += n
    return outs, D, Wk, R, Hh


def _check_e2e(ctx, frames, calls, K, S, render):
    outs, D, Wk, R, Hh = _process_sequence(ctx, frames, calls, K)
    E, since, Rr, _, _ = rr.rescue_lists(D, Wk, H, W_, max(1, K), S, 30)
    assert [r for r, _ in R] == Rr
    assert [s for _, s in R] == [s[len(d):] for s, d in zip(since, D)]
    B, Hr, ar, _ = hr.hold_lists(E, H, W_, K, 30)
    if K:
        assert [h for h, _ in Hh] == Hr and [a for _, a in Hh] == ar
    for t, fr in enumerate(frames):
        np.testing.assert_array_equal(outs[t], render(fr, B[t]), err_msg=f"frame {t}")
    return outs, D, Wk, Rr, since


def test_process_rescues_weak_boxes_across_calls(net_ctx, clip_frames):
    """[A, A, B, B, C, A] as calls of 4 + 2 at hold=2, rescue=0.2, rescue_span=3: read_rescue equals the
    reference over the GPU's own D and W lists, read_held equals the hold reference over E, every output
    frame is the oracle mosaic of B_t = E_t ++ H_t; with rescue off the same detections give other pixels."""
    K, S = 2, 3
    outs, D, Wk, R, since = _check_e2e(net_ctx(hold=K, rescue=0.2, rescue_span=S), clip_frames, (4, 2), K, S,
                                       lambda fr, b: omosaic.mosaic_frame(fr, b, 8))
    assert sum(len(r) for r in R) > 0 and R[0] == []
    assert any(s >= 2 for row in since for s in row)
    assert sum(len(k) for k in Wk) - sum(len(r) for r in R) > 0
    outs0, D0, _, _, Hh0 = _process_sequence(net_ctx(hold=K), clip_frames, (4, 2), K, rescue=False)
    assert D0 == D
    B0, _, _, _ = hr.hold_lists(D, H, W_, K, 30)
    for t, fr in enumerate(clip_frames):
        np.testing.assert_array_equal(outs0[t], omosaic.mosaic_frame(fr, B0[t], 8), err_msg=f"frame {t}")
    assert any(not np.array_equal(x, y) for x, y in zip(outs, outs0))


def test_process_rescues_weak_boxes_gaussian(net_ctx, clip_frames):
    from vdmi import _lib
    q = _lib.blur_weights(9, 0.0)
    _, _, _, R, _ = _check_e2e(net_ctx(hold=2, rescue=0.2, rescue_span=3, blur="gaussian", blur_ksize=9),
                               clip_frames[1:5], (4,), 2, 3, lambda fr, b: gr.blur_frame(fr, b, 9, 0.0, q=q))
    assert sum(len(r) for r in R) > 0


def test_process_without_hold_uses_a_window_of_one(net_ctx, clip_frames):
    _, _, _, R, _ = _check_e2e(net_ctx(rescue=0.2, rescue_span=3), clip_frames[:4], (3, 1), 0, 3,
                               lambda fr, b: omosaic.mosaic_frame(fr, b, 8))
    assert sum(len(r) for r in R) > 0


def test_process_lead_matches_on_E(net_ctx, clip_frames):
    """lead=2 with rescue: read_lead's B_t equals the lead reference over E (calls of 4 + 2 + flush), and
    the emitted frames are its oracle mosaic."""
    J, S = 2, 3
    ctx = net_ctx(lead=J, rescue=0.2, rescue_span=S)
    outs, D, Wk, B, lo = [], [], [], [], 0
    for n in (4, 2, 0):
        if n:
            out, faces, plates = ctx.process_lead(np.stack(clip_frames[lo:lo + n]), flags=_flags())
            weak = [ctx.read_rescue(net, n, "weak") for net in (0, 1)]
            D += [_lists(faces, b) + _lists(plates, b) for b in range(n)]
            Wk += [_lists(weak[0], b) + _lists(weak[1], b) for b in range(n)]
        else:
            out = ctx.lead_flush()
        if len(out):
            rows = ctx.read_lead(len(out), "all")
            B += [_rows(rows, i) for i in range(len(out))]
        outs += list(out)
        lo += n
    E, _, R, _, _ = rr.rescue_lists(D, Wk, H, W_, 1, S, 30)
    wantB, wantL = lr.blur_lists(E, H, W_, J, 30)
    assert [b for b, _ in B] == wantB and [l for _, l in B] == wantL
    assert sum(len(r) for r in R) > 0 and any(v < 0 for l in wantL for v in l)
    for t, fr in enumerate(clip_frames):
        np.testing.assert_array_equal(outs[t], omosaic.mosaic_frame(fr, wantB[t], 8), err_msg=f"frame {t}")


def test_off_is_off(gpu, clip_frames):
    """A context whose rescue was set and cleared, and one that never heard of it: identical outputs,
    vd_read_boxes and family-3 step counts; with rescue on the count grows by exactly RESCUE_STEPS."""
    import vdmi
    from vdmi import _lib, weights
    sd = weights.retinaface_state_dict(0)
    batch = np.stack(clip_frames[:4])
    res = {}
    for name in ("never", "cleared", "on"):
        ctx = vdmi.Context(precision="fp32", max_batch=4, hold=2, **({"rescue": 0.2} if name == "on" else {}))
        try:
            if name == "cleared":
                ctx.rescue(0.3, 0.0, 9)
                ctx.rescue(0.0)
            ctx.load_weights(0, sd)
            ctx.timing(True)
            ctx.timing_reset()
            out, faces, _ = ctx.process(batch)
            ctx.sync()
            rb = ctx.read_boxes(0, 4)
            res[name] = (out.copy(), [[a.tolist() for a in _fields(faces, b)] for b in range(4)],
                         [[a.tolist() for a in _fields(rb, b)] for b in range(4)],
                         [ctx.timing_read(f)[1] for f in range(7)])
        finally:
            ctx.close()
    np.testing.assert_array_equal(res["never"][0], res["cleared"][0])
    assert res["never"][1:] == res["cleared"][1:]
    assert res["on"][1:3] == res["never"][1:3]
    on, never = res["on"][3], res["never"][3]
    assert on[_lib.FAM_POST] == never[_lib.FAM_POST] + RESCUE_STEPS
    assert [v for f, v in enumerate(on) if f != _lib.FAM_POST] == [v for f, v in enumerate(never) if f != _lib.FAM_POST]


# ---- pipeline ---------------------------------------------------------------------------------------

N = 9


def _detectors(device_ids, rescue, span=3, hold=2):
    import vdmi
    from vdmi import weights
    face = vdmi.Retinaface(input_shape=[640, 640, 3], nms_iou=0.4, max_batch=4, device_ids=device_ids,
                           weights=weights.retinaface_state_dict(0), hold=hold, rescue=rescue, rescue_span=span)
    plate = vdmi.YOLO(weights="random", max_batch=4, device_ids=device_ids)
    return face, plate


def test_batch_process_images_rescue(gpu, tmp_path, net_ctx):
    """batch_process_images(rescue=0.2, rescue_span=3, hold=2, batch_size=4) over 9 frames: the written
    frames equal the oracle mosaic of B_t = E_t ++ H_t built by the references from a plain context's D
    and W lists, the records stay the detections, and two device shards (each warmed up on the
    rescue_span + hold frames before it) write the same bytes."""
    from vdmi.pipeline import batch_process_images
    K, S = 2, 3
    frames = {f"f{i:03d}.jpg": _frame(i) for i in range(N)}
    names = sorted(frames)
    (tmp_path / "in").mkdir()
    for n in names:
        (tmp_path / "in" / n).write_bytes(b"")
    ctx = net_ctx(rescue=0.2)
    D, Wk = [], []
    for lo in range(0, N, 4):
        n = min(4, N - lo)
        _, faces, plates = ctx.process(np.stack([frames[k] for k in names[lo:lo + n]]), flags=_flags())
        weak = ctx.read_rescue(0, n, "weak")
        D += [_lists(faces, b) + _lists(plates, b) for b in range(n)]
        Wk += [_lists(weak, b) for b in range(n)]
    E, _, R, _, _ = rr.rescue_lists(D, Wk, H, W_, K, S, 30)
    B, _, _, _ = hr.hold_lists(E, H, W_, K, 30)
    assert sum(len(r) for r in R) > 0
    runs = {}
    for name, ids, shard in (("one", [0], None), ("two", [0, 0], "devices")):
        saved, rec = {}, {}
        tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / name), *_detectors(ids, 0.2), batch_size=4,
                                   shard=shard, records=rec, mosaic_plates=True, hold=K, rescue=0.2, rescue_span=S,
                                   loader=lambda p: frames[os.path.basename(p)],
                                   saver=lambda img, p, saved=saved: saved.__setitem__(os.path.basename(p), img.copy()))
        runs[name] = (tot, rec, saved)
    tot, rec, saved = runs["one"]
    assert tot[0] == N and tot[1] + tot[2] == sum(len(d) for d in D)         # totals: the detections only
    for t, n in enumerate(names):
        got = []
        for key in ("faces", "plates"):
            v = rec[n][key]
            if v is not None:
                assert int(v[3]) <= len(v[0])
                got += [tuple(int(x) for x in b) for b in v[0][:int(v[3])]]
        assert got == D[t], n                             # records: the detections only, every box of the frame
        np.testing.assert_array_equal(saved[f"processed_{n}"], omosaic.mosaic_frame(frames[n], B[t], 8), err_msg=n)
    t2, r2, s2 = runs["two"]
    assert t2 == tot and sorted(s2) == sorted(saved)
    for k in saved:
        np.testing.assert_array_equal(saved[k], s2[k], err_msg=k)


def test_batch_process_images_rescue_needs_matching_detectors(gpu, tmp_path):
    from vdmi.pipeline import batch_process_images
    (tmp_path / "in").mkdir()
    for det, kw in ((_detectors([0], 0.0), dict(rescue=0.2, rescue_span=3)),
                    (_detectors([0], 0.2), dict(rescue=0.2, rescue_span=4)),
                    (_detectors([0], 0.2), dict(rescue=0.2, plate_rescue=0.25, rescue_span=3))):
        with pytest.raises(ValueError, match="rescue"):
            batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), *det, hold=2, **kw)


def test_dropped_batch_resets_the_rescue_history(gpu, tmp_path, net_ctx):
    """A batch whose inference fails is dropped; the batch after it must not rescue weak boxes over the
    gap: frame 8 is blurred with its strong boxes only, although it has weak boxes that match frame 3's."""
    from vdmi.pipeline import batch_process_images, fused_context
    frames = {f"f{i:03d}.jpg": _frame(i) for i in range(N)}
    (tmp_path / "in").mkdir()
    for n in frames:
        (tmp_path / "in" / n).write_bytes(b"")
    face, plate = _detectors([0], 0.2, hold=0)
    ctx = fused_context(face, plate, 4)
    real, calls = ctx.process, []

    def flaky(*a, **k):
        calls.append(1)
        if len(calls) == 2:                              # the second batch: frames 4..7
            raise RuntimeError("inference failure")
        return real(*a, **k)

    ctx.process = flaky
    saved, rec = {}, {}
    tot = batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), face, plate, batch_size=4, shard=None,
                               records=rec, mosaic_plates=True, rescue=0.2, rescue_span=3,
                               loader=lambda p: frames[os.path.basename(p)],
                               saver=lambda img, p: saved.__setitem__(os.path.basename(p), img.copy()))
    assert tot[0] == 5 and len(calls) == 3
    d8 = []
    for key in ("faces", "plates"):
        v = rec["f008.jpg"][key]
        if v is not None:
            d8 += [tuple(int(x) for x in b) for b in v[0][:int(v[3])]]
    np.testing.assert_array_equal(saved["processed_f008.jpg"], omosaic.mosaic_frame(frames["f008.jpg"], d8, 8))
    # without the reset frame 8 would have rescued boxes over frame 3's
    plain = net_ctx(rescue=0.2)
    _, f, p = plain.process(np.stack([frames["f003.jpg"], frames["f008.jpg"]]), flags=_flags())
    assert sum(int(c) for c in plain.read_rescue(0, 2, "rescued").count) > 0


def test_plate_split_is_strict_at_both_thresholds(gpu):
    """Class logit 0 gives a plate score of exactly 0.5. The plate test is strict: such a box is not
    strong at plate_conf=0.5, not weak at plate_rescue=0.5, weak at plate_rescue=0.45; and D ++ W at
    (0.6, 0.45) is the keep list at plate_conf=0.45 in every field."""
    import vdmi
    from vdmi import weights
    sd = weights.yolov8n_state_dict(0)
    frames = np.stack([_frame(0)])
    half = [10 * 80 + 10, 10 * 80 + 40, 35 * 80 + 10, 35 * 80 + 40]      # level 0 (stride 8), 240 px apart
    got = {}
    for name, kw in (("c50", dict(plate_conf=0.5)), ("c60_r50", dict(plate_conf=0.6, plate_rescue=0.5)),
                     ("c60_r45", dict(plate_conf=0.6, plate_rescue=0.45)), ("c45", dict(plate_conf=0.45))):
        ctx = vdmi.Context(precision="fp32", max_batch=1, **kw)
        try:
            ctx.load_weights(1, sd)
            raw = np.zeros_like(ctx.plate_raw(frames))       # the forward also fixes the canvas
            assert raw.shape == (1, 65, 5040)
            raw[0, 64, :] = -10.0
            raw[0, 64, half] = 0.0
            raw[0, 64, 10 * 80 + 70] = 3.0
            d = ctx.plate_postprocess(raw, (H, W_), cap=16)
            wk = ctx.read_rescue(1, 1, "weak", cap=16) if "plate_rescue" in kw else None
            got[name] = (d, ctx.read_boxes(1, 1, cap=16), wk)
        finally:
            ctx.close()
    for name in ("c50", "c60_r50", "c60_r45"):
        for b in got[name][:2]:
            assert int(b.count[0]) == 1 and float(b.score[0, 0]) > 0.9
        for x, y in zip(_fields(got[name][0], 0), _fields(got["c50"][0], 0)):
            np.testing.assert_array_equal(x, y)
    assert int(got["c60_r50"][2].count[0]) == 0
    wk = got["c60_r45"][2]
    assert int(wk.count[0]) == 4 and [float(s) for s in wk.frame(0)[2]] == [0.5] * 4
    assert int(got["c45"][0].count[0]) == 5
    for k in range(4):
        np.testing.assert_array_equal(np.concatenate([got["c60_r45"][0].frame(0)[k], wk.frame(0)[k]]),
                                      got["c45"][0].frame(0)[k])
