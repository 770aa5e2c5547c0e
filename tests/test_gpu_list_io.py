"""Caller box lists into vd_hold, vd_lead_lists and vd_rescue_lists (csrc/frames.cpp
Ctx::box_list_in): a device list whose xyxy is not 16-byte aligned is staged, because hold.hip,
lead.hip and rescue.hip read boxes as 16-byte vectors, and the staging of a host list may be
reused by the next call while the first call's device output has not been read yet. Exact
against tests/hold_ref.py, tests/lead_ref.py and tests/rescue_ref.py; no weights."""
import numpy as np
import pytest

import hold_ref as hr
import lead_ref as lr
import rescue_ref as rr

H = W = 64
CAP = 4
K, J, S, P = 2, 1, 5, 30
A, A2, FAR = (10, 10, 30, 30), (11, 10, 31, 30), (40, 40, 60, 62)
SEQ = [[[A], [A, FAR], []], [[FAR], [], [A2]]]                # two calls of 3 frames
WEAK = [[[], [], [A2, (41, 40, 61, 62)]], [[A], [FAR], []]]     # the weak lists beside SEQ as the strong ones
KINDS = {"hold": dict(hold=K), "lead": dict(lead=J), "rescue": dict(hold=1, rescue=0.2, rescue_span=S)}


@pytest.fixture
def ctx_of(gpu):
    """Fresh weight-less contexts by kind; closed after the test."""
    import vdmi
    made = []

    def make(kind):
        made.append(vdmi.Context(precision="fp32", max_batch=4, hold_iou_pct=P, **KINDS[kind]))
        return made[-1]

    yield make
    for c in made:
        c.close()


def _host(seq):
    from vdmi import _lib
    hb = _lib.HostBoxes(len(seq), CAP)
    for i, d in enumerate(seq):
        hb.count[i] = len(d)
        hb.xyxy[i, :len(d)] = np.asarray(d, np.int32).reshape(-1, 4)
    return hb


def _device(seq, pad):
    """Device lists whose xyxy starts `pad` int32 elements into its tensor (pad 1: address = 4 mod 16)."""
    import torch
    from vdmi import _lib
    from vdmi.context import DeviceBoxes

    class Padded(DeviceBoxes):
        def struct(self):
            return _lib.vd_boxes(self.cap, _lib.VD_DEVICE, self.count.data_ptr(), self.flat.data_ptr() + 4 * pad,
                                 None, None, None)

    hb = _host(seq)
    db = Padded.__new__(Padded)
    db.n, db.cap = hb.n, hb.cap
    db.count = torch.from_numpy(hb.count).to("cuda:0")
    db.flat = torch.zeros(pad + hb.xyxy.size, dtype=torch.int32, device="cuda:0")
    db.flat[pad:] = torch.from_numpy(hb.xyxy.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    assert db.struct().xyxy % 16 == (4 * pad) % 16
    return db


def _rows(out, m):
    """[(boxes, labels)] of rows [0, m) of a HostBoxes / DeviceBoxes."""
    cnt, xy, lab = (np.asarray(t.cpu()) if hasattr(t, "cpu") else t for t in (out.count, out.xyxy, out.label))
    assert int(cnt[:m].max(initial=0)) <= out.cap
    return [([tuple(int(v) for v in r) for r in xy[i, :cnt[i]]], [int(v) for v in lab[i, :cnt[i]]]) for i in range(m)]


def _call(ctx, kind, mk, call, out):
    """One call of `kind` over SEQ[call] (and WEAK[call]) with inputs made by mk; every frame leaves."""
    if kind == "hold":
        ctx.hold(mk(SEQ[call]), H, W, out=out)
    elif kind == "lead":
        _, m = ctx.lead_lists(mk(SEQ[call]), H, W, flush=True, out=out)
        assert m == len(SEQ[call])
    else:
        ctx.rescue_lists(mk(SEQ[call]), mk(WEAK[call]), H, W, out=out)


def _reference(kind):
    """[(boxes, labels)] per frame of both calls, the second continuing the first where a history carries on."""
    want = []
    if kind == "hold":
        hist = None
        for seq in SEQ:
            B, Hl, ages, hist = hr.hold_lists(seq, H, W, K, P, hist)
            want.append([(b, [0] * (len(b) - len(h)) + a) for b, h, a in zip(B, Hl, ages)])
    elif kind == "lead":                       # each call ends its stream with a flush
        for seq in SEQ:
            B, labels = lr.blur_lists(seq, H, W, J, P)
            want.append(list(zip(B, labels)))
    else:
        hist = None
        for seq, weak in zip(SEQ, WEAK):
            E, since, _, _, hist = rr.rescue_lists(seq, weak, H, W, 1, S, P, hist)
            want.append(list(zip(E, since)))
    return want


WANT = {kind: _reference(kind) for kind in KINDS}


def test_references_hold_lead_and_rescue_something():
    """The sequences are not vacuous: a box is held, led and rescued in either call, within CAP."""
    for kind in KINDS:
        for call in WANT[kind]:
            assert any(any(v != 0 for v in lab) for _, lab in call), kind
            assert all(len(b) <= CAP for b, _ in call), kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_unaligned_device_lists(ctx_of, kind):
    """xyxy at data_ptr() + 4 (both inputs for rescue): the reference's lists, and the aligned call's."""
    from vdmi import _lib
    got = []
    for pad in (1, 0):
        out = _lib.HostBoxes(3, CAP)
        _call(ctx_of(kind), kind, lambda seq: _device(seq, pad), 0, out)
        got.append(_rows(out, 3))
    assert got[0] == WANT[kind][0]
    assert got[1] == got[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_list_staging_is_reused_by_the_next_call(ctx_of, kind):
    """Two calls back to back, host inputs and device outputs (no host wait on the output), other
    lists in the second: both outputs, read afterwards, are their references."""
    import torch
    from vdmi.context import DeviceBoxes
    ctx = ctx_of(kind)
    outs = [DeviceBoxes(3, CAP, "cuda:0") for _ in SEQ]
    torch.cuda.synchronize()
    for call, out in enumerate(outs):
        _call(ctx, kind, _host, call, out)
    ctx.sync()
    for call, out in enumerate(outs):
        assert _rows(out, 3) == WANT[kind][call], call
