"""Rescue on tiled nets on the GPU (include/vdmi.h at vd_rescue_tiles): the merge kernel's rescue form
alone against tests/rescue_tiles_ref.py; the switch (off is off, the state rules); and vd_process /
vd_process_nv12 / vd_process_lead end to end in contexts that tile and rescue, against the reference merge,
cut and rescue of per-crop detections at the low threshold. Everything is exact. 360 x 640 frames, the fp32
plan, the `dense` seeded face weights, tiles (2, 2, 20): T = 5, max_batch 10, so two frames per call."""
import numpy as np
import pytest

import hold_ref as hr
import lead_ref as lr
import nv12_ref as nr
import rescue_tiles_ref as rtr
import tiles_ref as tr
from oracle import mosaic as omosaic

pytestmark = pytest.mark.gpu

A640 = 16800
H, W = 360, 640
# plate_conf is the default: naming it keeps these contexts (which also hold plate weights) apart from the
# face-only contexts other modules cache under the same settings
NET = dict(precision="fp32", max_batch=10, wkind="dense", plate_conf=0.5)
TILED = dict(tiles=(2, 2), tile_overlap=20)
LOW, PLOW, SPAN, HOLD = 0.2, 0.25, 3, 1       # 0.2 first, as the rescue tests use; the plate net: as they use
IOU = {False: 0.4, True: 0.7}
THR = 0.5


def _ctx(factory, **kw):
    from vdmi import weights
    ctx = factory(**{**NET, **kw})
    if not getattr(ctx, "_plates_loaded", False):
        ctx.load_weights(1, weights.yolov8n_state_dict(0))
        ctx._plates_loaded = True
    ctx.hold_reset()
    return ctx


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(b, i):
    k = int(b.count[i])
    assert k <= b.cap
    return b.xyxy[i, :k], b.xyxy_f[i, :k], b.score[i, :k], b.label[i, :k]


def _assert_rows(got, i, ref, what):
    """Row i of a HostBoxes against a merge_frame tuple, every field, bit for bit."""
    xi, xf, sc, lab = _rows(got, i)
    assert len(xi) == len(ref[0]), f"{what}: count {len(xi)} != {len(ref[0])}"
    assert np.array_equal(xi, ref[0]), f"{what}: int boxes"
    assert np.array_equal(_bits(xf), _bits(ref[1])), f"{what}: float boxes"
    assert np.array_equal(_bits(sc), _bits(ref[2])), f"{what}: scores"
    assert np.array_equal(lab, ref[3]), f"{what}: labels"


def _host(li):
    from vdmi import _lib
    b = _lib.HostBoxes(li.n, li.cap)
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        getattr(b, k)[...] = getattr(li, k)
    return b


def _device(li):
    import torch
    from vdmi.context import DeviceBoxes
    d = DeviceBoxes(li.n, li.cap, "cuda")
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        getattr(d, k).copy_(torch.from_numpy(getattr(li, k)))
    torch.cuda.synchronize()                            # the context reads them on its own stream
    return d


def _prefix_lists(li, T, thr, plates):
    """The per-input strong prefixes of `li` as lists of the same shape."""
    out = rtr.Lists(li.n, li.cap)
    for r in range(li.n):
        k = int(rtr.strong_mask(li.score[r, :int(li.count[r])], thr, plates).sum())
        out.count[r] = k
        for name in ("xyxy", "xyxy_f", "score", "label"):
            getattr(out, name)[r, :k] = getattr(li, name)[r, :k]
    return out


# ---- 1. the merge kernel alone ------------------------------------------------------------------------
ALL5 = (0, 1, 2, 3, 4)
MERGE_CASES = {
    # name: (plates, cap, random_lists keywords, output cap or None, lists in device memory)
    "lds": (False, 64, {}, None, False),
    "lds_device": (False, 64, {}, None, True),
    "spill": (False, 512, {}, None, False),                          # 5 x 512 = 2560 > the 2048 held in LDS
    "spill_device": (False, 512, {}, None, True),
    "tied_at_thr": (False, 64, dict(scores=(0.5,)), None, False),      # faces: all strong
    "all_weak": (False, 64, dict(scores=(0.45, 0.3, 0.2)), None, False),
    "all_strong": (False, 64, dict(scores=(0.9, 0.75)), None, False),
    "all_empty": (False, 8, dict(empty=ALL5), None, False),
    "one_empty": (False, 64, dict(empty=(2,)), None, False),
    "small_cap": (False, 64, {}, 8, False),
    "plates": (True, 64, {}, None, False),
    "plates_tied_at_thr": (True, 64, dict(scores=(0.5,)), None, False),   # plates: all weak
    # the plate net keeps at most 300 boxes per input: past 2048 only with T = 7 (tiles (2, 3), one frame a call)
    "plates_spill": (True, 300, dict(objects=2500), None, True),
}


@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_low_equals_reference(face_ctx_factory, case):
    """vdt_tiles_merge_low: the strong list the merge hands the caller and the whole merged rows with both
    counts equal the reference merge at low and its cut; the strong list also equals tiles_merge() of the
    per-input strong prefixes (the kernel form that runs with rescue off); entries of the caller's device
    arrays past the strong count are never written."""
    from vdmi import _lib
    plates, cap, kw, ocap, device = MERGE_CASES[case]
    ctx = _ctx(face_ctx_factory, **(dict(tiles=(2, 3), tile_overlap=20) if case == "plates_spill" else TILED))
    rects = ctx.tile_rects(H, W)
    T = len(rects)
    n = 10 // T
    origins = [(int(q[0]), int(q[1])) for q in rects]
    li = rtr.random_lists(sorted(MERGE_CASES).index(case), n, rects, cap, plates=plates, **kw)
    full = max(1, T * cap)
    # the strong arrays in device memory, where the kernel itself writes them (a host list comes back through
    # the staging, whole rows): what it leaves alone keeps the fill
    fill = rtr.Lists(n, ocap or full)
    for a in (fill.xyxy, fill.label):
        a[...] = -7
    fill.xyxy_f[...] = -7.0
    fill.score[...] = -7.0
    dstrong = _device(fill)
    _, whole = ctx.tiles_merge_low(_device(li) if device else _host(li), H, W, THR, plates=plates, strong=dstrong)
    ctx.sync()
    strong = _lib.HostBoxes(n, ocap or full)
    for k in ("count", "xyxy", "xyxy_f", "score", "label"):
        getattr(strong, k)[...] = getattr(dstrong, k).cpu().numpy()
    pre = _prefix_lists(li, T, THR, plates)
    off = (ctx.tiles_merge_plates if plates else ctx.tiles_merge)(_host(pre), H, W)
    ns = nw = 0
    for f in range(n):
        D, Wk, merged = rtr.split_frame(li.frame_lists(f, T), origins, A640, IOU[plates], THR, plates)
        print(f"{case} frame {f}: inputs {int(li.count[f * T:(f + 1) * T].sum())} merged {len(merged[2])} strong {len(D[2])}")
        _assert_rows(whole, f, merged, f"{case} frame {f} whole")
        k = len(D[2])
        assert int(strong.count[f]) == k                              # complete, whatever the cap
        kc = min(k, strong.cap)
        assert np.array_equal(strong.xyxy[f, :kc], D[0][:kc]) and np.array_equal(_bits(strong.xyxy_f[f, :kc]), _bits(D[1][:kc]))
        assert np.array_equal(_bits(strong.score[f, :kc]), _bits(D[2][:kc])) and np.array_equal(strong.label[f, :kc], D[3][:kc])
        assert (strong.xyxy[f, kc:] == -7).all() and (strong.label[f, kc:] == -7).all()
        assert (strong.xyxy_f[f, kc:] == -7.0).all() and (strong.score[f, kc:] == -7.0).all()
        _assert_rows(off, f, D, f"{case} frame {f} rescue-off merge of the strong prefixes")
        ns += k
        nw += len(Wk[2])
    if "spill" in case:
        assert int(li.count[:T].sum()) > 2048
    if case in ("all_weak", "plates_tied_at_thr"):
        assert ns == 0 and nw > 0
    elif case in ("all_strong", "tied_at_thr"):
        assert ns > 0 and nw == 0
    elif case == "all_empty":
        assert ns == 0 and nw == 0 and not whole.count.any()
    else:
        assert ns > 0 and nw > 0
    if case == "small_cap":
        assert ns > 2 * strong.cap


# ---- 2. off is off, and the state rules ----------------------------------------------------------------
def _frames_nv(idx, seed=5):
    """Synthetic 360 x 640 scenes on which the seeded weights fire (pixels doubled), as packed NV12."""
    from vdmi import synth
    rgb = np.stack([np.repeat(np.repeat(synth.frame(H // 2, W // 2, i, seed=seed), 2, 0), 2, 1) for i in idx])
    return nr.from_rgb(rgb)


def _same_rows(a, b, n):
    assert np.array_equal(a.count[:n], b.count[:n])
    for f in range(n):
        for x, y in zip(_rows(a, f), _rows(b, f)):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y), f


def test_switch_off_keeps_the_refusals(gpu):
    import vdmi
    from vdmi import _lib
    tiled = vdmi.Context(precision="fp32", max_batch=5, **TILED)
    with pytest.raises(_lib.VdError, match="vd_rescue: rescue and tiled detection \\(vd_tiles\\) cannot be combined") as e:
        tiled.rescue(0.2)
    assert e.value.code == _lib.VD_ERR_STATE and tiled.rescue_low == 0.0
    resc = vdmi.Context(precision="fp32", max_batch=5, rescue=0.2)
    with pytest.raises(_lib.VdError, match="vd_tiles: tiled detection and rescue \\(vd_rescue\\) cannot be combined") as e:
        resc.set_tiles((2, 2), 20)
    assert e.value.code == _lib.VD_ERR_STATE and resc.tiles == (1, 1)
    for c in (tiled, resc):
        assert c._lib.vd_rescue_tiles(c._h, 2) == _lib.VD_ERR_ARG and c._lib.vd_rescue_tiles(c._h, -1) == _lib.VD_ERR_ARG
        c.set_rescue_tiles(False)                                 # the value it has: nothing happens
    # on: both orders are accepted; off again is refused while both are on, and changes nothing
    tiled.set_rescue_tiles(True)
    tiled.rescue(0.2)
    resc.set_rescue_tiles(True)
    resc.set_tiles((2, 2), 20)
    for c in (tiled, resc):
        with pytest.raises(_lib.VdError, match="vd_rescue.*vd_tiles") as e:
            c.set_rescue_tiles(False)
        assert e.value.code == _lib.VD_ERR_STATE and c.rescue_tiles is True
        c.set_tiles((2, 3), 20)                                   # still on: the combination is still accepted
        c.set_tiles((1, 1))
        c.set_rescue_tiles(False)                                 # one of the two is off: accepted
        with pytest.raises(_lib.VdError, match="tiled detection"):
            c.set_tiles((2, 2), 20)
        c.close()


def test_switch_on_with_rescue_off_changes_nothing(face_ctx_factory):
    """detect / process of 2 frames in a tiled context with the switch on and rescue off equal those of a
    tiled context that never saw the switch: lists and pixels."""
    frames = nr.to_rgb(_frames_nv([0, 1]))
    never = _ctx(face_ctx_factory, **TILED)
    on = _ctx(face_ctx_factory, **TILED, rescue_tiles=True)
    assert on.rescue_tiles and not never.rescue_tiles
    _same_rows(on.detect(frames), never.detect(frames), 2)
    oa, fa, _ = on.process(frames)
    ob, fb, _ = never.process(frames)
    assert np.array_equal(oa, ob) and int(fa.count.sum()) > 0
    _same_rows(fa, fb, 2)
    _same_rows(on.read_boxes(0, 2), never.read_boxes(0, 2), 2)


# ---- 3..5. end to end ---------------------------------------------------------------------------------
IDX = [0, 0, 1, 1]        # a 4-frame stream: every scene twice, so what is weak in a frame meets its own past


def _flags(plates):
    from vdmi import _lib
    f = _lib.VD_PROC_FACES | _lib.VD_PROC_MOSAIC
    return f | _lib.VD_PROC_PLATES | _lib.VD_PROC_MOSAIC_PLATES if plates else f


def _input_lists(plain, frames, rects, net):
    """The per-input lists at the low threshold, from the library itself: every rectangle as a frame of its
    own through an UNTILED rescue context; read_boxes ++ read_rescue(which="weak") is its list at low (the
    path tests/test_gpu_rescue.py pins)."""
    n, T = len(frames), len(rects)
    rows = {}

    def run(batch, t):
        (plain.detect if net == 0 else plain.detect_plates)(batch)
        d, w = plain.read_boxes(net, n), plain.read_rescue(net, n, "weak")
        for f in range(n):
            rows[(f, t)] = tuple(np.concatenate([a, b]) for a, b in zip(d.frame(f), w.frame(f)))

    run(frames, 0)
    for t, (x0, y0, tw, th) in enumerate(rects.tolist()[1:], 1):
        run(np.ascontiguousarray(frames[:, y0:y0 + th, x0:x0 + tw]), t)
    li = rtr.Lists(n * T, max(1, max(len(r[2]) for r in rows.values())))
    for (f, t), r in rows.items():
        k = len(r[2])
        li.count[f * T + t] = k
        for name, v in zip(("xyxy", "xyxy_f", "score", "label"), r):
            getattr(li, name)[f * T + t, :k] = v
    return li


@pytest.fixture(scope="module")
def clip(face_ctx_factory):
    """The stream as packed NV12 and as the RGB frames it converts to (what the detectors see either way), the
    rectangles, and the per-input face and plate lists at LOW / PLOW."""
    nv = _frames_nv(IDX)
    frames = nr.to_rgb(nv)
    plain = _ctx(face_ctx_factory, rescue=LOW, plate_rescue=PLOW)
    rects = tr.tile_rects(H, W, 2, 2, 20)
    return dict(nv=nv, frames=frames, rects=rects, faces=_input_lists(plain, frames, rects, 0),
                plates=_input_lists(plain, frames, rects, 1))


EMPTY = (np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), [])


_REF = {}


def _reference(clip, nets, plates, hold=HOLD, lows=(LOW, PLOW)):
    """Computed once per setting and shared (never changed by a test)."""
    key = (nets, plates, hold, lows)
    if key not in _REF:
        _REF[key] = _make_reference(clip, nets, plates, hold, lows)
    return _REF[key]


def _make_reference(clip, nets, plates, hold, lows):
    """Per frame: D and W of both nets as merge tuples (a tiled net with a low: the merged list at low, cut; an
    untiled one: its whole-frame list, cut), then the rescue over D = faces ++ plates, W likewise, and the
    hold over E. lows: a net's 0 leaves it without weak boxes."""
    rects = clip["rects"]
    T = len(rects)
    origins = [(int(q[0]), int(q[1])) for q in rects]
    out = dict(D=[[], []], W=[[], []])
    for f in range(len(IDX)):
        for net in ((0, 1) if plates else (0,)):
            li = clip["plates" if net else "faces"].frame_lists(f, T)
            if not lows[net]:                               # rescue off for this net: the lists at the threshold
                li = rtr.strong_prefixes(li, THR, bool(net))
            if nets in ("both", "plates" if net else "faces"):
                D, Wk, _ = rtr.split_frame(li, origins, A640, IOU[bool(net)], THR, bool(net))
            else:
                whole = tuple(np.asarray(x) for x in li[0])
                k = int(rtr.strong_mask(whole[1], THR, bool(net)).sum())
                xi = np.asarray([[tr.trunc_i32(v) for v in b] for b in whole[0]], np.int32).reshape(-1, 4)
                m = (xi, whole[0], whole[1], whole[2], [(0, p) for p in range(len(whole[1]))])
                D, Wk = rtr.part(m, 0, k), rtr.part(m, k, len(whole[1]))
            out["D"][net].append(D)
            out["W"][net].append(Wk)
        if not plates:
            out["D"][1].append(EMPTY)
            out["W"][1].append(EMPTY)
    strong = [np.concatenate([a[0], b[0]]) for a, b in zip(*out["D"])]
    weak = [np.concatenate([a[0], b[0]]) for a, b in zip(*out["W"])]
    E, since, R, widx, _ = rtr.rescue_stream(strong, weak, H, W, max(1, hold), SPAN, 30)
    out.update(E=E, since=since, R=R, widx=widx, strong=strong, weak=weak)
    out["B"] = hr.hold_lists(E, H, W, hold, 30)[0] if hold else E
    return out


def _figures(ref, clip, net):
    """What the reference shows for one net over the stream (printed, then asserted on by the callers)."""
    T = len(clip["rects"])
    li = clip["plates" if net else "faces"]
    thr_weak = sum(int((~rtr.strong_mask(li.score[r, :int(li.count[r])], THR, bool(net))).sum()) for r in range(li.n))
    nweak = sum(len(w[2]) for w in ref["W"][net])
    nf = [len(w[2]) for w in ref["W"][0]]
    resc = sum(sum(1 for i in ix if (i >= nf[t]) == bool(net)) for t, ix in enumerate(ref["widx"]))
    from_tile = sum(1 for w in ref["W"][net] for t, _ in w[4] if t > 0)
    fig = dict(strong=sum(len(d[2]) for d in ref["D"][net]), weak=nweak, rescued=resc, weak_not_rescued=nweak - resc,
               weak_from_tiles=from_tile, input_weak=thr_weak)
    print(f"net {net}: {fig}")
    return fig


def _check_lists(ctx, ref, t0, n, faces, plates, check_plates):
    """The call's lists of frames [t0, t0 + n) of the stream against the reference: D (the caller's arrays and
    read_boxes), W (read_rescue weak, every field), R with since and score (read_rescue rescued)."""
    for net, got in ((0, faces), (1, plates)) if check_plates else ((0, faces),):
        rb, wk, rs = ctx.read_boxes(net, n), ctx.read_rescue(net, n, "weak"), ctx.read_rescue(net, n, "rescued")
        for b in range(n):
            t = t0 + b
            _assert_rows(got, b, ref["D"][net][t], f"net {net} frame {t} D")
            _assert_rows(rb, b, ref["D"][net][t], f"net {net} frame {t} read_boxes")
            _assert_rows(wk, b, ref["W"][net][t], f"net {net} frame {t} W")
            nf = len(ref["W"][0][t][2])
            ix = [i - (nf if net else 0) for i in ref["widx"][t] if (i >= nf) == bool(net)]
            sn = [s for i, s in zip(ref["widx"][t], ref["since"][t][len(ref["strong"][t]):]) if (i >= nf) == bool(net)]
            Wk = ref["W"][net][t]
            xi, xf, sc, lab = _rows(rs, b)
            assert np.array_equal(xi, Wk[0][ix].reshape(-1, 4)) and [int(v) for v in lab] == sn, f"net {net} frame {t} R"
            assert np.array_equal(_bits(xf), _bits(Wk[1][ix].reshape(-1, 4))) and np.array_equal(_bits(sc), _bits(Wk[2][ix]))


def _arrays(lists):
    cap = max(1, max(len(b) for b in lists))
    xy = np.zeros((len(lists), cap, 4), np.int32)
    for i, b in enumerate(lists):
        xy[i, :len(b)] = np.asarray(b, np.int32).reshape(-1, 4)
    return xy, np.asarray([len(b) for b in lists], np.int32)


def _run(ctx, clip, ref, plates, render):
    """The stream as two calls of two frames: lists and pixels."""
    assert ctx.frames_per_call() == 2
    for t0 in (0, 2):
        fr = clip["frames"][t0:t0 + 2]
        out, faces, pl = ctx.process(fr, flags=_flags(plates))
        _check_lists(ctx, ref, t0, 2, faces, pl, plates)
        want = render(ctx, fr, ref["B"][t0:t0 + 2])
        np.testing.assert_array_equal(out, want, err_msg=f"frames {t0}, {t0 + 1}")


def _oracle_mosaic(ctx, fr, B):
    return np.stack([omosaic.mosaic_frame(f, b, 8) for f, b in zip(fr, B)])


def test_faces_end_to_end(face_ctx_factory, clip):
    """Faces tiled and rescued at LOW = 0.2 (all five figures below hold on these frames), hold = 1, two calls
    of two frames: D, W, R with since and the pixelated frames equal the reference; and the smooth blur with
    cells = 8 of the same lists."""
    ref = _reference(clip, "faces", False)
    fig = _figures(ref, clip, 0)
    assert fig["weak"] > 0 and fig["rescued"] > 0 and fig["weak_not_rescued"] > 0 and fig["weak_from_tiles"] > 0
    assert fig["weak"] < fig["input_weak"]                  # the merge removed weak boxes
    kw = dict(**TILED, rescue_tiles=True, rescue=LOW, rescue_span=SPAN, hold=HOLD)
    _run(_ctx(face_ctx_factory, **kw), clip, ref, False, _oracle_mosaic)
    _run(_ctx(face_ctx_factory, **kw, blur="gaussian", cells=8), clip, ref, False,
         lambda c, fr, B: c.smooth(fr, *_arrays(B)))


@pytest.mark.parametrize("nets", ["plates", "both"])
def test_plates_end_to_end(face_ctx_factory, clip, nets):
    """tile_nets="plates" with plate_rescue alone (merged plates beside untiled faces without weak boxes: the
    split two-forward plate rows) and "both" with both lows."""
    lows = (0.0, PLOW) if nets == "plates" else (LOW, PLOW)
    ref = _reference(clip, nets, True, lows=lows)
    fig = _figures(ref, clip, 1)
    if nets == "both":
        _figures(ref, clip, 0)
    assert fig["weak"] > 0 and fig["rescued"] > 0 and fig["weak_not_rescued"] > 0 and fig["weak_from_tiles"] > 0
    assert fig["weak"] < fig["input_weak"]
    ctx = _ctx(face_ctx_factory, **TILED, tile_nets=nets, rescue_tiles=True, rescue=lows[0], plate_rescue=PLOW,
               rescue_span=SPAN, hold=HOLD)
    _run(ctx, clip, ref, True, _oracle_mosaic)


def test_nv12_surfaces(face_ctx_factory, clip):
    """tile_surfaces: process_nv12 on the NV12 form of the stream gives the lists of the RGB run, and both
    planes are mosaic_nv12 over B."""
    ref = _reference(clip, "faces", False)
    ctx = _ctx(face_ctx_factory, **TILED, rescue_tiles=True, rescue=LOW, rescue_span=SPAN, hold=HOLD, tile_surfaces=True)
    for t0 in (0, 2):
        nv = np.ascontiguousarray(clip["nv"][t0:t0 + 2])
        out, faces, _ = ctx.process_nv12(nv)
        _check_lists(ctx, ref, t0, 2, faces, None, False)
        want = ctx.mosaic_nv12(nv, *_arrays(ref["B"][t0:t0 + 2]))
        np.testing.assert_array_equal(np.asarray(out), np.asarray(want))
        assert not np.array_equal(np.asarray(out), nv)


def test_process_lead_matches_on_E(face_ctx_factory, clip):
    """lead = 1 in a context that tiles and rescues: the blur lists are the lead reference over E (2 + 2 +
    flush), and the emitted frames their oracle mosaic."""
    ref = _reference(clip, "faces", False, hold=0)
    wantB, wantL = lr.blur_lists(ref["E"], H, W, 1, 30)
    assert sum(len(r) for r in ref["R"]) > 0 and any(v < 0 for l in wantL for v in l)
    ctx = _ctx(face_ctx_factory, **TILED, rescue_tiles=True, rescue=LOW, rescue_span=SPAN, lead=1)
    outs, B = [], []
    for t0 in (0, 2, None):
        if t0 is None:
            out = ctx.lead_flush()
        else:
            out, faces, _ = ctx.process_lead(clip["frames"][t0:t0 + 2])
            _check_lists(ctx, ref, t0, 2, faces, None, False)
        if len(out):
            rows = ctx.read_lead(len(out), "all")
            for i in range(len(out)):
                k = int(rows.count[i])
                B.append(([tuple(int(v) for v in r) for r in rows.xyxy[i, :k]], [int(v) for v in rows.label[i, :k]]))
        outs += list(out)
    assert [b for b, _ in B] == wantB and [l for _, l in B] == wantL
    for t, fr in enumerate(clip["frames"]):
        np.testing.assert_array_equal(outs[t], omosaic.mosaic_frame(fr, wantB[t], 8), err_msg=f"frame {t}")


# ---- 6. state rules in a context that runs -----------------------------------------------------------------
def test_state_rules(face_ctx_factory, clip):
    from vdmi import _lib
    ref = _reference(clip, "faces", False)
    assert len(ref["R"][1]) > 0                            # frame 1 rescues in the undisturbed stream
    ctx = _ctx(face_ctx_factory, **TILED, rescue_tiles=True, rescue=LOW, rescue_span=SPAN, hold=HOLD)
    ctx.process(clip["frames"][0:1])
    # turning the switch off with both on: refused, nothing changes -- the next frame still rescues
    with pytest.raises(_lib.VdError, match="vd_rescue.*vd_tiles") as e:
        ctx.set_rescue_tiles(False)
    assert e.value.code == _lib.VD_ERR_STATE and ctx.rescue_tiles
    ctx.process(clip["frames"][1:2])
    assert int(ctx.read_rescue(0, 1, "rescued").count[0]) == len(ref["R"][1])
    # set_tiles in a rescue context resets the rescue history: the next frame rescues nothing
    ctx.hold_reset()
    ctx.process(clip["frames"][0:1])
    ctx.set_tiles((1, 2), 20)
    ctx.set_tiles((2, 2), 20)
    ctx.process(clip["frames"][1:2])
    assert int(ctx.read_rescue(0, 1, "rescued").count[0]) == 0 and int(ctx.read_rescue(0, 1, "weak").count[0]) > 0
    # ... and so does set_tile_nets while tiling is on
    ctx.process(clip["frames"][0:1])
    ctx.set_tile_nets("both")
    ctx.set_tile_nets("faces")
    ctx.process(clip["frames"][1:2])
    assert int(ctx.read_rescue(0, 1, "rescued").count[0]) == 0
    # pending lead frames refuse the switch
    lead = _ctx(face_ctx_factory, **TILED, rescue_tiles=True, rescue=LOW, rescue_span=SPAN, lead=1)
    lead.process_lead(clip["frames"][0:1])
    assert lead.lead_pending() == 1
    rc = lead._lib.vd_rescue_tiles(lead._h, 0)
    assert rc == _lib.VD_ERR_STATE and "pending" in _lib.last_error() and lead.rescue_tiles
    lead.lead_flush()
