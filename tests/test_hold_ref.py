"""Box hold without a GPU: hand-derived known answers of the definition (tests/hold_ref.py,
the checker of tests/test_gpu_hold.py) on a 100 x 100 frame, and the host-only product
checks: the vd_cfg fields, the Python argument checks, the pipeline's refusal."""
import ctypes

import pytest

import hold_ref as hr

H = W = 100
A = (10, 10, 30, 30)
FAR = (60, 60, 90, 95)


def _run(seq, K, P=30, history=None):
    return hr.hold_lists(seq, H, W, K, P, history)


def test_gap_fill_and_expiry():
    """A box in t-1 and none in t: held at t with age 1, then age 2, gone at t + K."""
    B, Hd, ages, hist = _run([[A], [], [], []], K=2)
    assert B == [[A], [A], [A], []]
    assert Hd == [[], [A], [A], []] and ages == [[], [1], [2], []]
    assert hist == [[], []]


def test_chain_keeps_only_the_latest_sighting():
    """The same box at t-2 and t-1, missing at t: the age-2 copy matches D_{t-1}."""
    B, Hd, ages, _ = _run([[A], [A], []], K=2)
    assert Hd[2] == [A] and ages[2] == [1]
    assert Hd[1] == [] and B[2] == [A]


def test_box_two_frames_back():
    B, Hd, ages, _ = _run([[A], [FAR], []], K=2)
    assert Hd[1] == [A] and ages[1] == [1]            # FAR does not match A
    assert Hd[2] == [FAR, A] and ages[2] == [1, 2]
    assert _run([[A], [FAR], []], K=1)[1][2] == [FAR]  # K = 1 looks one frame back only


def test_threshold_is_inclusive():
    """(0,0,10,10) against (0,0,10,3): 30 / 100 matches at P = 30; (0,0,9,3): 27 / 100 does not."""
    big = (0, 0, 10, 10)
    assert hr.match(big, (0, 0, 10, 3), 30) and not hr.match(big, (0, 0, 9, 3), 30)
    assert _run([[big], [(0, 0, 10, 3)]], K=1)[1][1] == []
    assert _run([[big], [(0, 0, 9, 3)]], K=1)[1][1] == [big]


def test_boxes_empty_after_clipping_are_never_held_and_never_match():
    empties = [(200, 200, 240, 230), (60, 30, 60, 50), (-50, -50, -10, -10)]
    assert [hr.clip_box(b, H, W) for b in empties] == [None, None, None]
    B, Hd, ages, _ = _run([empties, []], K=2)
    assert B[0] == empties and Hd[1] == [] and B[1] == []
    # as references they hide nothing: (60,30,60,50) lies inside the candidate
    cand = (50, 20, 70, 60)
    assert _run([[cand], empties], K=1)[1][1] == [cand]
    # a held box is stored unclipped; its clipped form is what is compared
    out = (-5, -5, 10, 10)
    assert _run([[out], []], K=1)[1][1] == [out]
    assert _run([[out], [(0, 0, 10, 10)]], K=1, P=100)[1][1] == []


def test_p_100_and_p_1():
    c = (0, 0, 10, 10)
    assert _run([[c], [(0, 0, 10, 10)]], K=1, P=100)[1][1] == []        # identical
    assert _run([[c], [(0, 0, 10, 9)]], K=1, P=100)[1][1] == [c]        # 90 / 100
    # inter 10, union 190: a match at P = 1 (1000 >= 190), none at P = 30 (1000 < 5700)
    assert _run([[c], [(9, 0, 19, 10)]], K=1, P=1)[1][1] == []
    assert _run([[c], [(9, 0, 19, 10)]], K=1, P=30)[1][1] == [c]
    # touching boxes share no area: never a match
    assert _run([[c], [(10, 0, 20, 10)]], K=1, P=1)[1][1] == [c]


def test_overlapping_boxes_of_one_frame_are_both_held():
    a, b = (10, 10, 30, 30), (12, 12, 32, 32)
    assert hr.match(a, b, 30)
    _, Hd, ages, _ = _run([[a, b], []], K=1)
    assert Hd[1] == [a, b] and ages[1] == [1, 1]        # candidates are judged on their own


def test_order_is_age_then_list_order():
    x1, x2, y1, y2 = (0, 0, 10, 10), (20, 0, 30, 10), (40, 0, 50, 10), (60, 0, 70, 10)
    B, Hd, ages, _ = _run([[x2, x1], [y2, y1], [FAR]], K=2)
    assert Hd[2] == [y2, y1, x2, x1] and ages[2] == [1, 1, 2, 2]
    assert B[2] == [FAR, y2, y1, x2, x1]


def test_history_carries_across_calls():
    seq = [[A], [FAR], [], [(0, 0, 5, 5)], []]
    one = _run(seq, K=3)
    for cut in (1, 2, 4):
        first = _run(seq[:cut], K=3)
        second = _run(seq[cut:], K=3, history=first[3])
        assert [first[i] + second[i] for i in range(3)] == list(one[:3]), cut
        assert second[3] == one[3]


# ---- host-only product checks ---------------------------------------------------------

def test_cfg_mirror_names_hold_fields_at_the_reserved_offsets():
    from vdmi import _lib
    fields = list(_lib.vd_cfg._fields_)
    names = [f[0] for f in fields]
    i = names.index("hold_frames")
    assert names[i:i + 3] == ["hold_frames", "hold_iou_pct", "reserved"]

    class Old(ctypes.Structure):      # the layout before the fields were named: reserved[3]
        _fields_ = fields[:i] + [("reserved", ctypes.c_int32 * 3)]
    assert ctypes.sizeof(_lib.vd_cfg) == ctypes.sizeof(Old)
    assert _lib.vd_cfg.hold_frames.offset == Old.reserved.offset
    assert _lib.vd_cfg.hold_iou_pct.offset == Old.reserved.offset + 4
    assert _lib.vd_cfg.reserved.offset == Old.reserved.offset + 8


def test_default_cfg_leaves_hold_off():
    from vdmi import _lib
    c = _lib.default_cfg()
    assert c.hold_frames == 0 and c.hold_iou_pct == 0
    assert _lib.load().vd_abi_version() == 2


@pytest.mark.parametrize("kw", [dict(hold=9), dict(hold=-1), dict(hold=1, hold_iou_pct=101),
                                dict(hold=1, hold_iou_pct=0)])
def test_context_refuses_bad_hold_settings_without_a_gpu(kw):
    import vdmi
    with pytest.raises(ValueError, match="hold"):
        vdmi.Context(**kw)


def test_pipeline_refuses_hold_with_foreign_detectors(tmp_path):
    from vdmi.pipeline import batch_process_images
    (tmp_path / "in").mkdir()
    with pytest.raises(ValueError, match="hold"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), hold=2)
    with pytest.raises(ValueError, match="hold"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), hold=9)
