"""Box hold with the linear motion model, without a GPU: hand-derived known answers of the
definition (tests/hold_motion_ref.py, the checker of tests/test_gpu_hold_motion.py) on a
100 x 100 frame, its properties on random sequences, and the host-only product checks: the
exported setter and the Python argument checks."""
import pytest

import hold_motion_ref as mr
import hold_ref as hr
from test_gpu_hold import _random_sequence

H = W = 100

WORKED = {   # name: (D_0, D_1, H_2, H_3) with D_2 = D_3 = [], K = 2, P = 30
    "moving": ((10, 10, 30, 30), (14, 10, 34, 30), (14, 10, 38, 30), (14, 10, 42, 30)),
    "shrinking": ((10, 10, 30, 30), (16, 10, 24, 30), (16, 10, 24, 30), (16, 10, 24, 30)),   # q inverted: hull = b
    "leaving": ((2, 40, 22, 60), (-4, 40, 16, 60), (-4, 40, 16, 60), (-4, 40, 16, 60)),      # clipped velocity
}


def _run(seq, K, P=30, history=None):
    return mr.hold_motion_lists(seq, H, W, K, P, history)


@pytest.mark.parametrize("name", sorted(WORKED))
def test_worked_examples(name):
    d0, d1, h2, h3 = WORKED[name]
    B, Hd, ages, _, stored = _run([[d0], [d1], [], []], K=2)
    assert Hd == [[], [], [h2], [h3]] and ages == [[], [], [1], [2]]
    assert stored == [[], [], [d1], [d1]]
    assert B[2] == [h2] and B[3] == [h3]


def test_tie_goes_to_the_lowest_index():
    """Two predecessors one step left and right of c: equal inter and union."""
    c, left, right = (10, 10, 30, 30), (8, 10, 28, 30), (12, 10, 32, 30)
    assert mr.iou_terms(c, left) == mr.iou_terms(c, right)
    assert _run([[right, left], [c], []], K=1)[1][2] == [(8, 10, 30, 30)]      # v = c - right = -2
    assert _run([[left, right], [c], []], K=1)[1][2] == [(10, 10, 32, 30)]     # v = c - left = +2


def test_best_iou_not_first_match():
    c, far, near = (10, 10, 30, 30), (4, 10, 24, 30), (9, 10, 29, 30)
    assert hr.match(c, far, 30) and hr.match(c, near, 30)
    assert _run([[far, near], [c], []], K=1)[1][2] == [(10, 10, 31, 30)]
    assert _run([[near, far], [c], []], K=1)[1][2] == [(10, 10, 31, 30)]
    assert _run([[far], [c], []], K=1)[1][2] == [(10, 10, 36, 30)]


def test_no_predecessor():
    a = (10, 10, 30, 30)
    assert _run([[a], [], []], K=2)[1] == [[], [a], [a]]                        # sighted in the stream's first frame
    assert _run([[(60, 60, 90, 95)], [a], []], K=1)[1][2] == [a]               # nothing in D_0 matches
    assert _run([[(200, 200, 240, 230)], [a], []], K=1)[1][2] == [a]           # empty after clipping
    # the frame before the sighting comes from the history of an earlier call
    first = _run([[(6, 10, 26, 30)]], K=1)
    assert len(first[3]) == 1
    assert _run([[a], []], K=1, history=first[3])[1][1] == [(10, 10, 34, 30)]
    assert _run([[a], []], K=1)[1][1] == [a]


def test_history_carries_across_calls():
    seq, h, w = _random_sequence(11)
    K, P = 3, 30
    one = mr.hold_motion_lists(seq, h, w, K, P)
    for cut in (1, 2, 5, 11):
        first = mr.hold_motion_lists(seq[:cut], h, w, K, P)
        second = mr.hold_motion_lists(seq[cut:], h, w, K, P, history=first[3])
        assert [first[i] + second[i] for i in range(3)] == list(one[:3]), cut
        assert second[3] == one[3] and len(one[3]) == K + 1


@pytest.mark.parametrize("P", [1, 30, 100])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_properties_on_random_sequences(K, P):
    seq, h, w = _random_sequence(100 * K + P)
    B0, H0, ages0, _ = hr.hold_lists(seq, h, w, K, P)
    B, Hm, ages, _, stored = mr.hold_motion_lists(seq, h, w, K, P)
    assert stored == H0 and ages == ages0                                   # same membership and ages
    assert [len(b) for b in B] == [len(b) for b in B0]
    moved = 0
    for t in range(len(seq)):
        assert B[t][:len(seq[t])] == seq[t]
        for m, s in zip(Hm[t], H0[t]):
            assert m[0] <= s[0] and m[1] <= s[1] and m[2] >= s[2] and m[3] >= s[3]   # held contains stored
            assert all(abs(v) <= 9 * 32768 for v in m)
            moved += m != s
    if P == 100:
        assert moved == 0                    # a predecessor equals c: v = 0
    else:
        assert moved >= 10


# ---- host-only product checks ---------------------------------------------------------

def test_vd_hold_motion_is_exported_and_bound():
    import ctypes
    from vdmi import _lib
    lib = _lib.load()
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert "vd_hold_motion" in sig
    assert lib.vd_hold_motion.argtypes == [ctypes.c_void_p, ctypes.c_int] and lib.vd_hold_motion.restype == ctypes.c_int
    assert (_lib.VD_HOLD_MOTION_OFF, _lib.VD_HOLD_MOTION_LINEAR) == (0, 1)
    assert lib.vd_hold_motion(None, 1) == _lib.VD_ERR_ARG                   # a null context is refused, not run
    assert lib.vd_abi_version() == 2


def test_context_refuses_motion_without_hold():
    import vdmi
    with pytest.raises(ValueError, match="hold_motion"):
        vdmi.Context(hold=0, hold_motion=True)


def test_detector_and_pipeline_refuse_motion_without_hold(tmp_path):
    import vdmi
    from vdmi.pipeline import batch_process_images
    with pytest.raises(ValueError, match="hold_motion"):
        vdmi.Retinaface(weights="random", hold=0, hold_motion=True)
    (tmp_path / "in").mkdir()
    with pytest.raises(ValueError, match="hold_motion"):
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), hold=0,
                             hold_motion=True)
    with pytest.raises(ValueError, match="hold"):                           # foreign detectors, as without motion
        batch_process_images(str(tmp_path / "in"), str(tmp_path / "out"), object(), object(), hold=2,
                             hold_motion=True)
