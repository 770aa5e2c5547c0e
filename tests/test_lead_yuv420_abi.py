"""The look-ahead hold's entry points for 4:2:0 surfaces in any layout and for 16-bit words, through the
layers, without a GPU: include/vdmi.h declares vd_process_lead_yuv420 and vd_process_lead_yuv420_16 and no
longer names them as gaps, libvdmi.so exports them, vdmi._lib binds them and Context carries the
methods. The null-context refusal shows each symbol is the real entry point."""
import ctypes
import inspect
import os

import pytest

from conftest import ROOT

ENTRIES = {"vd_process_lead_yuv420": "vd_yuv420", "vd_process_lead_yuv420_16": "vd_yuv420_16"}


def test_header_declares_the_entry_points():
    text = " ".join(open(os.path.join(ROOT, "include", "vdmi.h")).read().split()).replace(" * ", " ")   # comments as prose
    for needle in ("int vd_process_lead_yuv420(vd_ctx* ctx, const vd_yuv420* in, const vd_yuv420* out, int n, int h, int w, "
                   "int where, int flags, vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);",
                   "int vd_process_lead_yuv420_16(vd_ctx* ctx, const vd_yuv420_16* in, const vd_yuv420_16* out, int n, int h, "
                   "int w, int where, int flags, vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);",
                   "half the RGB ring"):
        assert needle in text, needle
    for gone in ("a planar form of vd_process_lead_nv12", "the look-ahead ring stays NV12",
                 "look-ahead on these surfaces (the ring stays 8-bit NV12)"):
        assert gone not in text, gone
    # what is still not offered stays named
    for still in ("tiling and the fixed Gaussian on surfaces", "4:2:2 and 4:4:4", "depth or shift conversion"):
        assert still in text, still


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_it(name):
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    assert hasattr(lib, name)
    m = ctypes.c_int(-1)
    assert getattr(lib, name)(None, None, None, 0, 2, 2, 0, 0, None, None, 0, 1, ctypes.byref(m)) == _lib.VD_ERR_ARG
    assert "null context" in _lib.last_error() and m.value == -1


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_lib_binds_it(name):
    from vdmi import _lib
    sig = {s[0]: s for s in _lib.SIGNATURES}[name]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 13
    assert sig[2][1] == sig[2][2] == ctypes.POINTER(getattr(_lib, ENTRIES[name]))
    assert sig[2][8] == sig[2][9] == ctypes.POINTER(_lib.vd_boxes)
    assert sig[2][12] == ctypes.POINTER(ctypes.c_int)


def test_context_has_the_methods():
    import vdmi
    common = ["self", "frames", "out", "faces", "plates", "flags", "flush", "layout", "out_layout", "matrix", "range", "height"]
    assert list(inspect.signature(vdmi.Context.process_lead_yuv420).parameters) == common
    sig = inspect.signature(vdmi.Context.process_lead_yuv420_16)
    assert list(sig.parameters) == common + ["depth", "shift"]
    assert sig.parameters["depth"].default == 10 and sig.parameters["shift"].default is None
    assert sig.parameters["layout"].default == "i420" and sig.parameters["flush"].default is False


def test_pending_mode_names_both_8bit_entries():
    """csrc/lead_state.h: refusals that name the pusher of pending 8-bit surfaces still contain the NV12
    entry's name (tests/test_gpu_lead_nv12.py matches on it), and 16-bit words have a mode of their own."""
    text = open(os.path.join(ROOT, "video-desensitization_amd", "csrc", "lead_state.h")).read()
    assert '"vd_process_lead_nv12 / vd_process_lead_yuv420"' in text
    assert "#define VD_LEAD_MODE_YUV16 4" in text and '"vd_process_lead_yuv420_16"' in text
