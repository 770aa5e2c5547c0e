"""The look-ahead hold's NV12 entry point through the layers, without a GPU: include/vdmi.h declares
vd_process_lead_nv12, libvdmi.so exports it, vdmi._lib binds it and Context carries
process_lead_nv12. The null-context refusal shows the symbol is the real entry point."""
import ctypes
import inspect
import os

from conftest import ROOT


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    for needle in ("int vd_process_lead_nv12(vd_ctx* ctx, const vd_nv12* in, const vd_nv12* out, int n, int h, int w, "
                   "int where, int flags,",
                   "vd_boxes* faces, vd_boxes* plates, int out_cap, int flush, int* n_out);",
                   "half the RGB ring"):
        assert needle in text, needle
    assert "has no NV12 entry point" not in text


def test_library_exports_it():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    assert hasattr(lib, "vd_process_lead_nv12")
    m = ctypes.c_int(-1)
    assert lib.vd_process_lead_nv12(None, None, None, 0, 2, 2, 0, 0, None, None, 0, 1, ctypes.byref(m)) == _lib.VD_ERR_ARG
    assert "null context" in _lib.last_error() and m.value == -1


def test_lib_binds_it():
    from vdmi import _lib
    sig = {s[0]: s for s in _lib.SIGNATURES}["vd_process_lead_nv12"]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 13
    assert sig[2][1] == sig[2][2] == ctypes.POINTER(_lib.vd_nv12)
    assert sig[2][8] == sig[2][9] == ctypes.POINTER(_lib.vd_boxes)


def test_context_has_process_lead_nv12():
    import vdmi
    params = list(inspect.signature(vdmi.Context.process_lead_nv12).parameters)
    assert params == ["self", "frames", "out", "faces", "plates", "flags", "flush", "matrix", "range", "height"]
