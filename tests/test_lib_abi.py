"""CPU-side checks of the C-ABI boundary: libvdmi.so loads, exports every entry
point include/vdmi.h declares, and its host-only calls behave (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header_functions():
    src = open(os.path.join(ROOT, "include", "vdmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vdt?_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    import vdmi
    from vdmi import _lib
    lib = vdmi.load()
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"libvdmi.so does not export {n}"
    bound = {s[0] for s in _lib.SIGNATURES}
    assert set(names) == bound, set(names) ^ bound


def test_struct_layout_matches_header(tmp_path):
    """ctypes mirrors of vd_cfg / vd_boxes / vdt_op have the C compiler's size and field offsets."""
    import shutil
    import subprocess
    from vdmi import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    fields = {"vd_cfg": [f[0] for f in _lib.vd_cfg._fields_], "vd_boxes": [f[0] for f in _lib.vd_boxes._fields_],
              "vdt_op": [f[0] for f in _lib.vdt_op._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vdmi.h"', "int main(void){"]
    for st, fl in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f in fl:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for st, cls in (("vd_cfg", _lib.vd_cfg), ("vd_boxes", _lib.vd_boxes), ("vdt_op", _lib.vdt_op)):
        assert int(out[st]) == ctypes.sizeof(cls)
        for f in fields[st]:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, f


def test_default_cfg_and_version():
    from vdmi import _lib
    lib = _lib.load()
    assert lib.vd_abi_version() == 2
    c = _lib.default_cfg()
    assert (c.input_h, c.input_w, c.max_batch) == (640, 640, 64)          # combine_detect.py:860, config.ini:35
    assert abs(c.confidence - 0.5) < 1e-9 and c.nms_iou == 0.4 and c.mosaic_level == 8


def test_errors_are_reported_not_raised_through_abi():
    from vdmi import _lib
    lib = _lib.load()
    assert lib.vd_create(None, 0, None) == _lib.VD_ERR_ARG
    assert "null" in _lib.last_error()
    assert lib.vd_detect(None, None, 0, 0, 0, 0, 0, None) == _lib.VD_ERR_ARG
    assert lib.vd_destroy(None) == _lib.VD_OK


def test_check_raises_typed_errors():
    from vdmi import _lib
    with pytest.raises(_lib.VdCapacityError):
        _lib.check(_lib.VD_ERR_CAPACITY)
    with pytest.raises(_lib.VdError):
        _lib.check(_lib.VD_ERR_ARG)


def test_host_boxes_struct():
    from vdmi import _lib
    hb = _lib.HostBoxes(3, 5)
    s = hb.struct()
    assert s.cap == 5 and s.where == _lib.VD_HOST and s.count == hb.count.ctypes.data
    hb.count[:] = [2, 0, 9]
    assert hb.frame(0)[0].shape == (2, 4) and hb.frame(2)[0].shape == (5, 4)


# ---- boundary hardening (GPU: a context needs a device) -------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["x6_dbg", "block32_dbg", "mosaic_copy", "face_group_lag", "plate_prio",
                                  "plate_cus", "x6_tail", "x6_slots", "x6_adepth", "x6_halo_n64",
                                  "x6_tr_epi"])
def test_set_option_refuses_debug_and_removed_switches(gpu, name):
    """The timing-only switches that skip work (wrong results) are not vd_set_option
    names -- only the test entry vdt_set_debug takes them -- and the dead experiment
    switches are gone."""
    import vdmi
    from vdmi import _lib
    ctx = vdmi.Context(precision="fp32", max_batch=1)
    try:
        with pytest.raises(_lib.VdError, match="unknown option"):
            ctx.set_option(name, 1)
        if name.endswith("_dbg"):
            ctx.set_debug(name, 0)
        else:
            with pytest.raises(_lib.VdError, match="unknown debug switch"):
                ctx.set_debug(name, 0)
        ctx.set_option("face_groups", 2)              # a production switch still takes
    finally:
        ctx.close()


@pytest.mark.gpu
def test_set_option_refuses_retired_gemm_loop_mode(gpu):
    """x6_gemm_uni keeps 0 (the general K loop) and 2 (the one-barrier 1x1 loop); the
    two-barrier uniform loop (1) is gone and vd_set_option says so."""
    import vdmi
    from vdmi import _lib
    ctx = vdmi.Context(precision="fp32", max_batch=1)
    try:
        with pytest.raises(_lib.VdError, match="x6_gemm_uni must be 0 or 2"):
            ctx.set_option("x6_gemm_uni", 1)
        ctx.set_option("x6_gemm_uni", 0)
        ctx.set_option("x6_gemm_uni", 2)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_process_refuses_overlapping_mosaic_output(gpu):
    """vd_process with VD_PROC_MOSAIC on device frames is out of place
    (combine_detect.py:142 blurs a copy, :247-249 reads each previous box's output):
    out == in, or out overlapping in by part of a frame, is VD_ERR_ARG -- the fused
    output pass would gather cell colours from pixels other workgroups already
    rewrote. vd_mosaic refuses the same. A separate output buffer works."""
    import torch
    import vdmi
    from vdmi import _lib, synth, weights
    fr = torch.from_numpy(synth.frames(2, 120, 160, seed=3)).cuda()
    ctx = vdmi.Context(precision="fp32", max_batch=2)
    try:
        ctx.load_weights(0, weights.retinaface_state_dict(0))
        with pytest.raises(_lib.VdError, match="out-of-place"):
            ctx.process(fr, out=fr)
        big = torch.zeros((3, 120, 160, 3), dtype=torch.uint8, device="cuda")
        big[:2] = fr
        with pytest.raises(_lib.VdError, match="out-of-place"):
            ctx.process(big[:2], out=big[1:])                # shifted by one frame: overlaps
        faces = _lib.HostBoxes(2, 4)
        faces.count[:] = [1, 0]
        faces.xyxy[0, 0] = [10, 10, 60, 50]
        with pytest.raises(_lib.VdError, match="out-of-place"):
            _mosaic_call(ctx, big[:2], big[1:], faces)
        _mosaic_call(ctx, big[:2], torch.empty_like(fr), faces)          # separate output: fine
        out, _, _ = ctx.process(fr)                          # out of place: fine
        assert out.shape == fr.shape
        torch.cuda.synchronize()
    finally:
        ctx.close()


def _mosaic_call(ctx, src, dst, boxes):
    """vd_mosaic on device frames through the raw ABI (src / dst torch uint8 [n,h,w,3])."""
    import ctypes
    from vdmi import _lib
    n, h, w, _ = src.shape
    s = boxes.struct()
    _lib.check(ctx._lib.vd_mosaic(ctx._h, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n, h, w,
                                  w * 3, _lib.VD_DEVICE, ctypes.byref(s), 8, _lib.VD_MOSAIC_OUT_OF_PLACE))
